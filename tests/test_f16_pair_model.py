"""CPU: a numpy model of the f16 pair operand format (defined in regtr_amd/csrc/mfma_operands.h: rg_split2_f16, RG_F16_SCALE,
rg_fold_low; used by csrc/gemm_x3.hip FMT = 1 and csrc/attention.hip precision 3) --
x = h0 + h1 / 2048 with h0 = f16(x), h1 = f16((x - h0) * 2048); a w = a0 w0 + (a0 w1 + a1 w0) / 2048 -- against float64, next to the
bf16 splits it replaces.  Pins the two design decisions: (1) three f16 terms are float32-grade (the three-term bf16 split is not);
(2) the 2048 scale is needed -- without it the residual plane of anything below 0.12 is an f16 subnormal, and hardware that flushes
those (or rounds them coarsely) loses the low half."""
import numpy as np


def _bf16(x):
    u = x.astype(np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7fff)) & 0xffff0000).view(np.float32)


def _f16(x, ftz):
    h = x.astype(np.float16)
    if ftz:
        h = np.where(np.abs(h.astype(np.float32)) < 6.103515625e-5, np.float16(0), h)
    return h.astype(np.float32)


def _mm(a, b):
    return a.astype(np.float64) @ b.astype(np.float64)        # products of 11-bit (8-bit) operands are exact; accumulate exactly


def _errors(scale, ftz, seed=0):
    rng = np.random.default_rng(seed)
    M, K, N, S = 256, 960, 64, 2048.0
    A = (rng.standard_normal((M, K)) * scale * np.exp(rng.standard_normal((M, K)))).astype(np.float32)
    W = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    ref = _mm(A, W)
    sc = np.abs(ref).max()
    a0, w0 = _bf16(A), _bf16(W)
    a1, w1 = _bf16(A - a0), _bf16(W - w0)
    a2, w2 = _bf16(A - a0 - a1), _bf16(W - w0 - w1)
    bf16x3 = _mm(a2, w0) + _mm(a1, w1) + _mm(a0, w2) + _mm(a1, w0) + _mm(a0, w1) + _mm(a0, w0)
    bf16x2 = _mm(a1, w0) + _mm(a0, w1) + _mm(a0, w0)
    h0, v0 = _f16(A, ftz), _f16(W, ftz)
    h1, v1 = _f16((A - h0) * S, ftz), _f16((W - v0) * S, ftz)
    pair = _mm(h0, v0) + (_mm(h0, v1) + _mm(h1, v0)) / S
    g1, u1 = _f16(A - h0, ftz), _f16(W - v0, ftz)
    unscaled = _mm(h0, v0) + _mm(h0, u1) + _mm(g1, v0)
    err = lambda y: float(np.abs(y - ref).max() / sc)
    return {'bf16x3': err(bf16x3), 'bf16x2': err(bf16x2), 'pair': err(pair), 'unscaled': err(unscaled)}


def test_f16_pair_is_float32_grade_and_needs_its_scale():
    for scale in (1.0, 1e-3, 30.0):
        for ftz in (False, True):
            e = _errors(scale, ftz)
            assert e['pair'] < 5e-6, (scale, ftz, e)                       # float32-grade even if subnormals were flushed (measured on MI355X,
                                                                           # tests/test_gpu_ops.py: 2.8e-7 ... 5e-7 -- the hardware keeps them)
            assert e['pair'] < e['bf16x2'] / 2, (scale, ftz, e)            # the three-term bf16 split is 2^-16 per product
            assert e['bf16x3'] < 1e-7, (scale, ftz, e)
        assert _errors(scale, True)['unscaled'] > 1e-4, scale             # subnormal residuals flushed: the low plane is gone
    assert _errors(1.0, False)['pair'] < 2e-7                             # subnormals honoured: 22 bits
