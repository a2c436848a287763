"""The two yardsticks of the exact-f32 GEMM (csrc/gemm.hip), in numpy, for tests/test_gpu_f32_routes.py.

  * fma32 / chain_product: the raw product restated as the float32 fused multiply-add chain the kernel's header claims -- per output
    element one chain from zero in ascending k for every K chunk of the split plan, then float32 additions of the chunks in split order
    from zero, as k_splitk_reduce does.  Python 3.10 has no math.fma; fma32 builds one from float64 pieces (proved against
    fractions.Fraction in tests/test_f32_chain_host.py).
  * gemm_ref: float64 result of the product and the fused epilogue with a per-element bound on |float32 kernel - float64|.

Operands are held to the NORMAL float32 range (no subnormal operand, product or sum, no overflow): fma32's float64 pieces are exact
there, and the matrix cores' treatment of subnormals is not part of the claim."""
import numpy as np

U = 2.0 ** -24


def fma32(a, b, c):
    """round_to_float32(a b + c) with ONE rounding, elementwise over float32 arrays (broadcast).
      * a b is exact in float64: two 24-bit significands give at most 48 bits, and the exponent range of float64 holds every product of
        two float32;
      * s = fl64(p + c) with its rounding error e by TwoSum (Knuth: exact for any two float64, no overflow here);
      * round to odd: when e != 0 the true sum lies strictly between s and its neighbour towards e; of those two float64 exactly one has
        an odd significand -- s itself, or else that neighbour.  The result carries 53 bits whose last is a sticky bit;
      * one cast to float32 (round to nearest even).  With 53 >= 24 + 2 bits the sticky bit decides every tie and near-tie as the
        infinitely precise sum would (Boldo & Melquiond, "Emulation of FMA and correctly rounded sums", 2008): no double rounding."""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), np.broadcast(p, c).shape)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def chain_product(a, b, k_chunk):
    """(M, K) x (K, N) float32 -> (M, N) float32 by the claimed arithmetic: per chunk of k_chunk columns of a, acc = fma32(a[:, k], b[k], acc)
    from zero in ascending k; one chunk is the result itself, more are added in float32 in chunk order from zero (0 + x = x exactly)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    M, K = a.shape
    out = None
    for k0 in range(0, K, k_chunk):
        acc = np.zeros((M, b.shape[1]), np.float32)
        for k in range(k0, min(K, k0 + k_chunk)):
            acc = fma32(a[:, k:k + 1], b[k:k + 1, :], acc)
        out = acc if out is None else (out + acc).astype(np.float32)
    return out


def fold_operand(a, stats, lens, slope):
    """The folded InstanceNorm + LeakyReLU operand in float64 from the float32 inputs: lrelu((a - mean) rstd) with the statistics of the
    row's cloud.  -> (a', relative operand error).  The kernel takes (a - mean) (U), the product with rstd (U) and, below zero, the
    product with the slope (U): three roundings, each relative to the value at hand, and no rounding changes a sign, so the branch taken
    is the exact one: |a'^ - a'| <= ((1 + U)^3 - 1) |a'|."""
    a64 = np.asarray(a, dtype=np.float64)
    st = np.asarray(stats, dtype=np.float64)
    seg = np.repeat(np.arange(len(lens)), lens)
    v = (a64 - st[seg, :, 0]) * st[seg, :, 1]
    return np.where(v > 0, v, v * float(np.float32(slope))), (1 + U) ** 3 - 1


def gemm_ref(a, b, s_eff, bias=None, row_div=None, residual=None, relu=False, a_rel=0.0):
    """float64 C = epilogue(A B) and the per-element bound on |kernel - C|.  a: the float64 operand (fold_operand's for a folded launch,
    with its relative error a_rel).

    The raw product.  An element is sum_k a_k b_k, computed as chunks of fma chains plus s_eff - 1 float32 additions (the first addition
    of the reduction, to zero, is exact).  A term passes through at most K roundings of its chain and the s_eff - 1 of the reduction, so
    with n = K + s_eff - 1 the classical bound (Higham, Accuracy and Stability, section 3.1) is gamma_n (|A| |B|)_ij, gamma_n =
    n U / (1 - n U).  While n^2 U <= 1 (asserted; n <= 4096, so n U <= 1 / 2): gamma_n = n U + n^2 U^2 / (1 - n U) <= n U + U / (1 - n U)
    <= (n + 2) U.  The float64 reference itself is off by at most gamma64_K (|A| |B|)_ij < 2^-17 U (|A| |B|)_ij, inside one more U.
    Hence the bound (K + c) U (|A| |B|)_ij with c = (s_eff - 1) + 3.  A folded operand with relative error a_rel adds
    a_rel (1 + gamma_n) (|A'| |B|)_ij <= a_rel (1 + 2^-11) (|A'| |B|)_ij.

    The epilogue, each step rounding once (IEEE division, addition; the maximum with zero is exact and 1-Lipschitz):
      q = acc / row_div:  e <- e / |row_div| + U (|q| + e / |row_div|)
      t = q + bias:       e <- e + U (|t| + e)
      relu:               e unchanged
      y = t + residual:   e <- e + U (|y| + e)
    -> (C float64, bound, raw product float64, raw bound)."""
    a = np.asarray(a, dtype=np.float64)
    b64 = np.asarray(b, dtype=np.float64)
    K = a.shape[1]
    n = K + s_eff - 1
    assert n * n * U <= 1.0
    raw = a @ b64
    mag = np.abs(a) @ np.abs(b64)
    c = (s_eff - 1) + 3
    e = (K + c) * U * mag + a_rel * (1 + 2.0 ** -11) * mag
    raw_bound = e
    y = raw
    if row_div is not None:
        d = np.abs(np.asarray(row_div, dtype=np.float64))[:, None]
        y = y / np.asarray(row_div, dtype=np.float64)[:, None]
        e = e / d + U * (np.abs(y) + e / d)
    if bias is not None:
        y = y + np.asarray(bias, dtype=np.float64)[None, :]
        e = e + U * (np.abs(y) + e)
    if relu:
        y = np.maximum(y, 0.0)
    if residual is not None:
        y = y + np.asarray(residual, dtype=np.float64)
        e = e + U * (np.abs(y) + e)
    return y, e, raw, raw_bound
