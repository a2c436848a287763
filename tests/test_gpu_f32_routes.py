"""GPU: the exact-f32 GEMM (csrc/gemm.hip) in every instantiation and regime its launcher can reach, and the small forward kernels that had
one loose case or only end-to-end coverage (k_layernorm, k_posemb_sine, k_add of csrc/norm.hip; k_overlap_avgpool, k_nearest_in_radius of
csrc/preprocess.hip).

Every parametrized GEMM case carries the route tests/dispatch.py derives for it (route_gemm_f32: instantiation + regime tags);
tests/test_dispatch_routes.py cross-checks the routes and fails when an instantiation of dispatch.F32_KERNELS, or one of the regimes
around them, is reached by no case.  Two yardsticks (tests/f32_chain_ref.py): float64 with a per-element bound (K + c) U (|A| |B|)_ij plus
the epilogue's roundings, on operands whose rows and columns span 10^-3 .. 10^3 so that no flat tolerance would do; and, for the raw
product, the float32 fma chain in ascending k -- one chain per split-K chunk, the chunks added in float32 in split order -- whose bit
patterns the kernel must reproduce.  Outputs go into NaN-filled windows inside sentinel-filled buffers.  Every test prints its worst
err / bound; docs/PARITY.md has them."""
import itertools

import numpy as np
import pytest
import torch

from tests import cross_encoder_grads_ref as CR
from tests import dispatch
from tests import f32_chain_ref as FR

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
SENTINEL = 777.0
GUARD = 3
SLOPE = 0.1


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _ratio(err, bound):
    """max err / bound; a zero bound (exact zeros) admits a zero error only."""
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max())


def _window(rows, cols, ld):
    """A (rows + GUARD, ld) sentinel buffer whose [:rows, :cols] window is NaN: what the kernel must overwrite, and all it may touch."""
    buf = torch.full((rows + GUARD, ld), SENTINEL, device='cuda')
    buf[:rows, :cols] = float('nan')
    return buf


def _check_window(buf, rows, cols):
    torch.cuda.synchronize()
    got = buf[:rows, :cols].cpu().numpy()
    assert np.all(np.isfinite(got)), 'an output element was not written (or is not finite)'
    assert torch.all(buf[rows:] == SENTINEL) and torch.all(buf[:rows, cols:] == SENTINEL), 'written outside the output window'
    return got


# ------------------------------------------------------------------------------------------------ regtr_gemm_f32
FOLD_LENS = [33, 1, 0, 64, 7, 200]                      # boundaries inside the first 64- and 128-row tiles, one-cloud tiles after them
FOLD_M = sum(FOLD_LENS)


def _r(M, N, K, view='plain', lens=None):
    """The route of a case.  view: 'plain' contiguous operands; 'off1' A one float into a wider buffer (data_ptr % 16 == 4, lda = K + 4);
    'strided' lda = K + 8 (alignment kept), ldc = N + 5, ldr = N + 3."""
    lda = {'plain': K, 'off1': K + 4, 'strided': K + 8}[view]
    return dispatch.route_gemm_f32(M, N, K, lda=lda, a_aligned16=view != 'off1', lens=lens)


UNSPLIT_KS = (1, 3, 4, 16, 31, 32, 33, 65)
UNSPLIT_NS = (1, 3, 32, 33, 64, 65)
EDGE_MS = (1, 63, 64, 65, 127, 128, 129)
GEMM_SHAPES = (
    # split-K: every instantiation; S_eff < S with a short last chunk; the existing deep case
    [(300, 32, 1030, 'plain'), (300, 32, 1024, 'plain'), (300, 3, 640, 'plain'), (130, 50, 515, 'plain'), (130, 64, 1030, 'off1'),
     (130, 1024, 3840, 'plain'), (130, 64, 1024, 'strided'), (300, 1, 640, 'strided')]
    # unsplit: K below a float4, at and around one 32-deep tile, two and three tiles; thin and wide outputs, aligned and not
    + [(129, N, K, 'plain') for K in UNSPLIT_KS for N in UNSPLIT_NS]
    # two and three full tiles on the float4 paths
    + [(129, N, K, 'plain') for K in (64, 96) for N in (3, 32, 64)]
    # the tile edges of both tiles (128 x 32 and 64 x 64), three k tiles with a one-element tail
    + [(M, N, 65, 'plain') for M in EDGE_MS[:-1] for N in (3, 32, 33, 64)]
    # strided operands; A off 16-byte alignment on both tiles
    + [(129, 32, 64, 'strided'), (129, 64, 64, 'strided'), (65, 3, 32, 'strided'), (129, 32, 64, 'off1'), (129, 64, 64, 'off1'),
       (130, 33, 96, 'off1')])
GEMM_CASES = [(M, N, K, view, _r(M, N, K, view)) for M, N, K, view in GEMM_SHAPES]
FOLD_CASES = [(N, K, _r(FOLD_M, N, K, lens=FOLD_LENS)) for N in (32, 64) for K in (64, 67, 640)]


def _operands(rng, M, N, K):
    """Rows of A and columns of B scaled by 10^(-3 .. 3): elements of one product differ by up to 10^12, all far inside the normal range."""
    rs = 10.0 ** rng.uniform(-3, 3, (M, 1))
    cs = 10.0 ** rng.uniform(-3, 3, (1, N))
    a = (rng.standard_normal((M, K)) * rs).astype(F32)
    b = (rng.standard_normal((K, N)) * cs).astype(F32)
    scale = rs * cs * np.sqrt(K)
    bias = (rng.standard_normal(N) * cs[0] * np.sqrt(K)).astype(F32)
    div = rng.integers(1, 40, M).astype(F32)
    res = (rng.standard_normal((M, N)) * scale).astype(F32)
    return a, b, bias, div, res


def _a_view(a, view):
    M, K = a.shape
    if view == 'plain':
        return _dev(a)
    big = torch.full((M, K + (4 if view == 'off1' else 8)), SENTINEL, device='cuda')
    v = big[:, 1:K + 1] if view == 'off1' else big[:, :K]
    v.copy_(_dev(a))
    assert (v.data_ptr() % 16 != 0) == (view == 'off1')
    return v


def _chain_sample(rng, M, N, K):
    """Rows and columns on which the fma chain is restated: everything for small products, else 24 rows x 48 columns with the corners."""
    if M * N * K <= 2e7:
        return np.arange(M), np.arange(N)
    pick = lambda n, k: np.unique(np.concatenate([[0, n - 1], rng.choice(n, min(n, k), replace=False)]))
    return pick(M, 24), pick(N, 48)


def _gemm_case(M, N, K, view, route, lens=None, seed=0):
    from regtr_amd import ops
    rng = np.random.default_rng(seed)
    a, b, bias, div, res = _operands(rng, M, N, K)
    _, k_chunk, s_eff = dispatch.gemm_f32_plan(M, N, K)
    assert ('+splitk_reduce' in route) == (s_eff > 1)
    a_dev, b_dev = _a_view(a, view), _dev(b)
    kw, a_f32, a64, a_rel = {}, a, a, 0.0
    if lens is not None:                                  # the folded operand: lrelu((a - mean) rstd), statistics per cloud
        stats = np.stack([rng.standard_normal((len(lens), K)), rng.uniform(0.5, 2.0, (len(lens), K))], -1).astype(F32)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        kw = dict(a_stats=_dev(stats), a_seg_off=_dev(off, torch.int32), a_slope=SLOPE)
        a64, a_rel = FR.fold_operand(a, stats, lens, SLOPE)
        seg = np.repeat(np.arange(len(lens)), lens)
        v = (a - stats[seg, :, 0]) * stats[seg, :, 1]     # float32, operation by operation, as the kernel's load does
        a_f32 = np.where(v > 0, v, v * F32(SLOPE)).astype(F32)
    ldc, ldr = (N + 5, N + 3) if view == 'strided' else (N, N)
    res_dev = torch.full((M, ldr), SENTINEL, device='cuda')
    res_dev[:, :N] = _dev(res)
    # bare: float64 bound and the exact chain
    ref, bound, raw, raw_bound = FR.gemm_ref(a64, b, s_eff, a_rel=a_rel)
    buf = _window(M, N, ldc)
    ops.gemm(a_dev, b_dev, out=buf[:M, :N], **kw)
    got = _check_window(buf, M, N)
    r_bare = _ratio(np.abs(got.astype(np.float64) - ref), bound)
    rows, cols = _chain_sample(rng, M, N, K)
    chain = FR.chain_product(a_f32[rows], b[:, cols], k_chunk)
    sub = got[np.ix_(rows, cols)]
    mism = int((sub.view(np.uint32) != chain.view(np.uint32)).sum())
    # the full epilogue: row_div, bias, ReLU, residual
    ref2, bound2, _, _ = FR.gemm_ref(a64, b, s_eff, bias=bias, row_div=div, residual=res, relu=True, a_rel=a_rel)
    buf = _window(M, N, ldc)
    ops.gemm(a_dev, b_dev, bias=_dev(bias), row_div=_dev(div), residual=res_dev[:, :N], relu=True, out=buf[:M, :N], **kw)
    got2 = _check_window(buf, M, N)
    r_epi = _ratio(np.abs(got2.astype(np.float64) - ref2), bound2)
    print(f'gemm_f32 {route} ({M}, {N}, {K}) {view}: bare err/bound {r_bare:.3f}, epilogue err/bound {r_epi:.3f}, '
          f'chain mismatches {mism} of {sub.size}')
    assert r_bare <= 1.0 and r_epi <= 1.0, (r_bare, r_epi)
    assert mism == 0, f'{mism} of {sub.size} elements differ from the float32 fma chain in ascending k'


@pytest.mark.parametrize('M,N,K,view,route', GEMM_CASES)
def test_gemm_f32_vs_fp64_and_chain(M, N, K, view, route):
    _gemm_case(M, N, K, view, route, seed=M * 1000003 + N * 1009 + K)


@pytest.mark.parametrize('N,K,route', FOLD_CASES)
def test_gemm_f32_fold_vs_fp64_and_chain(N, K, route):
    """The InstanceNorm + LeakyReLU fold on the A load: tiles inside one cloud and tiles that straddle clouds (a one-row and an empty
    cloud among them), aligned and element-wise loads, unsplit and split-K."""
    _gemm_case(FOLD_M, N, K, 'plain', route, lens=FOLD_LENS, seed=N * 1009 + K)


def test_gemm_f32_no_rows():
    """M = 0 with live pointers (an empty tensor has none, so this goes through the C ABI): accepted, nothing launched, nothing written."""
    from regtr_amd import _lib
    L = _lib.lib()
    assert dispatch.route_gemm_f32(0, 32, 64) == 'none'
    buf = torch.full((GUARD, 32), SENTINEL, device='cuda')
    a, b = torch.ones((4, 64), device='cuda'), torch.ones((64, 32), device='cuda')
    for N in (32, 64):
        _lib.check(L.regtr_gemm_f32(_lib.ptr(a), 64, _lib.ptr(b), N, _lib.ptr(buf), N, 0, N, 64 * 32 // N, None, None, None, 0, 0, None, None,
                                    0, 0.1, None, 0, _lib.stream()), 'regtr_gemm_f32')
    torch.cuda.synchronize()
    assert torch.all(buf == SENTINEL)


# ------------------------------------------------------------------------------------------------ regtr_layernorm
LN_DS = (4, 68, 252, 256, 260, 512, 516, 1020, 1024, 1028, 2052)
LN_NS = (1, 5, 257)
LN_FLAT = 1e-5


@pytest.mark.parametrize('n', LN_NS)
@pytest.mark.parametrize('D', LN_DS)
def test_layernorm_fwd_vs_fp64(D, n):
    """Column trip counts 1 .. 9 with lanes that own nothing, row counts that end inside a workgroup of four rows; `add` and y_plain on
    and off; rows offset by 0 and by 100 (the mean's error amplified by rstd |gamma|); one constant row (rstd = 1 / sqrt(eps)).  The flat
    1e-5 of tests/test_gpu_ops.py holds at offset 0 on every row but the constant one, whose bound is the derived one alone."""
    from regtr_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(7000 * D + n)
    gamma, beta = rng.standard_normal(D).astype(F32), rng.standard_normal(D).astype(F32)
    add = rng.standard_normal((n, D)).astype(F32)
    const_row = n // 2 if n >= 5 else None
    worst = 0.0
    for offset in (0.0, 100.0):
        x = (rng.standard_normal((n, D)) * 3 + 1 + offset).astype(F32)
        if const_row is not None:
            x[const_row] = F32(0.3 + offset)
        for with_add, with_plain in itertools.product((False, True), (False, True)):
            r = CR.layernorm_fwd(x, gamma, beta, add if with_add else None)
            y, yp = _window(n, D, D), _window(n, D, D)
            xd, gd, bd, ad = _dev(x), _dev(gamma), _dev(beta), _dev(add)
            _lib.check(L.regtr_layernorm(_lib.ptr(xd), n, D, _lib.ptr(gd), _lib.ptr(bd), 1e-5, _lib.ptr(ad) if with_add else None,
                                         _lib.ptr(y), _lib.ptr(yp) if with_plain else None, _lib.stream()), 'regtr_layernorm')
            outs = [('y', _check_window(y, n, D))]
            if with_plain:
                outs.append(('plain', _check_window(yp, n, D)))
            else:
                torch.cuda.synchronize()
                assert torch.all(torch.isnan(yp[:n])) and torch.all(yp[n:] == SENTINEL)
            for name, got in outs:
                err = np.abs(got.astype(np.float64) - r[name])
                ratio = _ratio(err, r['b_' + name])
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, offset, with_add, with_plain, ratio)
                if offset == 0.0:
                    keep = np.arange(n) != (-1 if const_row is None else const_row)
                    assert err[keep].max() < LN_FLAT, (name, float(err[keep].max()))
    print(f'layernorm D={D} n={n}: worst err/bound {worst:.3f}')


# ------------------------------------------------------------------------------------------------ regtr_posemb_sine
# No document shipped with ROCm states an ulp bound for the device sinf / cosf, so the bar is twice the worst error measured on an
# MI355X against float64 sin / cos of the float32 argument, over all cases below (docs/PARITY.md): 1.515 ulp measured, 3.03 allowed.
POSEMB_ULP_MEASURED = 1.515
POSEMB_COORDS = (0.0, 1e-3, -1e-3, 8.0, -8.0, 100.0, -100.0)


def _posemb_ref(xyz, npf, d_model, scale, temperature=10000):
    """float64 sin / cos of the argument the kernel forms in float32, operation by operation: p = (x * scale32) / dim_t[f]."""
    import math
    dim_t = torch.arange(npf, dtype=torch.float32)
    dim_t = (temperature ** (2 * torch.div(dim_t, 2, rounding_mode='trunc') / npf)).numpy()
    scale32 = F32(torch.tensor(scale * 2 * math.pi, dtype=torch.float32).item())
    p = ((xyz[:, :, None] * scale32).astype(F32) / dim_t[None, None, :]).astype(F32).astype(np.float64)
    f = np.arange(npf)
    ref = np.where(f % 2 == 1, np.cos(p), np.sin(p)).reshape(len(xyz), 3 * npf)
    return np.concatenate([ref, np.zeros((len(xyz), d_model - 3 * npf))], 1), dim_t, scale32


def _ulps(got, ref):
    """|got - ref| in units of the float32 spacing at |ref| (at least the smallest normal's)."""
    spacing = np.spacing(np.maximum(np.abs(ref), 2.0 ** -126).astype(F32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref) / spacing


@pytest.mark.parametrize('n', (1, 257))
@pytest.mark.parametrize('d_model,npf', [(6, 2), (32, 10), (256, 84), (260, 86), (260, 84)])
def test_posemb_sine_vs_fp64(d_model, npf, n):
    """Widths whose zero pad is 0, 2, 4, 2 and -- through the C ABI, with fewer frequencies than the width allows -- 8 columns, which
    must be +0 exactly; coordinates 0, +-1e-3, +-8, +-100 (arguments up to 628 radians: sinf's range reduction) beside random ones in
    [-4, 4]; scale 1 (the shipped configurations' own) and 3.7."""
    from oracle import regtr_ref
    from regtr_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(d_model * 31 + n)
    xyz = ((rng.random((n, 3)) - 0.5) * 8).astype(F32)
    k = min(n, len(POSEMB_COORDS))
    xyz[:k, 0] = POSEMB_COORDS[:k]
    if n > 2 * len(POSEMB_COORDS):
        xyz[k:2 * k, 1] = POSEMB_COORDS
        xyz[2 * k:3 * k, 2] = POSEMB_COORDS[::-1]
    worst = 0.0
    for scale in (1.0, 3.7):
        ref, dim_t, scale32 = _posemb_ref(xyz, npf, d_model, scale)
        pe = _window(n, d_model, d_model)
        xd, td = _dev(xyz), _dev(dim_t)
        _lib.check(L.regtr_posemb_sine(_lib.ptr(xd), n, npf, d_model, float(scale32), _lib.ptr(td), _lib.ptr(pe), _lib.stream()),
                   'regtr_posemb_sine')
        got = _check_window(pe, n, d_model)
        pad = got[:, 3 * npf:]
        assert pad.shape[1] == d_model - 3 * npf and np.all(pad.view(np.uint32) == 0), 'the pad columns must be +0'
        ulps = _ulps(got, ref)
        worst = max(worst, float(ulps.max()))
        zero = xyz == 0.0                                                     # sin(0) = 0 and cos(0) = 1 exactly
        if zero.any():
            i, a = np.nonzero(zero)
            blk = got[i[0], a[0] * npf:(a[0] + 1) * npf]
            assert np.all(blk[0::2] == 0.0) and np.all(blk[1::2] == 1.0)
        if scale == 1.0 and npf == d_model // 3 // 2 * 2:                     # the bar of tests/test_gpu_ops.py, at |xyz| <= 4
            small = np.abs(xyz).max(1) <= 4
            want = regtr_ref.pos_embed_sine(torch.from_numpy(xyz[small]), d_model, 1.0).numpy()
            assert np.abs(got[small] - want).max() < 2e-5
    print(f'posemb d_model={d_model} npf={npf} n={n}: worst error {worst:.3f} ulp')
    assert worst <= 2 * POSEMB_ULP_MEASURED, worst


# ------------------------------------------------------------------------------------------------ regtr_add_f32
@pytest.mark.parametrize('n', (0, 1, 3, 4, 5, 1023, 1024, 1027))
def test_add_f32_bit_equal(n):
    """The float4 body, the scalar tail of the last thread and the block edge at 1024 elements: bit-equal to float32 addition."""
    from regtr_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    out = torch.full((n + 8,), SENTINEL, device='cuda')
    out[:n] = float('nan')
    ad, bd = (_dev(np.concatenate([v, np.zeros(4, F32)])) for v in (a, b))     # (never an empty allocation)
    _lib.check(L.regtr_add_f32(_lib.ptr(ad), _lib.ptr(bd), n, _lib.ptr(out), _lib.stream()), 'regtr_add_f32')
    torch.cuda.synchronize()
    assert np.array_equal(out[:n].cpu().numpy().view(np.uint32), (a + b).view(np.uint32))
    assert torch.all(out[n:] == SENTINEL)


# ------------------------------------------------------------------------------------------------ regtr_overlap_avgpool
@pytest.mark.parametrize('nq', (1, 255, 257))
def test_overlap_avgpool_bit_equal(nq):
    """Restated in float32 in the kernel's order (entries left to right, one division, clamp): bit-equal.  H < ld (the columns past H
    hold indices that must not be read as entries); rows of shadows only give NaN; values outside [0, 1] come back clamped; a negative
    entry counts as padding."""
    from regtr_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(nq)
    ns, H, ld = 97, 7, 11
    ov = rng.uniform(-0.5, 1.7, ns).astype(F32)
    nbr = rng.integers(0, ns + 1, (nq, ld)).astype(np.int32)                 # ns itself: the shadow
    nbr[:, H:] = rng.integers(0, ns, (nq, ld - H))                            # valid-looking entries past H
    nbr[rng.random((nq, ld)) < 0.1] = -1
    nbr[0, :H] = ns
    if nq > 4:
        nbr[1, :H] = int(np.argmin(ov))                                       # a mean below 0 and one above 1: clamped
        nbr[2, :H] = int(np.argmax(ov))
        nbr[nq // 2, :H] = [ns, -1, ns, -1, ns, ns, -1]
        nbr[nq - 1, :H] = [0, 1, 2, 3, 4, 5, 6]
    want = np.empty(nq, F32)
    for q in range(nq):
        s, c = F32(0), F32(0)
        for h in range(H):
            i = nbr[q, h]
            if 0 <= i < ns:
                s, c = F32(s + ov[i]), F32(c + F32(1))
        with np.errstate(invalid='ignore'):
            v = F32(s) / F32(c)
        want[q] = v if np.isnan(v) else min(max(v, F32(0)), F32(1))
    assert np.isnan(want[0]) and ov.min() < 0 and ov.max() > 1
    if nq > 4:
        assert want[1] == 0 and want[2] == 1 and np.isnan(want[nq // 2])
    out = torch.full((nq + 8,), SENTINEL, device='cuda')
    od, nd = _dev(ov), _dev(nbr, torch.int32)
    _lib.check(L.regtr_overlap_avgpool(_lib.ptr(od), ns, _lib.iptr(nd), ld, nq, H, _lib.ptr(out), _lib.stream()), 'regtr_overlap_avgpool')
    torch.cuda.synchronize()
    got = out[:nq].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
    assert np.all((got[ok] >= 0) & (got[ok] <= 1)) and torch.all(out[nq:] == SENTINEL)


# ------------------------------------------------------------------------------------------------ regtr_nearest_in_radius
def _nearest_ref(q, q_lens, s, s_lens, radius):
    """Brute force in float64 over the float32 coordinates: the nearest support of the query's cloud with d2 < radius^2 (the caller's
    double), the lower index on a tie, -1 without one; d2 = (dx^2 + dy^2) + dz^2 as the kernel adds it."""
    q64, s64 = q.astype(np.float64), s.astype(np.float64)
    qo, so = np.concatenate([[0], np.cumsum(q_lens)]), np.concatenate([[0], np.cumsum(s_lens)])
    out = np.full(len(q), -1, np.int64)
    r2 = float(radius) * float(radius)
    for c in range(len(q_lens)):
        for i in range(qo[c], qo[c + 1]):
            if so[c + 1] == so[c]:
                continue
            d = q64[i] - s64[so[c]:so[c + 1]]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            j = int(np.argmin(d2))                                            # the first minimum: the lower index
            if d2[j] < r2:
                out[i] = so[c] + j
    return out


def _nearest(q, q_lens, s, s_lens, radius):
    from regtr_amd import overlap
    off = lambda lens: _dev(np.concatenate([[0], np.cumsum(lens)]), torch.int32)
    got = overlap.nearest_in_radius(_dev(q), off(q_lens), _dev(s), off(s_lens), radius)
    torch.cuda.synchronize()
    return got.cpu().numpy().astype(np.int64)


def test_nearest_in_radius_vs_brute_force():
    """Three clouds, the middle one without supports (its queries answer -1); duplicate supports (the lower index wins); supports of
    another cloud nearer than any of the query's own; a radius float32 cannot hold -- 0.7 rounds DOWN to float32, the cell grid is built
    at that float32, the ball test uses the caller's double: a support at distance float32(0.7) is inside."""
    rng = np.random.default_rng(11)
    r = 0.7
    assert float(F32(r)) < r
    s_lens, q_lens = [60, 0, 45], [50, 6, 40]
    s = (rng.random((sum(s_lens), 3)) * 4).astype(F32)
    q = (rng.random((sum(q_lens), 3)) * 4).astype(F32)
    s[7] = s[3]; s[20] = s[3]; s[70] = s[65]                                  # duplicates
    q[0] = s[3]; q[60] = s[65]                                                # queries on a duplicated support: distance 0 twice
    q[1] = [0, -8, -8]; s[0] = [F32(r), -8, -8]                              # at distance float32(r) < r exactly: inside
    q[2] = [20, 20, 20]                                                       # nothing in range
    s[61] = q[3]                                                              # cloud 2's support on a query of cloud 0: not a candidate
    want = _nearest_ref(q, q_lens, s, s_lens, r)
    got = _nearest(q, q_lens, s, s_lens, r)
    assert np.array_equal(got, want), np.nonzero(got != want)
    assert want[0] == 3 and want[60] == 65 and want[1] == 0 and want[2] == -1 and want[3] != 61
    assert np.all(want[50:56] == -1) and (want >= 0).sum() > 20 and (want == -1).sum() > 8


def test_nearest_in_radius_boundary_and_ties():
    """A representable radius, 5 / 8, with supports at exactly d2 = r2 on a 3-4-5 triangle in eighths (excluded: the test is d2 < r2);
    two supports at the same distance on either side (the lower index wins); a support one float32 step inside the sphere (included)."""
    r = 0.625
    q = np.array([[0, 0, 0], [8, 8, 8], [16, 16, 16], [0, 24, 24]], F32)
    inside = np.nextafter(F32(0.625), F32(0))
    s = np.array([[0.375, 0.5, 0],                      # q0: exactly on the sphere -- excluded
                  [8.25, 8, 8], [7.75, 8, 8],           # q1: two at distance 1/4 -- index 1
                  [16, 16, 16 + 0.625],                 # q2: on the sphere along one axis -- excluded
                  [inside, 24, 24], [0, 24.625, 24]], F32)                    # q3: one step inside wins over one on the sphere
    want = _nearest_ref(q, [4], s, [6], r)
    assert list(want) == [-1, 1, -1, 4]
    assert np.array_equal(_nearest(q, [4], s, [6], r), want)
