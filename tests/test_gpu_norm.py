"""GPU (-m gpu): the InstanceNorm kernels (csrc/norm.hip), the strip GEMM (csrc/gemm_stream.hip) and the block tail (csrc/block_tail.hip)
against float64, under bounds taken from each kernel's arithmetic.

Outputs are views inside larger buffers (NaN inside, finite sentinels around): every element of the view must be written and nothing
outside it.  The C ABI is called directly wherever the `ops` wrappers would hide a layout (strided outputs, ldc / ldy > N).  The float64
references run on the device.  tests/dispatch.py names the launch regime of every case, tests/test_dispatch_routes.py (CPU) asserts that
the cases reach every one of them, and tests/test_norm_bounds_host.py (CPU) shows that the checkers below reject a kernel that drops a
chunk of rows."""
import math

import numpy as np
import pytest
import torch

from tests import dispatch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24           # float32 unit roundoff
U64 = 2.0 ** -53
EPS = float(np.float32(1e-5))   # the eps the kernels add in float64: the float parameter's value, not 1e-5 (2.5e-8 of it apart, a fifth of
SLOPE = 0.1                     # the rounding bound of a constant channel's rstd)
SENTINEL = 1234.5
PAD = 8                  # sentinel rows / elements around a view


def _lib():
    from regtr_amd import _lib
    return _lib


def _seg(lens, device='cuda'):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device=device)


def _rows_cloud(lens, device):
    return torch.repeat_interleave(torch.arange(len(lens), device=device), torch.tensor(lens, device=device))


def _boxed(rows, cols, ld=None, dtype=torch.float32):
    """(buffer, view): a rows x cols NaN view with leading dimension ld inside PAD sentinel rows each side (and ld - cols sentinel columns)."""
    ld = cols if ld is None else ld
    buf = torch.full((rows + 2 * PAD, ld), SENTINEL, dtype=dtype, device='cuda')
    view = buf[PAD:PAD + rows, :cols]
    view.fill_(float('nan'))
    return buf, view


def _check_boxed(buf, view, what):
    outside = buf.clone()
    rows, cols = view.shape
    outside[PAD:PAD + rows, :cols] = SENTINEL
    assert (outside == SENTINEL).all(), f'{what}: written outside its view'
    nan = int(torch.isnan(view).sum())
    assert nan == 0, f'{what}: {nan} elements of the view left unwritten'


# ------------------------------------------------------------------------------------------------ float64 statistics and their bound
def moments64(x, lens):
    """Per cloud: n, mean, biased variance, E|x| and E x^2 of x's rows in float64 (two passes), shapes (n_clouds, C)."""
    dev = x.device
    n = torch.tensor(lens, dtype=torch.float64, device=dev)[:, None]
    rows = _rows_cloud(lens, dev)
    x64 = x.double()
    C = x.shape[1]
    z = torch.zeros((len(lens), C), dtype=torch.float64, device=dev)
    nn_ = n.clamp_min(1.0)
    mean = z.clone().index_add_(0, rows, x64) / nn_
    d = x64 - mean[rows]
    var = z.clone().index_add_(0, rows, d * d) / nn_
    eabs = z.clone().index_add_(0, rows, x64.abs()) / nn_
    return n, mean, var, eabs, var + mean * mean


def stats_ratio(got, n, mean, var, eabs, esq):
    """err / bound of float32 (mean, rstd) against the float64 statistics, worst over all entries (empty clouds must be exactly (0, 0)).

    The kernels sum x and x^2 in float64, take var = sum x^2 / n - mean^2 and round mean and 1 / sqrt(var + eps) to float32 once:
      mean:  u |mean| (the rounding) + 2 n 2^-53 E|x|  (n - 1 float64 additions of terms up to |x|, in the kernel and in the reference);
      rstd:  u rstd + 2 n 2^-53 (mean^2 + var) / (var + eps) rstd -- the float64 cancellation: sum x^2 / n carries n 2^-53 E x^2,
             mean^2 another 2 n 2^-53 |mean| E|x| <= 2 n 2^-53 E x^2, and the square root halves the relative error of var + eps."""
    mask = n[:, 0] > 0
    g = got.double()
    assert (g[~mask] == 0).all(), 'an empty cloud must give (0, 0)'
    r64 = 1.0 / torch.sqrt(var + EPS)
    bm = U * mean.abs() * (1 + 1e-6) + 2 * n * U64 * eabs + 1e-300
    br = (U * (1 + 1e-6) + 2 * n * U64 * esq / (var + EPS)) * r64
    rm = ((g[..., 0] - mean).abs() / bm)[mask]
    rr = ((g[..., 1] - r64).abs() / br)[mask]
    if rm.numel() == 0:
        return 0.0
    return max(rm.max().item(), rr.max().item())


# ------------------------------------------------------------------------------------------------ a. InstanceNorm statistics
def norm_lens(C, rows):
    """Eight clouds whose longest (128 rows) makes in_rows settle at `rows` (cdiv(128 rows, rows) x 8 = 1024 workgroups), next to an empty
    and a one-row cloud and lengths one short / one past the unrolled 4 TR-row step and a whole chunk."""
    TR = 1024 // C
    L = 128 * rows
    return [L, 0, 1, 4 * TR - 1, 4 * TR + 1, min(L, rows + 4 * TR + 1), 2 * rows - 1, 3]


def many_lens(C, seed=0):
    rng = np.random.default_rng(seed + C)
    lens = rng.integers(0, 200, 1200).tolist()
    lens[3], lens[7] = 0, 1
    return lens


def _norm_input(lens, C, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    M = sum(lens)
    scale = torch.rand(C, device='cuda', generator=g) * 4.9 + 0.1
    shift = (torch.rand(C, device='cuda', generator=g) - 0.5) * 6
    x = torch.randn((M + 5, C), device='cuda', generator=g) * scale + shift         # 5 rows past seg_off[n]
    x[:, 0] = 2.5                                                                      # a constant channel
    x[:, 1] = 1e3 + 1e-3 * torch.randn(M + 5, device='cuda', generator=g)              # an offset one: mean 1e3, sigma 1e-3
    return x


def _norm_cases():
    out = [(C, 'rows', r) for C, r in sorted(dispatch.NORM_KERNELS)]
    return out + [(C, 'many', 128) for C in dispatch.NORM_WIDTHS]


def case_lens(C, kind, rows):
    return norm_lens(C, rows) if kind == 'rows' else many_lens(C)


@pytest.mark.parametrize('C,kind,rows', _norm_cases())
def test_instnorm_stats_vs_fp64(C, kind, rows):
    lib = _lib()
    L = lib.lib()
    lens = case_lens(C, kind, rows)
    n_clouds, max_len = len(lens), max(lens)
    assert dispatch.in_rows(n_clouds, max_len, C) == rows
    x = _norm_input(lens, C, seed=C + rows)
    seg = _seg(lens)
    nb = L.regtr_instnorm_ws_bytes(n_clouds, max_len, C)
    assert nb == dispatch.instnorm_ws_bytes(n_clouds, max_len, C)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    buf, st = _boxed(n_clouds, 2 * C)
    lib.check(L.regtr_instnorm_stats(lib.ptr(x), lib.iptr(seg), n_clouds, max_len, C, EPS, st.data_ptr(), lib.bptr(ws), nb, lib.stream()),
              'regtr_instnorm_stats')
    torch.cuda.synchronize()
    _check_boxed(buf, st, 'stats')
    r = stats_ratio(st.view(n_clouds, C, 2), *moments64(x[:sum(lens)], lens))
    print(f'instnorm stats C {C} rows {rows} ({kind}): err/bound {r:.3f}')
    assert r <= 1


# ------------------------------------------------------------------------------------------------ b. finalize from tile partials
def tile_partials(x, lens, tile_rows):
    """The slot table regtr_instnorm_finalize_tiles reads, built here in float64: slot (tile + cloud) C + c = (sum, sum of squares) of the
    cloud's rows in that tile.  Slots no cloud owns are NaN, so a kernel that reads one fails."""
    M, C = x.shape
    rows = _rows_cloud(lens, x.device)
    slot = torch.arange(M, device=x.device) // tile_rows + rows
    n_slots = -(-max(M, 1) // tile_rows) + len(lens)
    p = torch.zeros((n_slots, C, 2), dtype=torch.float64, device=x.device)
    p[..., 0].index_add_(0, slot, x.double())
    p[..., 1].index_add_(0, slot, x.double() ** 2)
    used = torch.zeros(n_slots, dtype=torch.bool, device=x.device)
    used[slot] = True
    p[~used] = float('nan')
    return p, used


def finalize64(p, used, lens, tile_rows):
    """float64 (n, mean, var) of each cloud from the same partials, summed in slot order with the kernels' formula."""
    off = np.concatenate([[0], np.cumsum(lens)])
    C = p.shape[1]
    s = torch.zeros((len(lens), C, 2), dtype=torch.float64, device=p.device)
    for b, n in enumerate(lens):
        if n:
            t0, t1 = off[b] // tile_rows, (off[b + 1] - 1) // tile_rows
            s[b] = p[t0 + b:t1 + b + 1].sum(0)
    n = torch.tensor(lens, dtype=torch.float64, device=p.device)[:, None]
    mean = s[..., 0] / n.clamp_min(1)
    var = (s[..., 1] / n.clamp_min(1) - mean * mean).clamp_min(0)
    return n, mean, var


FINALIZE_CASES = [       # (C, tile_rows, lens)
    (64, 256, [300 * 256 - 100, 700]),                       # wave: 300 tiles, a cloud starting mid-tile
    (2048, 128, [1000, 0]),                                  # wave at n_clouds C = 4096, an empty cloud
    (241, 64, [0, 1, 130, 64, 5, 0, 64, 63, 1, 2, 700, 3, 0, 9, 128, 10]),   # wave at 3856, C not a multiple of 4
    (64, 64, [3] * 30 + [0, 1, 200, 0] + [65] * 31),         # thread<64> at 4160
    (160, 1, [0, 1, 300] + [7] * 23),                        # thread<128>, one-row tiles: a cloud over 300 tiles
    (257, 128, [129, 0, 1, 127, 256, 255, 3, 0, 500, 1, 2, 128, 64, 64, 700, 11]),   # thread<256> at 4112
    (4097, 256, [600]),                                      # thread<256>, one cloud wider than a workgroup's columns
    (64, 128, [3] * 70),                                     # thread<64>: 42 clouds in one 128-row tile
    (32, 256, [2, 256 * 3 + 7, 0, 1, 256 * 299]),            # wave: one cloud over 300 tiles
]


@pytest.mark.parametrize('C,tile_rows,lens', FINALIZE_CASES)
def test_instnorm_finalize_tiles_vs_fp64(C, tile_rows, lens):
    lib = _lib()
    g = torch.Generator(device='cuda').manual_seed(C + tile_rows + len(lens))
    M = sum(lens)
    x = torch.randn((M, C), device='cuda', generator=g) * (torch.rand(C, device='cuda', generator=g) * 3 + 0.1) + 0.7
    x[:, 0] = -4.0
    x[:, 1] = 1e3 + 1e-3 * torch.randn(M, device='cuda', generator=g)
    p, used = tile_partials(x, lens, tile_rows)
    seg = _seg(lens)
    n_clouds = len(lens)
    buf, st = _boxed(n_clouds, 2 * C)
    lib.check(lib.lib().regtr_instnorm_finalize_tiles(lib.dptr(p.contiguous()), lib.iptr(seg), n_clouds, C, tile_rows, EPS, st.data_ptr(),
                                                     lib.stream()), 'regtr_instnorm_finalize_tiles')
    torch.cuda.synchronize()
    _check_boxed(buf, st, 'stats')
    n, mean, var = finalize64(p, used, lens, tile_rows)
    _, _, _, eabs, esq = moments64(x, lens)
    r = stats_ratio(st.view(n_clouds, C, 2), n, mean, var, eabs, esq)
    print(f'finalize_tiles C {C} tile_rows {tile_rows} {dispatch.route_finalize_tiles(n_clouds, C)}: err/bound {r:.3f}')
    assert r <= 1


# ------------------------------------------------------------------------------------------------ c. apply
APPLY_CASES = [(4, [0, 1, 1025, 3]), (64, [700, 0, 1300]), (256, [1, 2, 5000]), (128, [3] * 70), (512, [301, 0, 450]), (1024, [301, 450, 0])]


def apply_combos(C):
    out = []
    for has_st in (True, False):
        for res in ('none', 'raw', 'norm'):
            for act in (0, 1):
                for alias in (False, True):
                    for rp in ('none', 'flag', 'xyz'):
                        if rp != 'none' and C > 256:
                            continue
                        out.append((has_st, res, act, alias, rp))
    return out


def _rand_stats(n_clouds, C, g):
    mu = torch.randn((n_clouds, C), device='cuda', generator=g) * 2
    rs = torch.rand((n_clouds, C), device='cuda', generator=g) * 3 + 0.05
    return torch.stack((mu, rs), -1).contiguous()


@pytest.mark.parametrize('C,lens', APPLY_CASES)
def test_instnorm_apply_vs_fp64(C, lens):
    """Every flag combination of regtr_instnorm_apply.  Reference: float64 from the same float32 statistics; bound per element
    4 u (|x - mu| r + |q - mu_r| r_r) (|x| for no statistics, |q| for a raw residual): the rounded difference, product, sum and LeakyReLU
    product.  The row flag is a float32 sum of the C results: it must be exact wherever |float64 row sum| exceeds the elements' bounds
    summed plus C u sum |y| (the sum's own rounding)."""
    lib = _lib()
    L = lib.lib()
    g = torch.Generator(device='cuda').manual_seed(C + len(lens))
    M, n_clouds, max_len = sum(lens), len(lens), max(lens)
    EXTRA = 5                                                        # rows past seg_off[n]: never touched
    seg = _seg(lens)
    rows = _rows_cloud(lens, 'cuda')
    x0 = torch.randn((M + EXTRA, C), device='cuda', generator=g) * 3 + 0.2
    q0 = torch.randn((M + EXTRA, C), device='cuda', generator=g) * 2 - 0.3
    st, rst = _rand_stats(n_clouds, C, g), _rand_stats(n_clouds, C, g)
    xyz = torch.randn((M + EXTRA, 3), device='cuda', generator=g)
    worst, n_flag = 0.0, 0
    for has_st, res, act, alias, rp in apply_combos(C):
        x = x0.clone()
        if alias:
            buf, y = None, x
        else:
            buf, y = _boxed(M + EXTRA, C)
            y[M:] = SENTINEL
        flag_buf = None
        if rp == 'flag':
            flag_buf = torch.full((M + EXTRA + 2 * PAD,), SENTINEL, device='cuda')
            flag_buf[PAD:PAD + M] = float('nan')
            fp = flag_buf[PAD:].data_ptr()
        elif rp == 'xyz':
            flag_buf = torch.full((M + EXTRA + 2 * PAD, 4), SENTINEL, device='cuda')
            flag_buf[PAD:PAD + M] = float('nan')
            fp = flag_buf[PAD:].data_ptr()
        lib.check(L.regtr_instnorm_apply(x.data_ptr(), lib.iptr(seg), n_clouds, max_len, C, st.data_ptr() if has_st else None,
                                         q0.data_ptr() if res != 'none' else None, rst.data_ptr() if res == 'norm' else None, act, SLOPE,
                                         y.data_ptr(), xyz.data_ptr() if rp == 'xyz' else None, fp if rp != 'none' else None,
                                         lib.stream()), 'regtr_instnorm_apply')
        torch.cuda.synchronize()
        what = f'C {C} stats {has_st} res {res} act {act} alias {alias} row_positive {rp}'
        if alias:
            assert torch.equal(y[M:], x0[M:]), f'{what}: rows past seg_off[n] written'
        else:
            assert (y[M:] == SENTINEL).all(), f'{what}: rows past seg_off[n] written'
            out = buf.clone()
            out[PAD:PAD + M + EXTRA] = SENTINEL
            assert (out == SENTINEL).all(), f'{what}: written outside the view'
        yv = y[:M].double()
        assert not torch.isnan(yv).any(), f'{what}: rows left unwritten'
        xd = x0[:M].double()
        if has_st:
            s = st.double()[rows]
            t = (xd - s[..., 0]) * s[..., 1]
            b = (xd - s[..., 0]).abs() * s[..., 1]
        else:
            t, b = xd, xd.abs()
        if res == 'raw':
            t, b = t + q0[:M].double(), b + q0[:M].double().abs()
        elif res == 'norm':
            s = rst.double()[rows]
            t = t + (q0[:M].double() - s[..., 0]) * s[..., 1]
            b = b + (q0[:M].double() - s[..., 0]).abs() * s[..., 1]
        if act:
            t = torch.where(t > 0, t, t * float(np.float32(SLOPE)))
        bound = 4 * U * b + 1e-30
        r = ((yv - t).abs() / bound).max().item() if M else 0.0
        assert r <= 1, f'{what}: err/bound {r:.3g}'
        worst = max(worst, r)
        if rp != 'none':
            fl = flag_buf[PAD:PAD + M + EXTRA]
            assert (fl[M:] == SENTINEL).all(), f'{what}: flags past seg_off[n] written'
            assert (flag_buf[:PAD] == SENTINEL).all(), f'{what}: flags before the rows written'
            f = fl[:M, 3] if rp == 'xyz' else fl[:M]
            if rp == 'xyz':
                assert torch.equal(fl[:M, :3], xyz[:M]), f'{what}: xyz not copied bit for bit'
            assert ((f == 0) | (f == 1)).all(), f'{what}: flags not 0 / 1'
            rs = t.sum(1)
            thr = bound.sum(1) + C * U * t.abs().sum(1)
            sure = rs.abs() > thr
            bad = (f.double() != (rs > 0).double()) & sure
            assert not bad.any(), f'{what}: flag of row {int(bad.nonzero()[0])} wrong'
            n_flag += int(sure.sum())
    print(f'instnorm apply C {C} lens {lens[:4]}: worst err/bound {worst:.3f}, {n_flag} flags checked')
    if C <= 256 and M:
        assert n_flag > 0


def test_instnorm_apply_and_stats_refusals():
    """Arguments the launchers refuse with RG_ERR_ARG before anything is written."""
    lib = _lib()
    L = lib.lib()
    lens = [40, 0, 9]
    seg = _seg(lens)
    M = sum(lens)
    for C, rp, xyz, mis in ((12, False, False, 0), (2048, False, False, 0), (512, True, False, 0), (64, False, True, 0), (64, True, True, 1)):
        x = torch.randn((M, C), device='cuda')
        y = torch.full((M, C), SENTINEL, device='cuda')
        flags = torch.full((M * 4 + 4,), SENTINEL, device='cuda')
        xyzt = torch.randn((M, 3), device='cuda')
        with pytest.raises(RuntimeError):
            lib.check(L.regtr_instnorm_apply(x.data_ptr(), lib.iptr(seg), len(lens), max(lens), C, None, None, None, 1, SLOPE, y.data_ptr(),
                                             xyzt.data_ptr() if xyz else None, flags[mis:].data_ptr() if rp else None, lib.stream()),
                      'regtr_instnorm_apply')
        torch.cuda.synchronize()
        assert (y == SENTINEL).all() and (flags == SENTINEL).all(), (C, rp, xyz, mis)
        if C in (12, 2048):
            st = torch.full((len(lens), C, 2), SENTINEL, device='cuda')
            ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
            assert L.regtr_instnorm_ws_bytes(len(lens), max(lens), C) == 256
            with pytest.raises(RuntimeError):
                lib.check(L.regtr_instnorm_stats(x.data_ptr(), lib.iptr(seg), len(lens), max(lens), C, EPS, st.data_ptr(), lib.bptr(ws),
                                                 1 << 20, lib.stream()), 'regtr_instnorm_stats')
            torch.cuda.synchronize()
            assert (st == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ d. strip GEMM
STREAM_CASES = [(32, 32), (32, 192), (32, 128), (64, 32), (64, 192), (64, 256), (128, 96), (128, 512), (128, 32)]


def f32_grade_ratio(err, err32, K, scale):
    """check_gemm's float32-grade rule (tests/dispatch_worker.py) as err / allowed: the exact-f32 kernel's bound, and at most twice that
    kernel's float64 error on the same operands (errors relative to max |ref|)."""
    tol = (2e-6 * K ** 0.5 * 4 + 1e-6) * max(1.0, scale / 10) / scale
    lim = min(tol, 2 * err32 + 1e-7 * max(1.0, scale / 10) / scale)
    return err / lim


def _stream_launch(a, planes, lens, seg, N, K, a_st, with_stats=True, ldc_pad=4):
    lib = _lib()
    L = lib.lib()
    from regtr_amd import ops
    M = a.shape[0]
    R = L.regtr_gemm_stream_tile_rows()
    assert R == 256
    ti = ops.tile_segments(seg, M, R)
    buf, out = _boxed(M, N, N + ldc_pad)
    partial = torch.full((((M + R - 1) // R + len(lens)) * N, 2), float('nan'), dtype=torch.float64, device='cuda') if with_stats else None
    lib.check(L.regtr_gemm_stream(a.data_ptr(), K, planes.data_ptr(), out.data_ptr(), N + ldc_pad, M, N, K, lib.ptr(a_st), SLOPE,
                                  lib.iptr(seg), len(lens), lib.iptr(ti), lib.dptr(partial), lib.stream()), 'regtr_gemm_stream')
    st = None
    if with_stats:
        sbuf, st = _boxed(len(lens), 2 * N)
        lib.check(L.regtr_instnorm_finalize_tiles(lib.dptr(partial), lib.iptr(seg), len(lens), N, R, EPS, st.data_ptr(), lib.stream()),
                  'regtr_instnorm_finalize_tiles')
        torch.cuda.synchronize()
        _check_boxed(sbuf, st, 'strip stats')
        st = st.view(len(lens), N, 2)
    torch.cuda.synchronize()
    return buf, out, st


@pytest.mark.parametrize('K,N', STREAM_CASES)
@pytest.mark.parametrize('li', range(5))
def test_gemm_stream_vs_fp64(li, K, N):
    """regtr_gemm_stream into C at ldc = N + 4, with and without the folded InstanceNorm + LeakyReLU operand, against float64 under
    check_gemm's float32-grade rule; the statistics (finalize_tiles, tile_rows 256) under the InstanceNorm bound against float64 of the C that
    was written.  The same launch with the third weight plane zeroed (a kernel that dropped its smallest terms) must fail the rule."""
    from regtr_amd import ops
    from tests.test_gpu_ops import STREAM_LENS
    lens = STREAM_LENS[li]
    g = torch.Generator(device='cuda').manual_seed(sum(lens) + N + K)
    M = sum(lens)
    seg = _seg(lens)
    rows = _rows_cloud(lens, 'cuda')
    a = torch.randn((M, K), device='cuda', generator=g) * torch.exp(torch.randn((M, 1), device='cuda', generator=g)) + 0.3
    w = torch.randn((N, K), device='cuda', generator=g) / K ** 0.5
    sw = ops.SplitWeight(w, 'nk')
    assert sw.planes is not None
    Npad, Kp = -(-N // 128) * 128, -(-K // 32) * 32
    zeroed = sw.planes.clone()
    zeroed[2 * Npad * Kp * 2:] = 0                                    # plane 2: the smallest terms of the split
    for fold in ((False, True) if K <= 64 else (False,)):
        a_st = ops.instnorm_stats(a, seg, max(lens)) if fold else None
        a64 = a.double()
        if fold:
            s = a_st.double()[rows]
            a64 = torch.nn.functional.leaky_relu((a64 - s[..., 0]) * s[..., 1], float(np.float32(SLOPE)))
        ref = a64 @ w.double().t()
        scale = max(ref.abs().max().item(), 1e-30)
        buf, out, st = _stream_launch(a, sw.planes, lens, seg, N, K, a_st)
        _check_boxed(buf, out, f'C K {K} N {N} fold {fold}')
        err = ((out.double() - ref).abs().max() / scale).item()
        out32 = ops.gemm(a, w.t().contiguous(), a_stats=a_st, a_seg_off=seg if fold else None)        # the exact-f32 kernel
        err32 = ((out32.double() - ref).abs().max() / scale).item()
        ratio = f32_grade_ratio(err, err32, K, scale)
        rs = stats_ratio(st, *moments64(out, lens))
        _, outz, _ = _stream_launch(a, zeroed, lens, seg, N, K, a_st, with_stats=False)
        zr = f32_grade_ratio(((outz.double() - ref).abs().max() / scale).item(), err32, K, scale)
        print(f'{dispatch.route_stream(M, N, K, fold)} lens {li}: err/allowed {ratio:.3f} (err {err:.2e}, exact-f32 {err32:.2e}), '
              f'stats err/bound {rs:.3f}, zeroed third plane err/allowed {zr:.2f}')
        assert ratio <= 1, (K, N, fold)
        assert rs <= 1, (K, N, fold)
        assert zr > 1, f'a strip kernel without its third weight plane passes the float32-grade rule ({zr:.2f})'


# ------------------------------------------------------------------------------------------------ e. block tail
def two_planes(w):
    """w rounded to its two leading bf16 planes (w0 + w1): a kernel that lost the third plane of the split."""
    w0 = w.to(torch.bfloat16).float()
    return w0 + (w - w0).to(torch.bfloat16).float()


def prod_stats64(x, lens, W):
    """float64 (mean, var) of the product x W per cloud from the input's float64 mean and covariance (two passes), and the input means."""
    dev = x.device
    K = x.shape[1]
    mean = torch.zeros((len(lens), K), dtype=torch.float64, device=dev)
    var = torch.zeros((len(lens), W.shape[1]), dtype=torch.float64, device=dev)
    o = 0
    W = W.double()
    for c, n in enumerate(lens):
        if n:
            blk = x[o:o + n].double()
            m = blk.mean(0)
            d = blk - m
            cov = d.t() @ d / n
            mean[c] = m
            var[c] = ((cov @ W) * W).sum(0).clamp_min(0)
        o += n
    return mean, mean @ W, var


def pivot_of(x, lens):
    """k_moments' pivot per cloud and channel: the trimmed mean (largest and smallest dropped) of the rows r0 + ((2 i + 1) n >> 5), i < 16."""
    out = torch.zeros((len(lens), x.shape[1]), dtype=torch.float64, device=x.device)
    o = 0
    for c, n in enumerate(lens):
        if n:
            idx = torch.tensor([o + (((2 * i + 1) * n) >> 5) for i in range(16)], device=x.device)
            v = x[idx].double()
            out[c] = (v.sum(0) - v.max(0).values - v.min(0).values) / 14
        o += n
    return out


def moment_stats_bound(x, lens, W, pivot, mean_in, mu, var, in_round):
    """Bound on |mean_k - mean| and |rstd_k - rstd| of the product statistics k_moments + k_tail_prepare report (shapes (n_clouds, N)).

    k_moments sums d = x - pivot per channel (s1, one float32 accumulator per lane over at most 256 rows: 256 u sum |d_a|) and d_a d_b
    (v_mfma_f32_32x32x2_f32: 256 steps of two products per accumulator, each step rounded: 512 u sum |d_a d_b|), float64 from there on.
    Propagated through mean_j = sum_a m_a W_aj, var_j = W^T Cov W:
      dmean_j <= 256 u sum_a |W_aj| E|d_a| + u |mean_j| (the rounding)                    + the input term
      dvar_j  <= 512 u E[(sum_a |W_aj| |d_a|)^2] + 2 (256 u sum_a |W_aj| E|d_a|) (sum_a |W_aj| |E d_a|)  + the input term
    and drstd <= (dvar / 2 / (var + eps) + u) rstd.  in_round: the relative error of the float32 operand itself next to the float64 one
    (2 u for the folded LeakyReLU(InstanceNorm(x)), u for x / num): e = in_round sum_a |W_aj| |x_a| moves the mean by E e and the
    variance by 2 E[|u_j - mean_j| e] + E e^2."""
    W = W.double()
    Wa = W.abs()
    N = W.shape[1]
    dm = torch.zeros((len(lens), N), dtype=torch.float64, device=x.device)
    dv = torch.zeros_like(dm)
    o = 0
    for c, n in enumerate(lens):
        if n:
            blk = x[o:o + n].double()
            d = blk - pivot[c]
            ed = d.abs().mean(0) @ Wa
            dm[c] = 256 * U * ed
            P = d.abs() @ Wa
            dv[c] = 512 * U * (P * P).mean(0) + 2 * (256 * U * ed) * ((d.mean(0)).abs() @ Wa)
            e = in_round * (blk.abs() @ Wa)
            uc = (blk - mean_in[c]) @ W
            dm[c] += e.mean(0)
            dv[c] += 2 * (uc.abs() * e).mean(0) + (e * e).mean(0)
        o += n
    r = 1.0 / torch.sqrt(var + EPS)
    bm = dm + U * mu.abs() + 1e-300
    br = (dv / 2 / (var + EPS) + U) * r * (1 + 1e-6)
    return bm, br


def out_stats_ratio(got, lens, mu, var, bm, br):
    mask = torch.tensor(lens, device=got.device) > 0
    g = got.double()
    assert (g[~mask] == 0).all(), 'an empty cloud must report (0, 0)'
    if not mask.any():
        return 0.0
    r = 1.0 / torch.sqrt(var + EPS)
    return max(((g[..., 0] - mu).abs() / bm)[mask].max().item(), ((g[..., 1] - r).abs() / br)[mask].max().item())


def tail_output_ratio(y, ref, y_path, stat_term, rows, n_clouds):
    """Output check of the block tail, cloud by cloud: max(|y - ref64| - stat_term) <= 2 max|y_path - ref64| + 4 u max(1, max|ref64|).

    y_path is the float32-grade path the tail replaces, on the same operands (exact-f32 GEMM, float64 statistics rounded to float32,
    regtr_instnorm_apply).  Per cloud, because the path's error differs between clouds: a one-row cloud normalises (u - mean) with rstd =
    eps^-1/2 = 316, which turns the path's GEMM rounding into 3e-5 there, and taken over the whole batch that would excuse anything in the
    others.  The floor is the rounding of the output itself: the normalised sum, the addition of the two sources, the LeakyReLU product and
    the store each round once (<= u |y|); a path that is exact on a tiny cloud must not demand more than that.
    stat_term (per element): the tail normalises with the statistics IT computed (float32-accumulated moments), the path with float64 ones
    -- y - y64 = (u - mean64)(rstd_k - rstd64) + rstd_k (mean64 - mean_eff) exactly, summed over the sources, where rstd_k is the value the
    kernel reports and uses and mean_eff = sum_a fl(m_a) W_aj (the operands are centred by float32 input means m_a): |mean_eff - mean64| <=
    |mean_k - mean64| + u |mean_k| + u sum_a |m_a| |W_aj|.  The reported statistics are checked against their own derived bound
    (moment_stats_bound), so this term is no looser than that check.  -> (worst ratio, its excess, its path error)"""
    floor = 4 * U * max(1.0, ref.abs().max().item())
    e_path = (y_path.double() - ref).abs().amax(1)
    e_ex = ((y.double() - ref).abs() - stat_term).amax(1)
    z = torch.full((n_clouds,), -math.inf, dtype=torch.float64, device=ref.device)
    p_c = z.clone().scatter_reduce_(0, rows, e_path, 'amax')
    x_c = z.clone().scatter_reduce_(0, rows, e_ex, 'amax')
    live = torch.isfinite(p_c)
    ratio = x_c[live] / (2 * p_c[live] + floor)
    i = int(ratio.argmax())
    return ratio[i].item(), x_c[live][i].item(), p_c[live][i].item()


def _stat_term(u_c, mu64, r64, got, mean_in, W, rows):
    """Per element of one source (see tail_output_ratio): |u - mean64| |rstd_k - rstd64| + rstd_k (|mean_k - mean64| + u |mean_k| +
    u sum_a |m_a| |W_aj|)."""
    g = got.double()
    dr = (g[..., 1] - r64).abs()
    dmu = (g[..., 0] - mu64).abs() + U * g[..., 0].abs() + U * (mean_in.abs() @ W.double().abs())
    return u_c.abs() * dr[rows] + (g[..., 1] * dmu)[rows]


def _tail_inputs(lens, K1, K2, N, seed, hazards=True):
    """x1 / f with the hazards of real encoder data: every cloud's first row an outlier 8 sigma out, a channel nearly constant at offset 50
    and one riding on the same offset, correlated channels; W2's column 7 nearly dead (eps dominates its rstd)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    M = sum(lens)
    x1 = torch.randn((M, K1), device='cuda', generator=g) * (torch.rand(K1, device='cuda', generator=g) * 2.7 + 0.3) \
        + (torch.rand(K1, device='cuda', generator=g) - 0.5) * 4
    f = torch.randn((M, K2), device='cuda', generator=g) * (torch.rand(K2, device='cuda', generator=g) * 1.7 + 0.3) \
        + (torch.rand(K2, device='cuda', generator=g) - 0.5) * 2
    if hazards and M:
        f[:, 5] = 0.25 * f[:, 4] + 3.0
        f[:, 6] = 50.0 + 1e-3 * f[:, 6]
        f[:, 7] += 50.0
        first = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]])[np.array(lens) > 0], device='cuda').long()
        x1[first] = x1.mean(0) + 8 * x1.std(0, correction=0)
        f[first] = f.mean(0) - 8 * f.std(0, correction=0)
    w1 = torch.randn((K1, N), device='cuda', generator=g) / math.sqrt(K1)
    w2 = torch.randn((K2, N), device='cuda', generator=g) / math.sqrt(K2)
    w2[:, 7] *= 1e-3
    return x1.contiguous(), f.contiguous(), w1.contiguous(), w2.contiguous()


def _call_block_tail(A1, a1_stats, row_div, A2, W1, W2, lens, seg, N, ldy_pad=4, with_stats=True):
    lib = _lib()
    L = lib.lib()
    from regtr_amd import ops
    M, K1 = A1.shape
    K2 = A2.shape[1] if A2 is not None else 0
    n_clouds, max_len = len(lens), max(lens)
    assert dispatch.route_block_tail(M, N, K1, K2) != 'refused'
    nb = L.regtr_block_tail_ws_bytes(n_clouds, max_len, N, K1, K2)
    assert nb == dispatch.block_tail_ws_bytes(n_clouds, max_len, N, K1, K2)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    ti = ops.tile_segments(seg, M, 256)
    buf, y = _boxed(M, N, N + ldy_pad)
    S = 2 if K2 else 1
    sbuf, st = _boxed(S * n_clouds, 2 * N) if with_stats else (None, None)
    lib.check(L.regtr_block_tail(A1.data_ptr(), A1.stride(0), lib.ptr(a1_stats), SLOPE, lib.ptr(row_div), A2.data_ptr() if A2 is not None else None,
                                 A2.stride(0) if A2 is not None else 0, lib.ptr(W1), lib.ptr(W2), lib.iptr(seg), n_clouds, max_len, lib.iptr(ti),
                                 M, N, K1, K2, EPS, SLOPE, y.data_ptr(), N + ldy_pad, lib.bptr(ws), nb, st.data_ptr() if with_stats else None,
                                 lib.stream()), 'regtr_block_tail')
    torch.cuda.synchronize()
    if with_stats:
        _check_boxed(sbuf, st, 'out_stats')
        st = st.view(S, n_clouds, N, 2)
    return buf, y, st


def _apply_path(u32, lens, seg, mu, var, res32=None, mu2=None, var2=None):
    """The float32-grade path: float64 statistics rounded to float32, regtr_instnorm_apply (with the second normalised source)."""
    from regtr_amd import ops
    st = torch.stack((mu, 1.0 / torch.sqrt(var + EPS)), -1).float().contiguous()
    rst = torch.stack((mu2, 1.0 / torch.sqrt(var2 + EPS)), -1).float().contiguous() if res32 is not None else None
    return ops.instnorm_apply(u32.contiguous(), seg, max(lens), st, residual=res32, res_stats=rst, lrelu=True)


TAIL_LENS = [[1], [0, 5, 0], [3] * 70, [511, 512, 513], [2047, 2048, 2049, 4097], [20000, 0, 33001, 12999], [70000]]


@pytest.mark.parametrize('lens', TAIL_LENS)
def test_block_tail_vs_fp64(lens):
    """Level-0 form (K1 32 folded, K2 64, N 128) at ldy = N + 4 against float64 of LeakyReLU(IN(x1' W1) + IN(f W2)), x1' =
    LeakyReLU(IN(x1)) by the float32 statistics the kernel is given; out_stats against float64 of the exact products."""
    from regtr_amd import ops
    K1, K2, N = 32, 64, 128
    M = sum(lens)
    seg = _seg(lens)
    rows = _rows_cloud(lens, 'cuda')
    x1, f, w1, w2 = _tail_inputs(lens, K1, K2, N, seed=M + len(lens))
    x1_st = ops.instnorm_stats(x1, seg, max(lens))
    buf, y, st = _call_block_tail(x1, x1_st, None, f, w1, w2, lens, seg, N)
    _check_boxed(buf, y, 'Y')
    s = x1_st.double()[rows]
    xn = torch.nn.functional.leaky_relu((x1.double() - s[..., 0]) * s[..., 1], float(np.float32(SLOPE)))
    m1, mu1, v1 = prod_stats64(xn, lens, w1)
    m2, mu2, v2 = prod_stats64(f, lens, w2)
    u1, u2 = xn @ w1.double() - mu1[rows], f.double() @ w2.double() - mu2[rows]
    r1, r2 = 1 / torch.sqrt(v1 + EPS), 1 / torch.sqrt(v2 + EPS)
    ref = torch.nn.functional.leaky_relu(u1 * r1[rows] + u2 * r2[rows], float(np.float32(SLOPE)))
    # out_stats
    b1 = moment_stats_bound(xn, lens, w1, pivot_of(xn, lens), m1, mu1, v1, 2 * U)
    b2 = moment_stats_bound(f.double(), lens, w2, pivot_of(f, lens), m2, mu2, v2, 0.0)
    rs = max(out_stats_ratio(st[0], lens, mu1, v1, *b1), out_stats_ratio(st[1], lens, mu2, v2, *b2))
    # output
    u1p = ops.gemm(x1, w1, a_stats=x1_st, a_seg_off=seg)                     # exact-f32 kernel, the fold included
    u2p = ops.gemm(f, w2)
    yp = _apply_path(u1p, lens, seg, mu1, v1, u2p, mu2, v2)
    term = _stat_term(u1, mu1, r1, st[0], m1, w1, rows) + _stat_term(u2, mu2, r2, st[1], m2, w2, rows)
    ro, excess, errp = tail_output_ratio(y, ref, yp, term, rows, len(lens))
    # sensitivity: a float64 tail whose weights lost their third plane fails the output check
    w1t, w2t = two_planes(w1), two_planes(w2)
    _, mu1t, v1t = prod_stats64(xn, lens, w1t)
    _, mu2t, v2t = prod_stats64(f, lens, w2t)
    yt = torch.nn.functional.leaky_relu((xn @ w1t.double() - mu1t[rows]) / torch.sqrt(v1t + EPS)[rows]
                                        + (f.double() @ w2t.double() - mu2t[rows]) / torch.sqrt(v2t + EPS)[rows], float(np.float32(SLOPE)))
    rt = tail_output_ratio(yt, ref, yp, term, rows, len(lens))[0]
    print(f'block tail lens {lens[:4]}{"..." if len(lens) > 4 else ""}: output err/allowed {ro:.3f} (excess {excess:.2e}, path {errp:.2e}), '
          f'out_stats err/bound {rs:.3f}, two-plane weights {rt:.1f}')
    assert ro <= 1 and rs <= 1
    if M > 1:
        assert rt > 1, f'a tail without the third weight plane passes the output check ({rt:.2f})'
    if max(lens) > 4096:        # out_stats that omit one 2048-row chunk fail their check
        c = int(np.argmax(lens))
        o = int(np.sum(lens[:c]))
        keep = torch.ones(M, dtype=torch.bool, device='cuda')
        keep[o + 2048:o + 4096] = False
        lens_d = list(lens)
        lens_d[c] -= 2048
        _, mu_d, v_d = prod_stats64(xn[keep], lens_d, w1)
        fake = torch.stack((mu_d, 1 / torch.sqrt(v_d + EPS)), -1)
        fake[torch.tensor(lens, device='cuda') == 0] = 0
        assert out_stats_ratio(fake, lens, mu1, v1, *b1) > 1, 'statistics without a 2048-row chunk pass the out_stats check'


def _first_block_check(wf, num, w16, lens, seg, y, st):
    """y, out_stats of the first-block form against float64 of the rows it read: x = WF / num (float64 quotient of the float32 operands)."""
    from regtr_amd import ops
    rows = _rows_cloud(lens, 'cuda')
    x32 = wf / num[:, None]                                                    # the float32 operand the tail forms (x / num)
    x64 = wf.double() / num.double()[:, None]
    m1, mu1, v1 = prod_stats64(x64, lens, w16)
    b1 = moment_stats_bound(x64, lens, w16, pivot_of(x32, lens), m1, mu1, v1, 2 * U)
    rs = out_stats_ratio(st[0], lens, mu1, v1, *b1)
    u1 = x64 @ w16.double() - mu1[rows]
    r1 = 1 / torch.sqrt(v1 + EPS)
    ref = torch.nn.functional.leaky_relu(u1 * r1[rows], float(np.float32(SLOPE)))
    up = ops.gemm(x32.contiguous(), w16)                                      # exact-f32 kernel on the same float32 operand
    yp = _apply_path(up, lens, seg, mu1, v1)
    term = _stat_term(u1, mu1, r1, st[0], m1, w16, rows)
    ro, excess, errp = tail_output_ratio(y, ref, yp, term, rows, len(lens))
    w16t = two_planes(w16)
    _, mu1t, v1t = prod_stats64(x64, lens, w16t)
    yt = torch.nn.functional.leaky_relu((x64 @ w16t.double() - mu1t[rows]) / torch.sqrt(v1t + EPS)[rows], float(np.float32(SLOPE)))
    rt = tail_output_ratio(yt, ref, yp, term, rows, len(lens))[0]
    return ro, rs, rt, excess, errp


H_MAX = 40


@pytest.mark.parametrize('lens', TAIL_LENS)
def test_first_block_direct_vs_fp64(lens):
    """First-block form (K1 16, K2 0, N 64; A1' = A1 / num) on synthetic WF rows at ldy = N + 4: a zero padding column (the gather's 16th),
    a channel nearly constant at offset 50, correlated channels, an outlier first row, a nearly dead output column."""
    M = sum(lens)
    seg = _seg(lens)
    g = torch.Generator(device='cuda').manual_seed(M + 3)
    wf = torch.rand((M, 16), device='cuda', generator=g) * torch.rand(16, device='cuda', generator=g) * 6
    wf[:, 15] = 0
    wf[:, 3] = 50 + 1e-3 * wf[:, 3]
    wf[:, 5] = 0.5 * wf[:, 4] + 0.25
    if M:
        first = torch.tensor(np.concatenate([[0], np.cumsum(lens)[:-1]])[np.array(lens) > 0], device='cuda').long()
        wf[first, :15] = wf[:, :15].mean(0) + 8 * wf[:, :15].std(0, correction=0)
    num = torch.randint(1, 41, (M,), device='cuda', generator=g).float()
    w16 = torch.randn((16, 64), device='cuda', generator=g) / 4
    w16[15] = 0
    w16[:, 9] *= 1e-3
    buf, y, st = _call_block_tail(wf.contiguous(), None, num, None, w16.contiguous(), None, lens, seg, 64)
    _check_boxed(buf, y, 'Y')
    ro, rs, rt, excess, errp = _first_block_check(wf, num, w16, lens, seg, y, st)
    print(f'first block (direct) lens {lens[:4]}: output err/allowed {ro:.3f} (excess {excess:.2e}, path {errp:.2e}), out_stats err/bound {rs:.3f}, '
          f'two-plane weights {rt:.1f}')
    assert ro <= 1 and rs <= 1
    if M > 1:
        assert rt > 1


@pytest.mark.parametrize('records', [False, True])
def test_first_block_kpconv_vs_fp64(records):
    """ops.kpconv_norm_lrelu (the Cin = 1 gather, c1 or c1p with the support records, then the block tail) against float64 in two bounded
    steps: the gather's WF and num (the same call kpconv_norm_lrelu makes) against a float64 KPConv of the same neighbours under the gather's
    bound (tests/test_gpu_gather.py:_verify), and the tail's output and statistics against float64 of WF / max(num, 1)."""
    from regtr_amd import ops
    from tests import test_gpu_gather as gg
    from tests.util import synth_cloud
    rng = np.random.default_rng(11 + records)
    lens = [20000, 0, 1, 9000, 511]
    s = np.concatenate([synth_cloud(rng, n) + 5.0 * i for i, n in enumerate(lens) if n]).astype(np.float32).reshape(-1, 3)
    M = sum(lens)
    r = 0.06
    seg = _seg(lens)
    sd = torch.from_numpy(s).cuda()
    x = torch.from_numpy(rng.uniform(0.5, 2.0, (M, 1)).astype(np.float32)).cuda()
    w = torch.from_numpy((rng.standard_normal((15, 64)) / 4).astype(np.float32)).cuda()
    kp = gg._kp(r)
    idx = ops.CellGrid(sd, seg, M, r).query(sd, seg, M, H_MAX)
    w16 = torch.cat((w, torch.zeros((1, 64), device='cuda'))).contiguous()
    xyzf = torch.cat((sd, x), 1).contiguous() if records else None
    y, st = ops.kpconv_norm_lrelu(sd, sd, idx, x, w16, kp, r * 0.8, seg, max(lens), xyzf=xyzf, want_stats=True)
    wf, num, _ = gg._gather(sd, sd, idx, x, kp, r * 0.8, xyzf=xyzf, ld_wf=16)
    rg = gg._verify(wf, num, sd, sd, idx, x, kp, r * 0.8, rec_flag=(x[:, 0] > 0).float() if records else None)
    ro, rs, rt, excess, errp = _first_block_check(wf.contiguous(), num.contiguous(), w16, lens, seg, y, st)
    print(f'first block (kpconv_norm_lrelu, records {records}): gather err/bound {rg:.3f}, output err/allowed {ro:.3f} (excess {excess:.2e}, '
          f'path {errp:.2e}), out_stats err/bound {rs:.3f}, two-plane weights {rt:.1f}')
    assert ro <= 1 and rs <= 1 and rt > 1


def test_block_tail_beyond_2_gib():
    """Bench geometry: level 0 of a 192-pair forward (384 clouds, Y = M x 128 floats > 2 GiB), checked on sampled rows that include the
    last tile and every cloud's first row, against float64 statistics of the whole clouds."""
    from regtr_amd import ops
    K1, K2, N = 32, 64, 128
    rng = np.random.default_rng(192)
    lens = rng.integers(10500, 13500, 384).tolist()
    M = sum(lens)
    assert M * N * 4 > 2 ** 31
    seg = _seg(lens)
    x1, f, w1, w2 = _tail_inputs(lens, K1, K2, N, seed=192)
    x1_st = ops.instnorm_stats(x1, seg, max(lens))
    y, st = ops.block_tail(x1, x1_st, f, ops.SplitWeight(w1.t().contiguous(), 'nk'), ops.SplitWeight(w2.t().contiguous(), 'nk'), seg,
                           max(lens), want_stats=True)
    torch.cuda.synchronize()
    off = np.concatenate([[0], np.cumsum(lens)])
    samp = np.unique(np.concatenate([np.arange(0, M, 1009), np.arange(M - 300, M), off[:-1], off[1:] - 1]))
    samp_t = torch.from_numpy(samp).cuda()
    rows_all = _rows_cloud(lens, 'cuda')
    rows = rows_all[samp_t]
    s = x1_st.double()
    mu1 = torch.zeros((len(lens), N), dtype=torch.float64, device='cuda')
    v1, mu2, v2 = torch.zeros_like(mu1), torch.zeros_like(mu1), torch.zeros_like(mu1)
    m1 = torch.zeros((len(lens), K1), dtype=torch.float64, device='cuda')
    m2 = torch.zeros((len(lens), K2), dtype=torch.float64, device='cuda')
    rs = 0.0
    for c, n in enumerate(lens):                  # whole clouds, one at a time: their float64 statistics and the out_stats check
        sl = slice(int(off[c]), int(off[c + 1]))
        xn = torch.nn.functional.leaky_relu((x1[sl].double() - s[c, :, 0]) * s[c, :, 1], float(np.float32(SLOPE)))
        a0, a, b = prod_stats64(xn, [n], w1)
        m1[c], mu1[c], v1[c] = a0[0], a[0], b[0]
        b1 = moment_stats_bound(xn, [n], w1, pivot_of(xn, [n]), a0, a, b, 2 * U)
        rs = max(rs, out_stats_ratio(st[0, c:c + 1], [n], a, b, *b1))
        a0, a, b = prod_stats64(f[sl], [n], w2)
        m2[c], mu2[c], v2[c] = a0[0], a[0], b[0]
        b2 = moment_stats_bound(f[sl].double(), [n], w2, pivot_of(f[sl], [n]), a0, a, b, 0.0)
        rs = max(rs, out_stats_ratio(st[1, c:c + 1], [n], a, b, *b2))
    sr = s[rows]
    xs = torch.nn.functional.leaky_relu((x1[samp_t].double() - sr[..., 0]) * sr[..., 1], float(np.float32(SLOPE)))
    u1, u2 = xs @ w1.double() - mu1[rows], f[samp_t].double() @ w2.double() - mu2[rows]
    r1, r2 = 1 / torch.sqrt(v1 + EPS), 1 / torch.sqrt(v2 + EPS)
    ref = torch.nn.functional.leaky_relu(u1 * r1[rows] + u2 * r2[rows], float(np.float32(SLOPE)))
    slens = torch.bincount(rows, minlength=len(lens)).tolist()
    sseg = _seg(slens)
    u1p = ops.gemm(x1[samp_t].contiguous(), w1, a_stats=x1_st, a_seg_off=sseg)
    u2p = ops.gemm(f[samp_t].contiguous(), w2)
    yp = _apply_path(u1p, slens, sseg, mu1, v1, u2p, mu2, v2)
    term = _stat_term(u1, mu1, r1, st[0], m1, w1, rows) + _stat_term(u2, mu2, r2, st[1], m2, w2, rows)
    ro, excess, errp = tail_output_ratio(y[samp_t], ref, yp, term, rows, len(lens))
    print(f'block tail M {M} ({M * N * 4 / 2 ** 30:.2f} GiB of Y), {len(samp)} sampled rows: output err/allowed {ro:.3f} '
          f'(excess {excess:.2e}, path {errp:.2e}), out_stats err/bound {rs:.3f}')
    assert ro <= 1 and rs <= 1
    assert torch.isfinite(y[samp_t]).all()
