"""GPU (-m gpu): the two launch forms of the strip GEMM (csrc/gemm_stream.hip) write the same bits.

Form 1 is one workgroup per (256-row tile, column block) -- k_gemm_strip; form 2 is one workgroup per 256-row tile that loads, folds and
splits its rows once and walks every column block through a two-slot LDS ring -- k_gemm_strip_cols, taken wherever there are two or more
column blocks.  Both run on the same inputs into poisoned C and stat_partial buffers: every word of both buffers, the row padding of C
included, must be equal, every C element and every statistic of a non-empty cloud must have been written, and the product must agree with
float64 at the tolerance of test_gemm_stream_vs_exact_f32.  Shapes are the smallest that reach every path of the walk: one to fifteen slots,
one to four passes per slot, a partial last slot ((64, 96): 64 + 32 columns; (32, 160): 128 + 32), 1 to 9 row tiles (9 is no multiple of the 8 the grid is padded to), waves with no row, and
tiles with one, two, three and no clouds' boundaries inside."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOPE, EPS = 0.1, 1e-5
# (K, N): two column blocks; three blocks of 32; the encoder's wide shapes at every K; eight blocks; fifteen blocks of 32 (the longest walk);
# and one column block, where form 2 must still be the one-shot kernel
# ... and, beside the issue's list, two whose last ring slot is partial (fewer passes than a whole slot: K = 128 slots are one pass wide)
# ... and the remaining shapes the product launches as a column walk
CASES = [(128, 128), (128, 96), (128, 256), (64, 256), (32, 256), (128, 512), (128, 480), (64, 64), (64, 96), (32, 160),
         (64, 512), (64, 192), (32, 192)]
# the (K, N) whose default launch (form 0) is the column walk: csrc/gemm_stream.hip sg_walks_columns
WALKED = {(128, 96), (128, 128), (128, 256), (128, 512), (64, 192), (64, 256), (64, 512), (32, 192), (32, 256)}
# cloud lengths; M = sum in {1, 33, 255, 256, 257, 700, 2049}
LAYOUTS = [[1], [33], [255], [256], [257], [700], [2049],                 # one cloud
           [20, 13], [100, 157], [300, 400],                              # a boundary inside a tile
           [100, 1, 50, 549],                                             # three clouds inside one tile, a 1-row cloud among them
           [100, 700, 1249],                                              # a cloud that spans tiles 0 .. 3
           [130, 0, 125], [0, 256], [1000, 0, 0, 1049]]                   # empty clouds
assert {sum(l) for l in LAYOUTS} == {1, 33, 255, 256, 257, 700, 2049}


def _lib():
    from regtr_amd import _lib
    return _lib


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(form, a, lda, planes, lens, seg, ti, N, K, ldc, a_st, with_stats):
    """regtr_gemm_stream_form into a NaN-filled C[M, ldc] and an all-ones-bytes stat_partial -> (C, stat_partial, finalised statistics)."""
    lib = _lib()
    L = lib.lib()
    M, R = sum(lens), L.regtr_gemm_stream_tile_rows()
    C = torch.full((M, ldc), float('nan'), dtype=torch.float32, device='cuda')
    partial = None
    if with_stats:
        partial = torch.full((((M + R - 1) // R + len(lens)) * N * 2 * 8,), 0xFF, dtype=torch.uint8, device='cuda').view(torch.float64)
    lib.check(L.regtr_gemm_stream_form(a.data_ptr(), lda, planes.data_ptr(), C.data_ptr(), ldc, M, N, K, lib.ptr(a_st), SLOPE, lib.iptr(seg),
                                       len(lens), lib.iptr(ti), lib.dptr(partial), form, lib.stream()), 'regtr_gemm_stream_form')
    st = None
    if with_stats:
        st = torch.full((len(lens), N, 2), float('nan'), dtype=torch.float32, device='cuda')
        lib.check(L.regtr_instnorm_finalize_tiles(lib.dptr(partial), lib.iptr(seg), len(lens), N, R, EPS, st.data_ptr(), lib.stream()),
                  'regtr_instnorm_finalize_tiles')
    return C, partial, st


@pytest.mark.parametrize('K,N', CASES)
def test_forms_write_the_same_bits(K, N):
    from regtr_amd import ops
    from tests.dispatch import sg_cols_per_wg
    L = _lib().lib()
    assert L.regtr_gemm_stream_supported(1, N, K)
    assert (N // sg_cols_per_wg(N, K) >= 2) == ((K, N) != (64, 64))
    g = torch.Generator(device='cuda').manual_seed(1000 * K + N)
    w = torch.randn((N, K), device='cuda', generator=g) / K ** 0.5
    sw = ops.SplitWeight(w, 'nk')
    assert sw.planes is not None
    R = L.regtr_gemm_stream_tile_rows()
    checked64 = False
    for lens in LAYOUTS:
        M = sum(lens)
        seg = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device='cuda')
        ti = ops.tile_segments(seg, M, R)
        wide = torch.randn((M, K + 8), device='cuda', generator=g) * 2 + 0.5
        rows = torch.repeat_interleave(torch.arange(len(lens), device='cuda'), torch.tensor(lens, device='cuda'))
        for fold in ((False, True) if K <= 64 else (False,)):
            a_st = ops.instnorm_stats(wide[:, :K].contiguous(), seg, max(lens)) if fold else None
            # (lda, ldc, statistics): the plain call; rows of A and C longer than K and N; no statistics
            for lda_pad, ldc_pad, with_stats in ((0, 0, True), (8, 4, True), (8, 4, False)):
                a = wide[:, :K].contiguous() if lda_pad == 0 else wide
                tag = (K, N, lens, fold, lda_pad, ldc_pad, with_stats)
                c1, p1, s1 = _launch(1, a, K + lda_pad, sw.planes, lens, seg, ti, N, K, N + ldc_pad, a_st, with_stats)
                c2, p2, s2 = _launch(2, a, K + lda_pad, sw.planes, lens, seg, ti, N, K, N + ldc_pad, a_st, with_stats)
                assert torch.equal(_bits(c1), _bits(c2)), tag                     # the padding too: neither form writes past column N
                assert not torch.isnan(c2[:, :N]).any(), tag                      # every element was written over the poison
                assert ldc_pad == 0 or torch.isnan(c2[:, N:]).all(), tag
                if with_stats:
                    assert torch.equal(_bits(p1), _bits(p2)), tag                 # slots neither form writes hold the poison in both
                    assert torch.equal(_bits(s1), _bits(s2)), tag
                    full = torch.tensor([n > 0 for n in lens], device='cuda')
                    assert torch.isfinite(s2[full]).all(), tag                    # an unwritten partial slot of a cloud would be NaN here
            if not checked64 and M == 2049:
                a64 = wide[:, :K].double()
                if fold:
                    s = a_st.double()[rows]
                    a64 = torch.nn.functional.leaky_relu((a64 - s[..., 0]) * s[..., 1], float(np.float32(SLOPE)))
                ref = a64 @ w.double().t()
                err = (c2[:, :N].double() - ref).abs().max().item()
                print(f'strip columns K {K} N {N} fold {fold}: max abs err vs float64 {err:.2e}, max |ref| {ref.abs().max().item():.2f}')
                assert err < 2e-5 * max(1.0, ref.abs().max().item()), (K, N, fold)
                checked64 = checked64 or not (K <= 64 and not fold)                 # (both operand forms at K <= 64)
    assert checked64


def test_which_form_launches():
    """The launcher's own answer (regtr_gemm_stream_walks_columns, host only) for every supported (K, N): form 1 never walks; form 2 walks
    exactly where there are two or more column blocks -- (64, 64) and every other single-block shape stay on k_gemm_strip; form 0, the
    product's launch, walks exactly the measured shapes."""
    from tests.dispatch import sg_cols_per_wg
    L = _lib().lib()
    seen = set()
    for K in (32, 64, 128):
        for N in range(32, 513, 32):
            assert L.regtr_gemm_stream_supported(1, N, K)
            ncol = N // sg_cols_per_wg(N, K)
            assert L.regtr_gemm_stream_walks_columns(N, K, 1) == 0
            assert L.regtr_gemm_stream_walks_columns(N, K, 2) == int(ncol >= 2), (K, N)
            assert L.regtr_gemm_stream_walks_columns(N, K, 0) == int((K, N) in WALKED), (K, N)
            seen.add((K, N))
    assert WALKED <= seen and L.regtr_gemm_stream_walks_columns(64, 64, 2) == 0
    assert all(L.regtr_gemm_stream_walks_columns(N, K, 2) == 1 for K, N in CASES if (K, N) != (64, 64))


@pytest.mark.parametrize('K,N', [(128, 256), (64, 256), (64, 64)])
def test_ops_switch_selects_the_form(K, N):
    """ops.strip_columns (None: the compiled-in choice per shape; True / False: force) reaches the launcher, and every setting returns the same
    product and statistics -- a strided A among them."""
    from regtr_amd import ops
    g = torch.Generator(device='cuda').manual_seed(K + N)
    lens = [300, 1, 0, 1748]
    M = sum(lens)
    seg = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), device='cuda')
    a = (torch.randn((M, K + 4), device='cuda', generator=g) * 2 + 0.5)[:, :K]
    sw = ops.SplitWeight(torch.randn((N, K), device='cuda', generator=g) / K ** 0.5, 'nk')
    a_st = ops.instnorm_stats(a.contiguous(), seg, max(lens)) if K <= 64 else None
    prev = ops.strip_columns
    assert prev is None
    res = {}
    try:
        for setting in (None, True, False):
            ops.strip_columns = setting
            res[setting] = ops.gemm_stream(a, sw, seg, a_stats=a_st, want_stats=True)
            assert torch.equal(res[setting][0], ops.gemm_stream(a, sw, seg, a_stats=a_st))
    finally:
        ops.strip_columns = prev
    for setting in (True, False):
        assert torch.equal(_bits(res[None][0]), _bits(res[setting][0])) and torch.equal(_bits(res[None][1]), _bits(res[setting][1]))
