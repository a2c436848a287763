"""Tensor-level wrappers over the C ABI (include/regtr_hip.h).  torch is used for device memory and the current
stream only; every arithmetic step runs in libregtr_hip.so.  Nothing here synchronises with the host, with one documented
exception: `KdTree` (the reference-order parity mode) reads its row width back.  Every pointer handed to the library is checked
for device, dtype and contiguity (_lib.ptr / iptr / bptr / dptr)."""
import functools
import math
import operator

import torch

from . import _lib, context
from ._lib import bptr, check, dptr, iptr, ptr, raw, stream


def _ws(nbytes, device):
    """Every workspace a launcher is handed comes from here (tests replace this one function to control what a workspace holds)."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def _ws_as(numel, dtype, device):
    """Typed scratch of `numel` elements: a view of a _ws byte buffer."""
    return _ws(int(numel) * dtype.itemsize, device).view(dtype)


# ------------------------------------------------------------------------------------------------ preprocessing
F16_OPERAND_LIMIT = 65504.0 / 2     # f16 pair operands: largest finite f16 is 65504; weights are audited with a factor of headroom


VOXEL_KEY_MODES = {'origin': 0, 'floor': 1, 'floor_rcp': 2}


def grid_subsample(xyz, seg_off, n_cap, dl, row_order=0, key_mode=0, out_cap=None):
    """xyz (n_cap,3) f32, seg_off (B+1,) i32 [device] -> (out_xyz (n_cap,3) [first out_seg_off[-1] rows live],
    out_seg_off (B+1,) i32 [device]).  Row order: clouds stacked; voxels of a cloud by first appearance (row_order 0) or in
    the reference's libstdc++ unordered_map iteration order (row_order 1, parity mode).  key_mode: 0 the CPU op's voxel rule
    floor((p - origin) / dl), 1 PreprocessorGPU's floor(p / dl), 2 floor(p * (1 / dl)) (include/regtr_hip.h)."""
    L = _lib.lib()
    n_clouds = seg_off.numel() - 1
    out_cap = int(n_cap if out_cap is None else min(out_cap, n_cap))
    out = torch.empty((max(out_cap, 1), 3), dtype=torch.float32, device=xyz.device)
    out_off = torch.empty(n_clouds + 1, dtype=torch.int32, device=xyz.device)
    nb = L.regtr_grid_subsample_ordered_ws_bytes(n_cap, n_clouds, int(row_order))
    ws = _ws(nb, xyz.device)
    check(L.regtr_grid_subsample_ordered(ptr(xyz), iptr(seg_off), n_clouds, n_cap, float(dl), int(row_order), int(key_mode), out_cap, ptr(out),
                                         iptr(out_off), bptr(ws), nb, stream()), 'regtr_grid_subsample_ordered')
    return out, out_off


self_query_kernel = True     # tests / A-B runs: False routes self queries through the per-query kernel as well
SELF_QUERY_MIN_POINTS = 262144      # measured: 38k points (one pair) 48 us vs 15 us per table; 2.4M points (64 pairs) 1.25 vs 1.9 ms


class CellGrid:
    """Support-point cell grid for one radius; serves any number of radius queries (conv + pool tables of a level)."""

    def __init__(self, s_xyz, s_seg_off, ns_cap, radius):
        L = _lib.lib()
        self.n_clouds = s_seg_off.numel() - 1
        self.s_xyz, self.s_seg_off, self.ns_cap, self.radius = s_xyz, s_seg_off, int(ns_cap), float(radius)
        self.nbytes = L.regtr_cellgrid_ws_bytes(self.ns_cap, self.n_clouds)
        self.ws = _ws(self.nbytes, s_xyz.device)
        check(L.regtr_cellgrid_build(ptr(s_xyz), iptr(s_seg_off), self.n_clouds, self.ns_cap, self.radius, bptr(self.ws),
                                     self.nbytes, stream()), 'regtr_cellgrid_build')

    def query(self, q_xyz, q_seg_off, nq_cap, K, want_count=False, order=0):
        """order 0: the K nearest supports of the ball, rows ascending (d2, index) [reference CPU Preprocessor]; 1: the first K by support
        index, rows ascending by index [reference PreprocessorGPU / pytorch3d ball_query]."""
        L = _lib.lib()
        idx = torch.empty((max(nq_cap, 1), K), dtype=torch.int32, device=q_xyz.device)
        cnt = mx = None
        if want_count:
            cnt = torch.empty(max(nq_cap, 1), dtype=torch.int32, device=q_xyz.device)
            mx = torch.zeros(1, dtype=torch.int32, device=q_xyz.device)
        # the grid's own supports: cell-centric kernel (large sets only: one wave per query keeps more of the chip busy on a pair or two)
        if self_query_kernel and q_xyz is self.s_xyz and q_seg_off is self.s_seg_off and self.ns_cap >= SELF_QUERY_MIN_POINTS:
            check(L.regtr_radius_query_self(iptr(self.s_seg_off), self.ns_cap, self.n_clouds, self.radius, int(K), int(order),
                                            bptr(self.ws), self.nbytes, iptr(idx), iptr(cnt), iptr(mx), stream()), 'regtr_radius_query_self')
        else:
            check(L.regtr_radius_query(ptr(q_xyz), iptr(q_seg_off), int(nq_cap), iptr(self.s_seg_off), self.ns_cap,
                                       self.n_clouds, self.radius, int(K), int(order), bptr(self.ws), self.nbytes, iptr(idx), iptr(cnt),
                                       iptr(mx), stream()), 'regtr_radius_query')
        return (idx, cnt, mx) if want_count else idx


class KdTree:
    """Parity mode (cfg.kpconv_ref_row_order): nanoflann-order neighbour tables (csrc/ref_order.hip, in libregtr_parity.so: include/
    regtr_hip_parity.h).  Unlike CellGrid this synchronises with the host (the list capacity must cover the largest in-ball count, known only
    after a first pass)."""

    def __init__(self, s_xyz, s_seg_off, ns_cap):
        L = _lib.parity_lib()
        self.n_clouds = s_seg_off.numel() - 1
        self.s_xyz, self.s_seg_off, self.ns_cap = s_xyz, s_seg_off, int(ns_cap)
        self.nbytes = L.regtr_kdtree_ws_bytes(self.ns_cap, self.n_clouds)
        self.ws = _ws(self.nbytes, s_xyz.device)
        check(L.regtr_kdtree_build(ptr(s_xyz), iptr(s_seg_off), self.n_clouds, self.ns_cap, bptr(self.ws), self.nbytes, stream()),
              'regtr_kdtree_build')

    def query(self, q_xyz, q_seg_off, nq_cap, radius, K, list_cap=128):
        """-> (idx (nq_cap, K) i32 in the reference's row order, max in-ball count (host int))."""
        L = _lib.parity_lib()
        dev = q_xyz.device
        idx = torch.empty((max(nq_cap, 1), K), dtype=torch.int32, device=dev)
        while True:
            st = torch.zeros(2, dtype=torch.int32, device=dev)          # [max in-ball count, traversal-stack overflow]
            sb = L.regtr_kdtree_query_scratch_bytes(int(list_cap))
            scratch = _ws(sb, dev)
            check(L.regtr_kdtree_radius_query(ptr(q_xyz), iptr(q_seg_off), int(nq_cap), ptr(self.s_xyz), iptr(self.s_seg_off),
                                              self.ns_cap, self.n_clouds, float(radius), int(K), int(list_cap), bptr(self.ws),
                                              self.nbytes, bptr(scratch), sb, iptr(idx), None, st.data_ptr(), st.data_ptr() + 4,
                                              stream()), 'regtr_kdtree_radius_query')
            max_count, overflow = (int(v) for v in st.cpu())
            if overflow:
                raise RuntimeError('regtr_kdtree_radius_query: traversal stack overflow (tree deeper than the parity mode supports)')
            if max_count <= list_cap:
                break
            list_cap = max_count                 # a ball held more supports than the list: the sort needs them all, run again
        return idx, max_count


# ------------------------------------------------------------------------------------------------ dense
class SplitWeight:
    """A weight matrix prepared for both dense kernels: `kn` (K, N) float32 for regtr_gemm_f32 and, when N is a multiple
    of 64, the three bf16 planes of its exact 3-way split for regtr_gemm_x3.  Build once per parameter (cache it)."""

    def __init__(self, w, layout):
        """w: float32 CUDA tensor; layout 'nk' = (N, K) as nn.Linear stores it, 'kn' = (K, N)."""
        L = _lib.lib()
        w = w.detach().contiguous()
        if layout == 'nk':
            self.N, self.K = w.shape
            self.kn = w.t().contiguous()
        else:
            self.K, self.N = w.shape
            self.kn = w
        self.planes = None
        self._w, self._layout, self._planes16, self._f16_ok = w, layout, None, None
        if L.regtr_gemm_x3_supported(1, self.N, self.K) or L.regtr_gemm_stream_supported(1, self.N, self.K):
            self.planes = _ws(L.regtr_gemm_split_weights_bytes(self.N, self.K), w.device)
            check(L.regtr_gemm_split_weights(ptr(w), w.stride(0), self.N, self.K, 0 if layout == 'nk' else 1, bptr(self.planes),
                                             stream()), 'regtr_gemm_split_weights')


    @property
    def f16_ok(self):
        """The weights fit the f16 pair format's range (audited once per weight version: one small reduction + read-back; a weight
        at or beyond 65504 would make every product non-finite, so such a matrix stays on the bf16x3 planes)."""
        if self._f16_ok is None:
            self._f16_ok = bool(self._w.numel() == 0 or float(self._w.abs().max()) < F16_OPERAND_LIMIT)
        return self._f16_ok

    @property
    def planes16(self):
        """The f16 pair planes of regtr_gemm_split_weights_f16 (regtr_gemm_x3's n_planes = 4), built on first use."""
        if self._planes16 is None:
            L = _lib.lib()
            if not self.f16_ok:
                raise RuntimeError('SplitWeight.planes16: a weight of magnitude >= 65504 cannot take the f16 pair format (check .f16_ok)')
            self._planes16 = _ws(L.regtr_gemm_split_weights_f16_bytes(self.N, self.K), self._w.device)
            check(L.regtr_gemm_split_weights_f16(ptr(self._w), self._w.stride(0), self.N, self.K, 0 if self._layout == 'nk' else 1,
                                                 bptr(self._planes16), stream()), 'regtr_gemm_split_weights_f16')
        return self._planes16


# float32-grade contractions as three f16 MFMA terms (the f16 pair split, csrc/gemm_x3.hip) where the row-strip kernel serves the shape,
# instead of six (planes = 3) / three (planes = 2) bf16 terms: what cfg.compute_dtype 'fp32' asks for.  Whether a given launch takes the format
# is a field of the per-forward context (context.current().f16_pair, set by RegTR.forward; `with ops.f16_pair(flag):` for tests and direct op
# calls) -- not a module global: two models on two host threads do not share it.
_f16_shape = {}


def f16_pair(on):
    """`with ops.f16_pair(True):` -- the enclosed launches (this thread) take the f16 pair format where it is served."""
    return context.current().derive(f16_pair=bool(on))


def f16_pair_ok(M, N, K, with_stats=False):
    key = (M, N, K, bool(with_stats))
    v = _f16_shape.get(key)
    if v is None:
        if len(_f16_shape) > 4096:
            _f16_shape.clear()
        v = _f16_shape[key] = bool(_lib.lib().regtr_gemm_x3_f16_supported(M, N, K, 1 if with_stats else 0))
    return v


class _GemmTimer:
    """bench.py's roofline_gemm: HIP events around one dense launch on its stream + what ran (context.recording(gemm_records=[...]))."""
    __slots__ = ('rec', 'e0', 'meta')

    def __init__(self, rec, **meta):
        self.rec, self.meta = rec, meta
        if rec is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def done(self, **more):
        if self.rec is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.rec.append((self.e0, e1, dict(self.meta, **more)))


_x3_shape = {}       # (M, N, K) -> (supported, preferred, workspace bytes, statistics tile rows, launch tile rows): host-side plan queries, memoised


def _x3_plan(M, N, K):
    p = _x3_shape.get((M, N, K))
    if p is None:
        L = _lib.lib()
        ok = bool(L.regtr_gemm_x3_supported(M, N, K))
        p = (ok, bool(ok and L.regtr_gemm_x3_preferred(M, N, K)), L.regtr_gemm_x3_ws_bytes(M, N, K) if ok else 0,
             (L.regtr_gemm_x3_stat_tile_rows(M, N, K) if M > 0 else 0) if ok else 0, L.regtr_gemm_x3_tile_rows(M, N, K) if ok else 0)
        if len(_x3_shape) > 4096:
            _x3_shape.clear()
        _x3_shape[(M, N, K)] = p
    return p


def gemm(a, b, bias=None, row_div=None, residual=None, relu=False, out=None, a_stats=None, a_seg_off=None, a_slope=0.1,
         want_stats=None, eps=1e-5, planes=3):
    """a (M,K) @ b with the fused epilogue of regtr_gemm_f32 / regtr_gemm_x3.  b: a (K,N) float32 tensor (exact-f32 MFMA
    kernel) or a SplitWeight (bf16x3 split kernel when the shape allows).  `a` may be a row-strided view.
    a_stats (n_seg,K,2) + a_seg_off: A is read as LeakyReLU(InstanceNorm(a)) (per-cloud stats) on the fly.
    want_stats = (seg_off, max_len): also return the per-cloud InstanceNorm (mean, rstd) table (n_clouds,N,2) of the
    result -- from the GEMM epilogue when the kernel supports it, else by a pass over the result.
    planes: bf16 planes per operand on the split kernel -- 3 float32-grade (default), 2 three-term split, 1 plain bf16."""
    L = _lib.lib()
    M, K = a.shape
    sw = b if isinstance(b, SplitWeight) else None
    b_kn = sw.kn if sw is not None else b
    Kb, N = b_kn.shape
    assert K == Kb and a.stride(1) == 1 and b_kn.is_contiguous()
    # the shallow encoder levels' Linears (short K, millions of rows, statistics wanted): one-shot strip kernel
    if (sw is not None and sw.planes is not None and want_stats is not None and bias is None and row_div is None and residual is None
            and not relu and planes == 3 and out is None and stream_ok(M, N, K, a, a_stats)
            and (a_stats is None or a_seg_off is want_stats[0])):
        tm = _GemmTimer(context.current().gemm_records, M=M, N=N, K=K, route='one-shot strip (bf16x3)', terms=6, w_bytes=6, fold=a_stats is not None, stats=True)
        res = gemm_stream(a, sw, want_stats[0], a_stats=a_stats, a_slope=a_slope, want_stats=True, eps=eps)
        tm.done()
        return res
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    ldr = residual.stride(0) if residual is not None else 0
    lda = a.stride(0) if M > 1 else K
    ldc = out.stride(0) if M > 1 else N
    n_seg = a_seg_off.numel() - 1 if a_stats is not None else 0
    x3_ok, x3_pref, nb, x3_R, x3_rows = _x3_plan(M, N, K) if sw is not None and sw.planes is not None else (False, False, 0, 0, 0)
    # (N = 32, the level-0 KPConv contractions, stay on the exact-f32 kernel: a pure A stream on which the six-term bf16 strip loses, 1.20 vs
    #  1.14 ms, and the f16 pair strip ties -- 27.71 vs 27.73 ms per forward, docs/NEGATIVES.md)
    ctx = context.current()
    use_f16_pair = ctx.f16_pair and not ctx.force_x3
    if ctx.force_x3:
        planes = 3
    f16_range_log = ctx.f16_range_log
    if (x3_ok and lda % 4 == 0 and a.data_ptr() % 16 == 0 and not force_f32_gemm and (N >= 64 or a_stats is None)
            and (force_x3_gemm or x3_pref)):
        ws = _ws(nb, a.device) if nb else None
        R = x3_R if want_stats is not None else 0
        partial, s_off, n_clouds = None, None, 0
        if R:
            s_off = want_stats[0]
            n_clouds = s_off.numel() - 1
            partial = _ws_as(((M + R - 1) // R + n_clouds) * N * 2, torch.float64, a.device)
        seg_rows = s_off if R else a_seg_off                    # the cloud table of the rows, when the launch needs one
        ti = None
        if seg_rows is not None and (a_seg_off is None or s_off is None or a_seg_off is s_off):
            ti = tile_segments(seg_rows, M, x3_rows)
        pl, npl = sw.planes, int(planes)
        if use_f16_pair and npl >= 2 and sw.f16_ok and f16_pair_ok(M, N, K, R > 0 or a_stats is not None or ti is not None):
            pl, npl = sw.planes16, 4
            if f16_range_log is not None:      # tests / audits: the largest operand magnitude handed to the f16 pair format (synchronises)
                f16_range_log.append((M, N, K, float(a.abs().max()) if M else 0.0, float(sw.kn.abs().max())))
        tm = _GemmTimer(ctx.gemm_records, M=M, N=N, K=K, route='split GEMM (f16 pair)' if npl == 4 else f'split GEMM (bf16 x{npl})',
                        terms={4: 3, 3: 6, 2: 3, 1: 1}[npl], w_bytes={4: 4, 3: 6, 2: 4, 1: 2}[npl], fold=a_stats is not None, stats=R > 0)
        check(L.regtr_gemm_x3(raw(a), lda, bptr(pl), raw(out), ldc, M, N, K, ptr(bias), ptr(row_div),
                              raw(residual), ldr, 1 if relu else 0,
                              ptr(a_stats), iptr(a_seg_off), n_seg, a_slope, bptr(ws), nb, dptr(partial), iptr(s_off), n_clouds,
                              npl, iptr(ti), ctx.status_ptr(), stream()), 'regtr_gemm_x3')
        tm.done()
        if R:
            stats = torch.empty((n_clouds, N, 2), dtype=torch.float32, device=a.device)
            check(L.regtr_instnorm_finalize_tiles(dptr(partial), iptr(s_off), n_clouds, N, R, eps, ptr(stats), stream()),
                  'regtr_instnorm_finalize_tiles')
            return out, stats
    else:
        nb = L.regtr_gemm_f32_ws_bytes(M, N, K)
        ws = _ws(nb, a.device) if nb else None
        tm = _GemmTimer(ctx.gemm_records, M=M, N=N, K=K, route='exact-f32 MFMA', terms=0, w_bytes=4, fold=a_stats is not None, stats=False)
        check(L.regtr_gemm_f32(raw(a), lda, ptr(b_kn), N, raw(out), ldc, M, N, K, ptr(bias), ptr(row_div),
                               raw(residual), ldr, 1 if relu else 0,
                               ptr(a_stats), iptr(a_seg_off), n_seg, a_slope, bptr(ws), nb, stream()), 'regtr_gemm_f32')
        tm.done()
    if want_stats is not None:
        return out, instnorm_stats(out, want_stats[0], want_stats[1], eps)
    return out


def tile_segments(seg_off, M, rows):
    """(n_tiles, 4) int32 table of regtr_tile_segments for the rows described by `seg_off`, cached on the offsets tensor itself (one
    tiny launch per pyramid level and tile height per forward)."""
    cache = getattr(seg_off, '_regtr_tiles', None)
    if cache is None:
        cache = seg_off._regtr_tiles = {}
    key = (M, rows, seg_off.data_ptr(), seg_off._version)      # an offsets tensor refilled in place must not serve stale cloud boundaries
    t = cache.get(key)
    if t is None:
        t = torch.empty(((M + rows - 1) // rows, 4), dtype=torch.int32, device=seg_off.device)
        check(_lib.lib().regtr_tile_segments(iptr(seg_off), seg_off.numel() - 1, M, rows, iptr(t), stream()), 'regtr_tile_segments')
        for k in [k for k in cache if k[2:] != key[2:]]:           # tables of the tensor's earlier contents
            del cache[k]
        cache[key] = t
    return t


def stream_ok(M, N, K, a, a_stats=None):
    """The one-shot strip kernel (csrc/gemm_stream.hip) serves this product and is the faster choice (tall problems only)."""
    return bool(use_stream_gemm and not force_f32_gemm and not force_x3_gemm and M >= STREAM_MIN_ROWS and a.stride(1) == 1
                and a.stride(0) % 4 == 0 and a.data_ptr() % 16 == 0 and (a_stats is None or K <= 64)
                and _lib.lib().regtr_gemm_stream_supported(M, N, K))


def gemm_stream(a, sw, seg_off, a_stats=None, a_slope=0.1, want_stats=False, eps=1e-5):
    """regtr_gemm_stream: a' @ W for K in {32, 64, 128}, N <= 512 on millions of rows (see csrc/gemm_stream.hip).
    want_stats: also return the per-cloud InstanceNorm (mean, rstd) table of the result.  -> out | (out, stats)"""
    L = _lib.lib()
    M, K = a.shape
    N = sw.N
    n_clouds = seg_off.numel() - 1
    R = L.regtr_gemm_stream_tile_rows()
    ti = tile_segments(seg_off, M, R)
    partial = None
    if want_stats:
        partial = _ws_as(((M + R - 1) // R + n_clouds) * N * 2, torch.float64, a.device)
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    form = 0 if strip_columns is None else (2 if strip_columns else 1)
    check(L.regtr_gemm_stream_form(raw(a), a.stride(0) if M > 1 else K, bptr(sw.planes), ptr(out), N, M, N, K, ptr(a_stats), a_slope,
                                   iptr(seg_off), n_clouds, iptr(ti), dptr(partial), form, stream()), 'regtr_gemm_stream_form')
    if not want_stats:
        return out
    stats = torch.empty((n_clouds, N, 2), dtype=torch.float32, device=a.device)
    check(L.regtr_instnorm_finalize_tiles(dptr(partial), iptr(seg_off), n_clouds, N, R, eps, ptr(stats), stream()),
          'regtr_instnorm_finalize_tiles')
    return out, stats


def block_tail_ok(x1, x1_stats, f, sw1, sw2):
    """regtr_block_tail serves this resnet-block tail (shape, alignment, size) and is switched on."""
    M, K1 = x1.shape
    return bool(use_block_tail and not force_f32_gemm and not force_x3_gemm and M >= STREAM_MIN_ROWS and f.shape[0] == M
                and x1_stats is not None and sw1.N == sw2.N and x1.stride(1) == 1 and f.stride(1) == 1
                and x1.stride(0) % 4 == 0 and f.stride(0) % 4 == 0 and x1.data_ptr() % 16 == 0 and f.data_ptr() % 16 == 0
                and x1_stats.data_ptr() % 16 == 0 and _lib.lib().regtr_block_tail_supported(M, sw1.N, K1, f.shape[1]))


def block_tail(x1, x1_stats, f, sw1, sw2, seg_off, max_len, slope=0.1, eps=1e-5, want_stats=False):
    """LeakyReLU(InstanceNorm(x1' @ W1) + InstanceNorm(f @ W2)), x1' = LeakyReLU(InstanceNorm(x1)) by x1_stats: the tail of a resnet
    bottleneck block with a Linear shortcut (kpconv_blocks.py:727-741) without writing either product (csrc/block_tail.hip).
    sw1 / sw2: SplitWeight of unary2 / unary_shortcut.  want_stats: also return the (2, n_clouds, N, 2) (mean, rstd) of the products."""
    return _block_tail(x1, x1_stats, None, f, sw1.kn, sw2.kn, seg_off, max_len, slope, eps, want_stats)


def _block_tail(x1, x1_stats, row_div, f, w1_kn, w2_kn, seg_off, max_len, slope, eps, want_stats):
    L = _lib.lib()
    M, K1 = x1.shape
    K2, N = (f.shape[1] if f is not None else 0), w1_kn.shape[1]
    n_clouds = seg_off.numel() - 1
    nb = L.regtr_block_tail_ws_bytes(n_clouds, int(max_len), N, K1, K2)
    ws = _ws(nb, x1.device)       # sized per call, used across four launches
    ti = tile_segments(seg_off, M, 256)
    y = torch.empty((M, N), dtype=torch.float32, device=x1.device)
    st = torch.empty((2 if K2 else 1, n_clouds, N, 2), dtype=torch.float32, device=x1.device) if want_stats else None
    tm = _GemmTimer(context.current().gemm_records, M=M, N=N, K=K1 + K2, route='block tail (moments + two-source strip, bf16x3)', terms=6, w_bytes=6,
                    fold=True, stats=True, passes=2)
    check(L.regtr_block_tail(raw(x1), x1.stride(0), ptr(x1_stats), slope, ptr(row_div), raw(f) if f is not None else None,
                             f.stride(0) if f is not None else 0, ptr(w1_kn), ptr(w2_kn), iptr(seg_off), n_clouds, int(max_len),
                             iptr(ti), M, N, K1, K2, eps, slope, ptr(y), N, bptr(ws), nb, ptr(st), stream()), 'regtr_block_tail')
    tm.done()
    return (y, st) if want_stats else y


def first_block_ok(nq, Cin, KP, Cout):
    """kpconv_norm_lrelu serves the encoder's first block (one input feature, 15 kernel points, 64 outputs, a tall batch)."""
    return bool(use_block_tail and not force_f32_gemm and not force_x3_gemm and Cin == 1 and KP == 15 and nq >= STREAM_MIN_ROWS
                and _lib.lib().regtr_block_tail_supported(nq, Cout, 16, 0))


def kpconv_norm_lrelu(q_xyz, s_xyz, nbr, x, w16_kn, kernel_points, extent, seg_off, max_len, xyzf=None, slope=0.1, eps=1e-5,
                      want_stats=False):
    """SimpleBlock with one input feature (kpconv_blocks.py:590-646): KPConv -> InstanceNorm -> LeakyReLU.  The gather writes its
    15 weighted sums per query as 16-float rows; the contraction, the InstanceNorm (statistics from the rows' 16 x 16 second
    moments) and the LeakyReLU are one pass over them (regtr_block_tail, K2 = 0).  w16_kn: the (15, Cout) weights padded to (16, Cout)."""
    L = _lib.lib()
    nq, H = nbr.shape
    ns = x.shape[0]
    KP = kernel_points.shape[0]
    wf = torch.empty((nq, 16), dtype=torch.float32, device=x.device)
    num = torch.empty(nq, dtype=torch.float32, device=x.device)
    rec = context.current().gather_records           # bench.py's roofline: this gather is one of a forward's KPConv gather launches too
    if rec is not None:
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
    check(L.regtr_kpconv_gather(ptr(q_xyz), nq, ptr(s_xyz), ns, iptr(nbr), H, ptr(x), 1, None, ptr(xyzf), ptr(kernel_points), KP,
                                float(extent), None, None, 0, slope, ptr(wf), 16, ptr(num), stream()), 'regtr_kpconv_gather')
    if rec is not None:
        e1.record()
    res = _block_tail(wf, None, num, None, w16_kn, None, seg_off, max_len, slope, eps, want_stats)
    if rec is not None:
        e2.record()
        rec.append((e0, e1, e2, nq, H, 1, w16_kn.shape[1]))
    return res


STREAM_MIN_ROWS = 131072     # below this a forward is launch-bound (a pair or two): the tiled kernels and separate passes are as fast
# The SMALL-batch regime: forwards with fewer level-0 rows than this take the small-batch kernel forms at EVERY level (no packed support
# records / pre-normalised gather, no strip GEMM, no block tails) and the encoder's blocks go out through one C call (regtr_encoder_fwd).
# Measured with the one-call encoder (profiles/r05_ab_h.txt: bench.py --pairs n, small regime forced on / off): 2 pairs 3.01 vs 3.30 ms, 3 pairs
# 3.32 vs 3.50, 4 pairs 3.85 vs 3.67, 8 pairs 5.52 vs 5.33 -- the crossover sits between 114 k and 152 k rows.  (Round 4, op-by-op issue: 65536.)
SMALL_REGIME_ROWS = 131072
# Routing switches: plain module attributes, never read from the environment.  Tests and measure.py assign them to take the other path as the reference.
use_stream_gemm = True      # one-shot strip kernel for the shallow levels' Linears
use_block_tail = True       # resnet-block tail / first block from input moments (csrc/block_tail.hip)
# launch form of the strip GEMM's wide outputs (two or more column blocks): None = the measured choice per (K, N) compiled into
# csrc/gemm_stream.hip; True = one workgroup per row tile walks all column blocks; False = one workgroup per column block.  Same bits either way.
strip_columns = None
PRENORM_MIN_ROWS = 65536        # a LEVEL with fewer rows than this (of a large batch): the extra normalise pass costs more than the gather saves
prenorm_gather = True       # unary1's IN + LReLU applied before the gather (packed support records)
# unary2's folded InstanceNorm + LeakyReLU operand is applied by a separate in-place pass instead where the fold would route to the tiled kernel
# (K > 64) and the level has at least this many rows (kpconv.py ResnetBottleneckBlock; a pair or two per forward is launch-bound: the fold saves
# the extra launch there)
PREAPPLY_MIN_ROWS = 8192
# csrc/encoder.hip sequences the small-batch regime with these rules compiled in (ENC_PREAPPLY_ROWS, no strip / block-tail form below
# STREAM_MIN_ROWS): the one-call path equals the op-by-op path only while the gates nest like this (kpconv.KPFEncoder._one_call_ok)
assert PREAPPLY_MIN_ROWS == 8192, 'csrc/encoder.hip compiles this gate in (ENC_PREAPPLY_ROWS)'      # (a SMALL_REGIME_ROWS beyond STREAM_MIN_ROWS: _one_call_ok caps it)
# the six cross-encoder layers enqueued by one C call (regtr_cross_encoder_fwd) instead of 72 op calls
use_one_call_cross_encoder = True
# the encoder's blocks enqueued by one C call (regtr_encoder_fwd) in the small-batch regime (< 65536 level-0 rows) instead of ~130 op calls
use_one_call_encoder = True
force_f32_gemm = False      # tests / A-B runs: route every GEMM to the exact-f32 MFMA kernel
force_x3_gemm = False       # tests: route every supported shape to the split kernel, also where it is not the faster one


def layernorm(x, gamma, beta, add=None, eps=1e-5, want_plain=False, out=None):
    n, D = x.shape
    y = torch.empty_like(x) if out is None else out
    yp = torch.empty_like(x) if want_plain else None
    check(_lib.lib().regtr_layernorm(ptr(x), n, D, ptr(gamma), ptr(beta), eps, ptr(add), ptr(y), ptr(yp), stream()),
          'regtr_layernorm')
    return (y, yp) if want_plain else y


def add(a, b):
    """a + b, same shape, contiguous float32 (with_pos_embed of the post-norm encoder layer)."""
    assert a.shape == b.shape
    out = torch.empty_like(a)
    check(_lib.lib().regtr_add_f32(ptr(a), ptr(b), a.numel(), ptr(out), stream()), 'regtr_add_f32')
    return out


_posemb_tables = {}


def posemb_sine(xyz, d_model, scale=1.0, temperature=10000):
    """PositionEmbeddingCoordsSine.forward (position_embedding.py:29-50).  The 84-entry frequency table is
    init-time constant data computed exactly the way the reference computes it (float32 pow)."""
    n_dim = 3
    npf = d_model // n_dim // 2 * 2
    key = (npf, temperature, float(scale), xyz.device)
    ent = _posemb_tables.get(key)
    if ent is None:          # (once per configuration and device: building these per forward cost a one-pair forward 0.2 ms of host time)
        dim_t = torch.arange(npf, dtype=torch.float32)
        dim_t = (temperature ** (2 * torch.div(dim_t, 2, rounding_mode='trunc') / npf)).to(xyz.device)
        ent = _posemb_tables[key] = (dim_t, torch.tensor(scale * 2 * math.pi, dtype=torch.float32).item())
    dim_t, scale32 = ent
    pe = torch.empty((xyz.shape[0], d_model), dtype=torch.float32, device=xyz.device)
    check(_lib.lib().regtr_posemb_sine(ptr(xyz), xyz.shape[0], npf, d_model, scale32, ptr(dim_t), ptr(pe), stream()),
          'regtr_posemb_sine')
    return pe


POSEMB_MLP_WIDTHS = (3, 32, 64, 128, 256)      # the input widths of PositionEmbeddingLearned's five Linears (the last one's output: d_model)
POSEMB_MLP_ACTS = 480                          # 32 + 64 + 128 + 256: h1 | h2 | h3 | h4, the row of the saved-activations buffer
# A-B switch of the learned positional embedding: regtr_posemb_mlp (one launch, the hidden activations stay in LDS), or the same MLP
# composed from five ops.gemm calls on the exact-f32 kernel (tools/posemb_mlp_bench.py measures both; docs/KERNELS.md)
use_fused_posemb_mlp = True


def _posemb_mlp_check(xyz, weights):
    if not isinstance(xyz, torch.Tensor) or xyz.device.type != 'cuda':
        raise RuntimeError(f'posemb_mlp: xyz must be a GPU tensor (got {getattr(xyz, "device", type(xyz))}); there is no CPU fallback')
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise RuntimeError(f'posemb_mlp: xyz must be (n, 3), got {tuple(xyz.shape)}')
    if len(weights) != 5:
        raise RuntimeError(f'posemb_mlp: five (weight (K, N), bias (N,)) pairs are needed, got {len(weights)}')
    d_model = int(weights[4][0].shape[1])
    widths = POSEMB_MLP_WIDTHS + (d_model,)
    for l, (w, b) in enumerate(weights):
        if tuple(w.shape) != (widths[l], widths[l + 1]) or tuple(b.shape) != (widths[l + 1],):
            raise RuntimeError(f'posemb_mlp: layer {l} must be a ({widths[l]}, {widths[l + 1]}) weight in (K, N) layout and a '
                               f'({widths[l + 1]},) bias, got {tuple(w.shape)} and {tuple(b.shape)}')
    return d_model


def posemb_mlp(xyz, weights, save=False):
    """PositionEmbeddingLearned.forward (position_embedding.py:53-72) in one launch (regtr_posemb_mlp): xyz (n, 3), weights five
    (w (K, N) float32 -- the Linear's weight transposed --, bias (N,)) pairs of the MLP 3 -> 32 -> 64 -> 128 -> 256 -> d_model -> pe
    (n, d_model).  save=True -> (pe, acts): acts (n, 480) = h1 | h2 | h3 | h4, the activations after their ReLUs; pe is the same bits
    either way.  Exact float32 (vector FMAs / the f32 MFMA), float32's operand range.  Nothing here synchronises."""
    if not use_fused_posemb_mlp:
        return posemb_mlp_composed(xyz, weights, save)
    d_model = _posemb_mlp_check(xyz, weights)
    n = xyz.shape[0]
    pe = torch.empty((n, d_model), dtype=torch.float32, device=xyz.device)
    acts = torch.empty((n, POSEMB_MLP_ACTS), dtype=torch.float32, device=xyz.device) if save else None
    w5 = (_lib._c.c_void_p * 5)(*[ptr(w) for w, _ in weights])
    b5 = (_lib._c.c_void_p * 5)(*[ptr(b) for _, b in weights])
    check(_lib.lib().regtr_posemb_mlp(ptr(xyz), n, w5, b5, d_model, ptr(pe), ptr(acts), stream()), 'regtr_posemb_mlp')
    return (pe, acts) if save else pe


def posemb_mlp_composed(xyz, weights, save=False):
    """posemb_mlp from five ops.gemm calls on the exact-f32 kernel (regtr_gemm_f32 takes K = 3), the ReLUs in the epilogues; with save the
    four activations are written as the column blocks of one (n, 480) buffer, as regtr_posemb_mlp lays them out."""
    d_model = _posemb_mlp_check(xyz, weights)
    n = xyz.shape[0]
    acts = torch.empty((n, POSEMB_MLP_ACTS), dtype=torch.float32, device=xyz.device) if save else None
    h, c0 = xyz, 0
    for w, b in weights[:4]:
        N = w.shape[1]
        h = gemm(h, w, bias=b, relu=True, out=acts[:, c0:c0 + N] if save else None)
        c0 += N
    pe = gemm(h, weights[4][0], bias=weights[4][1])
    return (pe, acts) if save else pe


# ------------------------------------------------------------------------------------------------ KPConv encoder
def kpconv(q_xyz, s_xyz, nbr, x, w_flat, kernel_points, extent, x_stats=None, s_seg_off=None, q_seg_off=None, slope=0.1,
           want_stats=None, xyzf=None):
    """KPConv.forward (kpconv_blocks.py:269-414), non-deformable / linear / sum.
    nbr (Nq,H) i32, x (Ns,Cin), w_flat (KP*Cin, Cout) -> (Nq, Cout).
    x_stats (n_clouds,Cin,2): the input features are LeakyReLU(InstanceNorm(x)) applied on the fly (the tail of the
    preceding UnaryBlock, kpconv_blocks.py:556-561), with s_seg_off / q_seg_off the support / query cloud offsets.
    xyzf (Ns,4): (x, y, z, f) records of the supports, f = row-positivity of x as instnorm_apply(row_xyz=, row_positive=) writes
    them (x final, no x_stats), or the feature itself when Cin == 1: one 16-byte load per neighbour in the gather.
    want_stats = (seg_off, max_len) of the QUERY rows: returns (out, InstanceNorm stats of out)."""
    L = _lib.lib()
    assert xyzf is None or x_stats is None
    nq, H = nbr.shape
    ns, Cin = x.shape
    KP = kernel_points.shape[0]
    dev = x.device
    n_seg = s_seg_off.numel() - 1 if x_stats is not None else 0
    # the matrix-core gather derives the positivity flags from the rows it reads; every other case (channel counts / row
    # widths it does not take, unaligned views, >= 2^29 feature elements, no supports) needs them precomputed
    fused_flag = (L.regtr_kpconv_gather_computes_flag(Cin, H) and x.data_ptr() % 16 == 0 and ns > 0 and ns * Cin < (1 << 29)
                  and (x_stats is None or x_stats.data_ptr() % 16 == 0))
    flag = None
    if not fused_flag:
        xyzf = None
        flag = torch.empty(ns, dtype=torch.float32, device=dev)
        check(L.regtr_rowsum_positive(ptr(x), ns, Cin, ptr(x_stats), iptr(s_seg_off) if x_stats is not None else None, n_seg,
                                      slope, ptr(flag), stream()), 'regtr_rowsum_positive')
    wf = torch.empty((nq, KP * Cin), dtype=torch.float32, device=dev)
    num = torch.empty(nq, dtype=torch.float32, device=dev)
    rec = context.current().gather_records
    if rec is not None:
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
    check(L.regtr_kpconv_gather(ptr(q_xyz), nq, ptr(s_xyz), ns, iptr(nbr), H, ptr(x), Cin, ptr(flag), ptr(xyzf),
                                ptr(kernel_points), KP, float(extent), ptr(x_stats),
                                iptr(q_seg_off) if x_stats is not None else None, n_seg, slope, ptr(wf), 0, ptr(num), stream()),
          'regtr_kpconv_gather')
    if rec is not None:
        e1.record()
    res = gemm(wf, w_flat, row_div=num, want_stats=want_stats)       # (out, stats) when want_stats is given
    if rec is not None:
        e2.record()
        rec.append((e0, e1, e2, nq, H, Cin, (res[0] if want_stats is not None else res).shape[1]))
    return res


# (bench.py times every KPConv gather launch with HIP events on the launch stream: context.recording(gather_records=[...]))


def maxpool(x, nbr, width=None):
    """max_pool (kpconv_blocks.py:127-143).  width: use only the first `width` columns of nbr -- the reference's CPU tables are
    min(max in-ball count, K) wide (kpconv.py:255-258), so a full row holds no zero shadow row (parity mode)."""
    ns, C = x.shape
    nq, H = nbr.shape
    out = torch.empty((nq, C), dtype=torch.float32, device=x.device)
    check(_lib.lib().regtr_maxpool_gather(ptr(x), ns, C, iptr(nbr), H, nq, H if width is None else int(width), ptr(out), stream()),
          'regtr_maxpool_gather')
    return out


def instnorm_stats(x, seg_off, max_len, eps=1e-5):
    L = _lib.lib()
    n_clouds = seg_off.numel() - 1
    C = x.shape[1]
    stats = torch.empty((n_clouds, C, 2), dtype=torch.float32, device=x.device)
    nb = L.regtr_instnorm_ws_bytes(n_clouds, max_len, C)
    ws = _ws(nb, x.device)
    check(L.regtr_instnorm_stats(ptr(x), iptr(seg_off), n_clouds, int(max_len), C, eps, ptr(stats), bptr(ws), nb,
                                 stream()), 'regtr_instnorm_stats')
    return stats


def instnorm_apply(x, seg_off, max_len, stats, residual=None, res_stats=None, lrelu=False, slope=0.1, out=None, row_positive=None,
                   row_xyz=None):
    """row_positive: optional (rows,) float32 output, 1.0 where the result's row sum is > 0 (KPConv's normaliser flag); with
    row_xyz (rows,3) it is (rows,4) and receives (x, y, z, flag) records -- the `xyzf` operand of kpconv()."""
    assert row_xyz is None or (row_positive is not None and row_positive.shape == (x.shape[0], 4) and row_xyz.shape == (x.shape[0], 3))
    n_clouds = seg_off.numel() - 1
    C = x.shape[1]
    if out is None:
        out = torch.empty_like(x)
    check(_lib.lib().regtr_instnorm_apply(ptr(x), iptr(seg_off), n_clouds, int(max_len), C, ptr(stats), ptr(residual),
                                          ptr(res_stats), 1 if lrelu else 0, slope, ptr(out), ptr(row_xyz), ptr(row_positive), stream()),
          'regtr_instnorm_apply')
    return out


# ------------------------------------------------------------------------------------------------ attention + pose
def mha(q, k, v, seg_off, kv_of, max_len, n_heads, precision=0):
    """q, k, v: (N, E) column views of a packed projection; returns (N, E) concatenated heads.
    precision: 0 float32-grade (bf16x3 split MFMA), 1 plain bf16 operands, 2 exact-f32 MFMA (see regtr_hip.h)."""
    N, E = q.shape
    hd = E // n_heads
    out = torch.empty((N, E), dtype=torch.float32, device=q.device)
    ctx = context.current()
    rec = ctx.mha_records
    if ctx.force_x3 and precision == 3:
        precision = 0                      # the range fallback: bf16x3 operands (float32's range)
    if rec is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(_lib.lib().regtr_mha_fwd(raw(q), q.stride(0), raw(k), k.stride(0), raw(v), v.stride(0),
                                   ptr(out), E, iptr(seg_off), iptr(kv_of), seg_off.numel() - 1, int(max_len), n_heads, hd,
                                   1.0 / math.sqrt(hd), int(precision), ctx.status_ptr(), stream()), 'regtr_mha_fwd')
    if rec is not None:
        e1.record()
        rec.append((e0, e1))
    return out


def mha_bwd(q, k, v, d_out, seg_off, kv_of, max_len, n_heads, out=None):
    """Backward of the attention core (regtr_mha_bwd): q, k, v, d_out (N, E) row-strided column views as ops.mha takes them -> (dq, dk,
    dv), the three (N, E) column blocks of a packed (N, 3E) buffer -- the layout the in-projection's backward wants.  out: that buffer
    (float32, contiguous), or None for a zero-filled new one; rows outside every cloud are not written.  A function of (q, k, v, d_out)
    only: the forward's output and precision play no part.  Nothing here synchronises."""
    L = _lib.lib()
    N, E = q.shape
    hd = E // n_heads
    if out is None:
        out = torch.zeros((N, 3 * E), dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != (N, 3 * E):
        raise RuntimeError(f'mha_bwd: out must be ({N}, {3 * E}), got {tuple(out.shape)}')
    for t in (q, k, v, d_out):
        if tuple(t.shape) != (N, E) or (E > 1 and t.stride(1) != 1):
            raise RuntimeError(f'mha_bwd: q, k, v and d_out must be ({N}, {E}) views with unit column stride')
    base = ptr(out)
    nb = L.regtr_mha_bwd_ws_bytes(N, n_heads)
    ws = _ws(max(nb, 1), q.device)
    ld = lambda t: t.stride(0) if N > 1 else E
    check(L.regtr_mha_bwd(raw(q), ld(q), raw(k), ld(k), raw(v), ld(v), raw(d_out), ld(d_out),
                          base, 3 * E, base + 4 * E if base else None, 3 * E, base + 8 * E if base else None, 3 * E,
                          iptr(seg_off), iptr(kv_of), seg_off.numel() - 1, N, int(max_len), n_heads, hd, 1.0 / math.sqrt(hd),
                          bptr(ws), nb, stream()), 'regtr_mha_bwd')
    return out[:, :E], out[:, E:2 * E], out[:, 2 * E:]


def layernorm_bwd(x, gamma, dy, dres=None, eps=1e-5, out=None):
    """Backward of ops.layernorm (regtr_layernorm_bwd): x, dy (n, D) contiguous, gamma (D,), dres (n, D) an optional gradient that
    reached x through another branch (added into dx) -> (dx (n, D), dgamma (D,), dbeta (D,)).  Mean and rstd are recomputed from x.
    out: the dx buffer (may be dres itself).  Nothing here synchronises."""
    L = _lib.lib()
    n, D = x.shape
    for name, t in (('dy', dy), ('dres', dres), ('out', out)):
        if t is not None and tuple(t.shape) != (n, D):
            raise RuntimeError(f'layernorm_bwd: {name} must be ({n}, {D}), got {tuple(t.shape)}')
    dx = torch.empty_like(x) if out is None else out
    dgb = torch.zeros((2, D), dtype=torch.float32, device=x.device)       # n = 0: nothing is launched and the sums are 0
    nb = L.regtr_layernorm_bwd_ws_bytes(n, D)
    ws = _ws(max(nb, 1), x.device)
    base = ptr(dgb)
    check(L.regtr_layernorm_bwd(ptr(x), n, D, ptr(gamma), eps, ptr(dy), ptr(dres), ptr(dx), base, base + 4 * D, bptr(ws), nb, stream()),
          'regtr_layernorm_bwd')
    return dx, dgb[0], dgb[1]


def bias_relu_bwd(g, h=None, inplace=False):
    """Column sums of a gradient (regtr_bias_relu_bwd): g (n, N) float32, row-strided with unit column stride.  Without h -> db (N,) =
    sum over rows of g: a Linear's bias gradient.  With h (n, N), the activation stored after the forward's ReLU -> (dh, db): dh = g
    where h > 0 else 0, db its column sums; inplace=True writes dh over g.  Nothing here synchronises."""
    L = _lib.lib()
    n, N = g.shape
    if N > 1 and g.stride(1) != 1:
        raise RuntimeError('bias_relu_bwd: g must have unit column stride')
    dh = None
    if h is not None:
        if tuple(h.shape) != (n, N) or (N > 1 and h.stride(1) != 1):
            raise RuntimeError(f'bias_relu_bwd: h must be ({n}, {N}) with unit column stride, got {tuple(h.shape)}')
        dh = g if inplace else torch.empty((n, N), dtype=torch.float32, device=g.device)
    db = torch.zeros((N,), dtype=torch.float32, device=g.device)          # n = 0: nothing is launched and the sums are 0
    nb = L.regtr_bias_relu_bwd_ws_bytes(n, N)
    ws = _ws(max(nb, 1), g.device)
    ld = lambda t: t.stride(0) if n > 1 else N
    check(L.regtr_bias_relu_bwd(raw(g), ld(g), raw(h), ld(h) if h is not None else 0, raw(dh), ld(dh) if dh is not None else 0, ptr(db),
                                n, N, bptr(ws), nb, stream()), 'regtr_bias_relu_bwd')
    return (dh, db) if h is not None else db


def attn_xyz(q, k, xyz, seg_off, kv_of, max_len):
    """CorrespondenceDecoder.simple_attention: q, k (L, N, D) contiguous, xyz (N, 3) -> (L, N, 3)."""
    Lyr, N, D = q.shape
    out = torch.empty((Lyr, N, 3), dtype=torch.float32, device=q.device)
    check(_lib.lib().regtr_attn_xyz(ptr(q), ptr(k), ptr(xyz), ptr(out), iptr(seg_off), iptr(kv_of), seg_off.numel() - 1, N, Lyr,
                                    int(max_len), D, 1.0 / math.sqrt(D), stream()), 'regtr_attn_xyz')
    return out


def weighted_procrustes(kp, corr, logit, seg_off, n_pairs):
    """kp (N,3), corr (L,N,3), logit (L,N), seg_off (2B+1,) i32 -> pose (L,B,3,4)."""
    Lyr, N = logit.shape
    pose = torch.empty((Lyr, n_pairs, 3, 4), dtype=torch.float32, device=kp.device)
    check(_lib.lib().regtr_weighted_procrustes(ptr(kp), ptr(corr), ptr(logit), iptr(seg_off), n_pairs, N, Lyr, ptr(pose),
                                               context.current().status_ptr(), stream()), 'regtr_weighted_procrustes')
    return pose


def weighted_procrustes_bwd(kp, corr, logit, seg_off, n_pairs, d_pose, want_logit=True, want_kp=False, want_weight=False):
    """The backward of weighted_procrustes (regtr_weighted_procrustes_bwd): its inputs and d_pose (L, B, 3, 4) ->
    (d_corr (L, N, 3), d_logit (L, N) | None, d_kp (L, N, 3) | None, d_weight (L, N) | None).  d_kp is per layer (kp's gradient is its sum
    over L); d_weight is the gradient with respect to sigmoid(logit).  Nothing is saved by the forward; a pair whose pose is not
    differentiable (include/regtr_hip.h) gets zero rows."""
    for t in (kp, corr, logit, seg_off, d_pose):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise RuntimeError(f'weighted_procrustes_bwd: every tensor must be on the GPU (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    Lyr, N = logit.shape
    if tuple(corr.shape) != (Lyr, N, 3) or tuple(kp.shape) != (N, 3) or tuple(d_pose.shape) != (Lyr, n_pairs, 3, 4) or \
            seg_off.numel() != 2 * n_pairs + 1:
        raise RuntimeError(f'weighted_procrustes_bwd: kp (N, 3), corr (L, N, 3), logit (L, N), seg_off (2B + 1,), d_pose (L, B, 3, 4) expected, '
                           f'got {tuple(kp.shape)}, {tuple(corr.shape)}, {tuple(logit.shape)}, {tuple(seg_off.shape)}, {tuple(d_pose.shape)}')
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=kp.device)
    d_corr = new(Lyr, N, 3)
    d_logit = new(Lyr, N) if want_logit else None
    d_kp = new(Lyr, N, 3) if want_kp else None
    d_weight = new(Lyr, N) if want_weight else None
    check(_lib.lib().regtr_weighted_procrustes_bwd(ptr(kp), ptr(corr), ptr(logit), iptr(seg_off), n_pairs, N, Lyr, ptr(d_pose), ptr(d_corr),
                                                   ptr(d_logit), ptr(d_kp), ptr(d_weight), stream()), 'regtr_weighted_procrustes_bwd')
    return d_corr, d_logit, d_kp, d_weight


# ------------------------------------------------------------------------------------------------ losses (validation / test)
def infonce(anc, pos_t, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, r_p, r_n, anc_pose=None, rows=False):
    """InfoNCE feature loss of packed, ragged pairs (regtr_infonce).  anc (N_anc, D) and pos_t (N_pos, D) row-strided views (pos_t: the
    TRANSFORMED positives G W_sym), xyz (N, 3), seg_off (B+1,) int32 on the device, max_anc >= every pair's anchor count.
    anc_pose (B, 12) float32 or None: applied to anc_xyz first.  Returns pair_out (B, 2) = (masked loss sum, mask count); with rows=True
    also (row_loss, row_mask) (N_anc,).  Nothing here synchronises."""
    L = _lib.lib()
    n_anc, D = anc.shape
    n_pos = pos_t.shape[0]
    B = anc_seg_off.numel() - 1
    dev = anc.device
    out = torch.empty((B, 2), dtype=torch.float32, device=dev)
    rl = torch.empty(n_anc, dtype=torch.float32, device=dev) if rows else None
    rm = torch.empty(n_anc, dtype=torch.float32, device=dev) if rows else None
    nb = L.regtr_infonce_ws_bytes(B, int(max_anc))
    ws = _ws(max(nb, 1), dev)
    lda = anc.stride(0) if n_anc > 1 else D
    ldp = pos_t.stride(0) if n_pos > 1 else D
    assert anc.stride(1) == 1 and pos_t.stride(1) == 1
    check(L.regtr_infonce(raw(anc) if n_anc else None, lda, raw(pos_t) if n_pos else None, ldp, ptr(anc_xyz) if n_anc else None,
                          ptr(pos_xyz) if n_pos else None, iptr(anc_seg_off), iptr(pos_seg_off), B, n_anc, n_pos, int(max_anc), D,
                          float(r_p), float(r_n), ptr(anc_pose), ptr(out), ptr(rl), ptr(rm), bptr(ws), nb, stream()), 'regtr_infonce')
    return (out, rl, rm) if rows else out


def loss_terms(logit, gt_overlap, kp, warped, seg_off, pose):
    """The O(N) loss terms of one layer (regtr_loss_terms): logit / gt_overlap (N,), kp / warped (N, 3) packed like RegTR.forward's
    coarsest level (seg_off (2B+1,) int32: src clouds, then tgt clouds), pose (B, 3, 4) or (B, 4, 4) float32.  Returns (B, 5): BCE sum,
    src sum w|err|_1, src sum w, tgt sum w|err|_1, tgt sum w."""
    B = seg_off.numel() // 2
    N = logit.shape[0]
    pose = pose.contiguous()
    out = torch.empty((B, 5), dtype=torch.float32, device=logit.device)
    check(_lib.lib().regtr_loss_terms(ptr(logit) if N else None, ptr(gt_overlap) if N else None, ptr(kp) if N else None,
                                      ptr(warped) if N else None, iptr(seg_off), B, N, ptr(pose), pose.shape[-2] * pose.shape[-1],
                                      ptr(out), stream()), 'regtr_loss_terms')
    return out


def se3_transform(xyz, seg_off, pose):
    """xyz (N, 3) packed clouds (seg_off (C+1,) int32), pose (C, 3, 4) or (C, 4, 4) float32 -> (N, 3): cloud c's points x' = R_c x + t_c,
    rounded per operation (regtr_se3_transform)."""
    n = xyz.shape[0]
    pose = pose.contiguous()
    out = torch.empty((n, 3), dtype=torch.float32, device=xyz.device)
    check(_lib.lib().regtr_se3_transform(ptr(xyz) if n else None, iptr(seg_off), seg_off.numel() - 1, n, ptr(pose),
                                         pose.shape[-2] * pose.shape[-1], ptr(out) if n else None, stream()), 'regtr_se3_transform')
    return out


# ------------------------------------------------------------------------------------------------ training-loss backward
def infonce_rows(anc, pos_t, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, r_p, r_n, anc_pose=None):
    """ops.infonce with the decisions its backward reuses (regtr_infonce_rows): -> (pair_out (B, 2), row_lse (N_anc,), row_idx (N_anc,)
    int32, row_mask (N_anc,)).  pair_out is bit-identical to ops.infonce's.  Nothing here synchronises."""
    L = _lib.lib()
    n_anc, D = anc.shape
    n_pos = pos_t.shape[0]
    B = anc_seg_off.numel() - 1
    dev = anc.device
    out = torch.empty((B, 2), dtype=torch.float32, device=dev)
    lse = torch.empty(n_anc, dtype=torch.float32, device=dev)
    idx = torch.empty(n_anc, dtype=torch.int32, device=dev)
    rm = torch.empty(n_anc, dtype=torch.float32, device=dev)
    nb = L.regtr_infonce_ws_bytes(B, int(max_anc))
    ws = _ws(max(nb, 1), dev)
    lda = anc.stride(0) if n_anc > 1 else D
    ldp = pos_t.stride(0) if n_pos > 1 else D
    assert anc.stride(1) == 1 and pos_t.stride(1) == 1
    check(L.regtr_infonce_rows(raw(anc) if n_anc else None, lda, raw(pos_t) if n_pos else None, ldp, ptr(anc_xyz) if n_anc else None,
                               ptr(pos_xyz) if n_pos else None, iptr(anc_seg_off), iptr(pos_seg_off), B, n_anc, n_pos, int(max_anc), D,
                               float(r_p), float(r_n), ptr(anc_pose), ptr(out), None, ptr(rm) if n_anc else None,
                               ptr(lse) if n_anc else None, iptr(idx) if n_anc else None, bptr(ws), nb, stream()), 'regtr_infonce_rows')
    return out, lse, idx, rm


def infonce_bwd(anc, pos_t, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, max_pos, r_n, saved, grad, mean_div, anc_pose=None):
    """Backward of (1 / mean_div) sum_b pair_out[b,0] / pair_out[b,1] (regtr_infonce_bwd): saved = infonce_rows' result, grad a 0-dim
    float32 device tensor.  -> (d_anc (N_anc, D), d_pos_t (N_pos, D)), d_pos_t the gradient of the TRANSFORMED positives.  anc / pos_t
    contiguous.  Nothing here synchronises."""
    out, lse, idx, rm = saved
    n_anc, D = anc.shape
    n_pos = pos_t.shape[0]
    B = anc_seg_off.numel() - 1
    d_anc = torch.empty((n_anc, D), dtype=torch.float32, device=anc.device)
    d_pos = torch.empty((n_pos, D), dtype=torch.float32, device=anc.device)
    check(_lib.lib().regtr_infonce_bwd(ptr(anc) if n_anc else None, D, ptr(pos_t) if n_pos else None, D,
                                       ptr(anc_xyz) if n_anc else None, ptr(pos_xyz) if n_pos else None, iptr(anc_seg_off),
                                       iptr(pos_seg_off), B, n_anc, n_pos, int(max_anc), int(max_pos), D, float(r_n), ptr(anc_pose),
                                       ptr(lse) if n_anc else None, iptr(idx) if n_anc else None, ptr(rm) if n_anc else None, ptr(out),
                                       ptr(grad.reshape(1)), float(mean_div), ptr(d_anc) if n_anc else None, D,
                                       ptr(d_pos) if n_pos else None, D, stream()), 'regtr_infonce_bwd')
    return d_anc, d_pos


CIRCLE_DEFAULTS = dict(log_scale=10.0, pos_margin=0.1, pos_optimal=0.1, neg_margin=1.4, neg_optimal=1.4)     # feature_loss.py:168


def _circle_args(anc, pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, max_pos, r_p, r_n, params, anc_pose):
    """The leading arguments regtr_circle_rows and regtr_circle_bwd share."""
    n_anc, D = anc.shape
    n_pos = pos.shape[0]
    p = dict(CIRCLE_DEFAULTS, **(params or {}))
    lda = anc.stride(0) if n_anc > 1 else D
    ldp = pos.stride(0) if n_pos > 1 else D
    assert anc.stride(1) == 1 and pos.stride(1) == 1
    return (raw(anc) if n_anc else None, lda, raw(pos) if n_pos else None, ldp, ptr(anc_xyz) if n_anc else None,
            ptr(pos_xyz) if n_pos else None, iptr(anc_seg_off), iptr(pos_seg_off), anc_seg_off.numel() - 1, n_anc, n_pos, int(max_anc),
            int(max_pos), D, float(r_p), float(r_n), float(p['log_scale']), float(p['pos_margin']), float(p['pos_optimal']),
            float(p['neg_margin']), float(p['neg_optimal']), ptr(anc_pose))


def circle_rows(anc, pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, max_pos, r_p, r_n, params=None, anc_pose=None):
    """CircleLossFull ('euclidean') of packed, ragged pairs (regtr_circle_rows).  anc (N_anc, D) / pos (N_pos, D) row-strided views, xyz
    (N, 3), seg_off (B+1,) int32 on the device, max_anc / max_pos >= every pair's counts, params: overrides of CIRCLE_DEFAULTS, anc_pose
    (B, 12) float32 or None: applied to anc_xyz first.  -> (pair_out (B, 4) = (sum of selected row losses, their number, sum of selected
    column losses, their number), anc_lse (N_anc, 2), anc_sel (N_anc,), pos_lse (N_pos, 2), pos_sel (N_pos,)): what circle_bwd reuses.
    The pair loss is (out0 / out1 + out2 / out3) / 2.  Nothing here synchronises."""
    n_anc, n_pos, dev = anc.shape[0], pos.shape[0], anc.device
    B = anc_seg_off.numel() - 1
    out = torch.empty((B, 4), dtype=torch.float32, device=dev)
    a_lse = torch.empty((n_anc, 2), dtype=torch.float32, device=dev)
    a_sel = torch.empty(n_anc, dtype=torch.float32, device=dev)
    p_lse = torch.empty((n_pos, 2), dtype=torch.float32, device=dev)
    p_sel = torch.empty(n_pos, dtype=torch.float32, device=dev)
    head = _circle_args(anc, pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, max_pos, r_p, r_n, params, anc_pose)
    check(_lib.lib().regtr_circle_rows(*head, ptr(out), ptr(a_lse) if n_anc else None, ptr(a_sel) if n_anc else None,
                                       ptr(p_lse) if n_pos else None, ptr(p_sel) if n_pos else None, stream()), 'regtr_circle_rows')
    return out, a_lse, a_sel, p_lse, p_sel


def circle_bwd(anc, pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, max_pos, r_p, r_n, saved, grad, mean_div, params=None,
               anc_pose=None):
    """Backward of (1 / mean_div) sum_b (out0 / out1 + out2 / out3)_b / 2 (regtr_circle_bwd): saved = circle_rows' result, grad a 0-dim
    float32 device tensor -> (d_anc (N_anc, D), d_pos (N_pos, D)); a NaN pair's rows are zero.  Nothing here synchronises."""
    out, a_lse, a_sel, p_lse, p_sel = saved
    n_anc, D = anc.shape
    n_pos = pos.shape[0]
    d_anc = torch.empty((n_anc, D), dtype=torch.float32, device=anc.device)
    d_pos = torch.empty((n_pos, D), dtype=torch.float32, device=anc.device)
    head = _circle_args(anc, pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, max_anc, max_pos, r_p, r_n, params, anc_pose)
    check(_lib.lib().regtr_circle_bwd(*head, ptr(a_lse) if n_anc else None, ptr(a_sel) if n_anc else None, ptr(p_lse) if n_pos else None,
                                      ptr(p_sel) if n_pos else None, ptr(out), ptr(grad.reshape(1)), float(mean_div),
                                      ptr(d_anc) if n_anc else None, D, ptr(d_pos) if n_pos else None, D, stream()), 'regtr_circle_bwd')
    return d_anc, d_pos


def gemm_tn(a, b, fold=False):
    """a (M, N1)^T @ b (M, N2) -> (N1, N2) over a tall M (regtr_gemm_tn: split-K, fixed-order second pass, bit-reproducible); N1, N2
    multiples of 64.  fold=True (N1 == N2): InfoNCELossFull's dW from dW_sym = a^T b (upper triangle dW_sym + dW_sym^T, diagonal
    doubled, zero below).  a / b may be row-strided views with unit column stride (a column block of a wider buffer)."""
    L = _lib.lib()
    M, N1 = a.shape
    N2 = b.shape[1]
    out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
    nb = L.regtr_gemm_tn_ws_bytes(M, N1, N2)
    ws = _ws(max(nb, 1), a.device)
    (pa, lda), (pb, ldb) = _rows_ptr(a), _rows_ptr(b)
    check(L.regtr_gemm_tn(pa if M else None, lda, pb if M else None, ldb, M, N1, N2, int(bool(fold)), ptr(out), N2, bptr(ws), nb,
                          stream()), 'regtr_gemm_tn')
    return out


def _rows_ptr(t):
    """(device pointer, row stride) of a float32 (M, N) operand of the transposed GEMMs: a contiguous tensor goes through ptr()'s checks
    as before; a row-strided view with unit column stride (a column block of a wider buffer) through raw() with its own stride."""
    if t.is_contiguous():
        return ptr(t), t.shape[1]
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < t.shape[1]:
        raise RuntimeError(f'regtr_amd transposed GEMM: an operand must have unit column stride, got strides {tuple(t.stride())}')
    return raw(t), t.stride(0)


def corr_l1_bwd(kp, warped, w, seg_off, pose, grad, den):
    """Backward of CorrCriterion('mae') (regtr_corr_l1_bwd): kp / warped (N, 3), w (N,) packed by seg_off (B+1,) int32, pose (B, 3|4, 4),
    grad and den 0-dim float32 device tensors (den: the clamped weight sum) -> d warped (N, 3)."""
    n = kp.shape[0]
    pose = pose.contiguous()
    out = torch.empty((n, 3), dtype=torch.float32, device=kp.device)
    check(_lib.lib().regtr_corr_l1_bwd(ptr(kp) if n else None, ptr(warped) if n else None, ptr(w) if n else None, iptr(seg_off),
                                       seg_off.numel() - 1, n, ptr(pose), pose.shape[-2] * pose.shape[-1], ptr(grad.reshape(1)),
                                       ptr(den.reshape(1)), ptr(out) if n else None, stream()), 'regtr_corr_l1_bwd')
    return out


# ------------------------------------------------------------------------------------------------ KPConv backward
def kpconv_wf(q_xyz, s_xyz, nbr, x, kernel_points, extent):
    """The gather half of a plain kpconv() call (no x_stats, no xyzf) on its own: -> (wf (Nq, KP Cin), num (Nq,)), the very values that
    call contracts with the weights and divides by -- what KPConv's backward recomputes instead of keeping wf alive."""
    L = _lib.lib()
    nq, H = nbr.shape
    ns, Cin = x.shape
    KP = kernel_points.shape[0]
    flag = None
    if not (L.regtr_kpconv_gather_computes_flag(Cin, H) and x.data_ptr() % 16 == 0 and ns > 0 and ns * Cin < (1 << 29)):
        flag = torch.empty(ns, dtype=torch.float32, device=x.device)
        check(L.regtr_rowsum_positive(ptr(x), ns, Cin, None, None, 0, 0.1, ptr(flag), stream()), 'regtr_rowsum_positive')
    wf = torch.empty((nq, KP * Cin), dtype=torch.float32, device=x.device)
    num = torch.empty(nq, dtype=torch.float32, device=x.device)
    check(L.regtr_kpconv_gather(ptr(q_xyz), nq, ptr(s_xyz), ns, iptr(nbr), H, ptr(x), Cin, ptr(flag), None, ptr(kernel_points), KP,
                                float(extent), None, None, 0, 0.1, ptr(wf), 0, ptr(num), stream()), 'regtr_kpconv_gather')
    return wf, num


def nbr_transpose(nbr, ns):
    """The neighbour table by support (regtr_nbr_transpose): nbr (Nq, H) int32, entries outside [0, ns) shadows -> (row_off (ns + 1,),
    entries (Nq H,)) int32: support s's incoming entries q H + h are entries[row_off[s]:row_off[s + 1]], ascending; entries past
    row_off[ns] are not written.  A pure function of nbr.  Nothing here synchronises."""
    L = _lib.lib()
    nq, H = nbr.shape
    ns = int(ns)
    row_off = torch.empty(ns + 1, dtype=torch.int32, device=nbr.device)
    entries = torch.empty(max(nq * H, 1), dtype=torch.int32, device=nbr.device)
    nb = L.regtr_nbr_transpose_ws_bytes(nq, H, ns)
    ws = _ws(max(nb, 1), nbr.device)
    check(L.regtr_nbr_transpose(iptr(nbr) if nq else None, nq, H, ns, iptr(row_off), iptr(entries), bptr(ws), nb, stream()),
          'regtr_nbr_transpose')
    return row_off, entries


def kpconv_gather_bwd(dwf, q_xyz, s_xyz, H, kernel_points, extent, transposed, out=None):
    """Backward of the KPConv gather with respect to the features (regtr_kpconv_gather_bwd): dwf (Nq, KP Cin) the gradient of the
    weighted-feature rows, transposed = nbr_transpose(nbr, Ns) of the (Nq, H) table the forward gathered through -> dx (Ns, Cin).
    out: the dx buffer, or None for a new one.  Bit-reproducible.  Nothing here synchronises."""
    nq, ns, KP = q_xyz.shape[0], s_xyz.shape[0], kernel_points.shape[0]
    if dwf.shape[0] != nq or dwf.shape[1] % KP:
        raise RuntimeError(f'kpconv_gather_bwd: dwf must be ({nq}, {KP} Cin), got {tuple(dwf.shape)}')
    Cin = dwf.shape[1] // KP
    row_off, entries = transposed
    if row_off.numel() != ns + 1 or entries.numel() < nq * H:
        raise RuntimeError(f'kpconv_gather_bwd: the transposed table is not one of a ({nq}, {H}) table over {ns} supports')
    dx = torch.empty((ns, Cin), dtype=torch.float32, device=dwf.device) if out is None else out
    if out is not None and tuple(out.shape) != (ns, Cin):
        raise RuntimeError(f'kpconv_gather_bwd: out must be ({ns}, {Cin}), got {tuple(out.shape)}')
    check(_lib.lib().regtr_kpconv_gather_bwd(ptr(dwf) if nq else None, ptr(q_xyz) if nq else None, nq, ptr(s_xyz), ns, int(H), Cin,
                                             ptr(kernel_points), KP, float(extent), iptr(row_off), iptr(entries), ptr(dx), stream()),
          'regtr_kpconv_gather_bwd')
    return dx


def instnorm_bwd(x, seg_off, max_len, stats, dy, residual=None, res_stats=None, lrelu=False, slope=0.1, want_dx=True, want_dres=False,
                 out_dx=None, out_dres=None):
    """Backward of instnorm_apply(x, seg_off, max_len, instnorm_stats(x), residual, res_stats [= instnorm_stats(residual)], lrelu, slope)
    (regtr_instnorm_bwd): the forward's own arguments plus dy (N, C), the gradient of its output -> (dx, dres), None where not wanted.
    out_dx / out_dres: the buffers to write, or None for new ones.  Bit-reproducible.  Nothing here synchronises."""
    L = _lib.lib()
    n_clouds = seg_off.numel() - 1
    N, C = x.shape
    if tuple(dy.shape) != (N, C) or (residual is not None and tuple(residual.shape) != (N, C)):
        raise RuntimeError(f'instnorm_bwd: dy and residual must be ({N}, {C}) like x')
    if want_dres and residual is None:
        raise RuntimeError('instnorm_bwd: want_dres needs the residual the forward took')
    dx = dres = None
    if want_dx:
        dx = torch.empty_like(x) if out_dx is None else out_dx
    if want_dres:
        dres = torch.empty_like(x) if out_dres is None else out_dres
    for o in (dx, dres):
        if o is not None and tuple(o.shape) != (N, C):
            raise RuntimeError(f'instnorm_bwd: an output buffer must be ({N}, {C}), got {tuple(o.shape)}')
    nb = L.regtr_instnorm_bwd_ws_bytes(n_clouds, int(max_len), C)
    ws = _ws(max(nb, 1), x.device)
    check(L.regtr_instnorm_bwd(ptr(x), iptr(seg_off), n_clouds, int(max_len), C, ptr(stats), ptr(residual), ptr(res_stats),
                               1 if lrelu else 0, slope, ptr(dy), ptr(dx), ptr(dres), bptr(ws), nb, stream()), 'regtr_instnorm_bwd')
    return dx, dres


def maxpool_argmax(x, nbr, width=None, out=None):
    """The column of nbr (of the first `width`) each maximum of maxpool(x, nbr, width) came from (regtr_maxpool_argmax): (Nq, C) int16, the
    lowest column on equal values, -1 where the zero shadow row won.  out: the buffer to write, or None for a new one."""
    ns, C = x.shape
    nq, ld = nbr.shape
    arg = torch.empty((nq, C), dtype=torch.int16, device=x.device) if out is None else out
    if tuple(arg.shape) != (nq, C):
        raise RuntimeError(f'maxpool_argmax: out must be ({nq}, {C}), got {tuple(arg.shape)}')
    check(_lib.lib().regtr_maxpool_argmax(ptr(x) if ns else None, ns, C, iptr(nbr) if nq else None, ld, nq, ld if width is None else int(width),
                                          ptr(arg, torch.int16) if nq else None, stream()), 'regtr_maxpool_argmax')
    return arg


def maxpool_fwd_argmax(x, nbr, width=None, out=None, out_arg=None):
    """maxpool(x, nbr, width) and maxpool_argmax(x, nbr, width) from ONE pass over the rows (regtr_maxpool_fwd_argmax) -> (out (Nq, C)
    float32, arg (Nq, C) int16), each bit-equal to the separate launch's.  out / out_arg: the buffers to write, or None for new ones."""
    ns, C = x.shape
    nq, ld = nbr.shape
    res = torch.empty((nq, C), dtype=torch.float32, device=x.device) if out is None else out
    arg = torch.empty((nq, C), dtype=torch.int16, device=x.device) if out_arg is None else out_arg
    if tuple(res.shape) != (nq, C) or tuple(arg.shape) != (nq, C):
        raise RuntimeError(f'maxpool_fwd_argmax: out and out_arg must be ({nq}, {C}), got {tuple(res.shape)}, {tuple(arg.shape)}')
    check(_lib.lib().regtr_maxpool_fwd_argmax(ptr(x) if ns else None, ns, C, iptr(nbr) if nq else None, ld, nq, ld if width is None else int(width),
                                              ptr(res) if nq else None, ptr(arg, torch.int16) if nq else None, stream()),
          'regtr_maxpool_fwd_argmax')
    return res, arg


def maxpool_bwd(dy, arg, H, transposed, out=None):
    """Backward of maxpool (regtr_maxpool_gather_bwd): dy (Nq, C) the gradient of the pooled rows, arg = maxpool_argmax(...) of the same
    call, transposed = nbr_transpose(the (Nq, H) table the forward pooled through, Ns) -> dx (Ns, C).  out: the dx buffer, or None for a
    new one.  A float32 sum in ascending entry order per element: bit-reproducible.  Nothing here synchronises."""
    nq, C = dy.shape
    row_off, entries = transposed
    ns = row_off.numel() - 1
    if tuple(arg.shape) != (nq, C) or entries.numel() < nq * H:
        raise RuntimeError(f'maxpool_bwd: arg must be ({nq}, {C}) and the transposed table one of a ({nq}, {H}) table')
    dx = torch.empty((ns, C), dtype=torch.float32, device=dy.device) if out is None else out
    if tuple(dx.shape) != (ns, C):
        raise RuntimeError(f'maxpool_bwd: out must be ({ns}, {C}), got {tuple(dx.shape)}')
    check(_lib.lib().regtr_maxpool_gather_bwd(ptr(dy) if nq else None, ptr(arg, torch.int16) if nq else None, nq, int(H), C, iptr(row_off),
                                              iptr(entries) if nq else None, ns, ptr(dx) if ns else None, stream()), 'regtr_maxpool_gather_bwd')
    return dx


def row_div(x, div):
    """x (n, N) / div (n,)[:, None] (regtr_row_div): KPConv's backward through its neighbour-count normaliser."""
    n, N = x.shape
    out = torch.empty((n, N), dtype=torch.float32, device=x.device)
    check(_lib.lib().regtr_row_div(ptr(x), N, ptr(div), n, N, ptr(out), N, stream()), 'regtr_row_div')
    return out


def gemm_tn_any(a, b):
    """gemm_tn (no fold) for any widths (regtr_gemm_tn_any): a (M, N1)^T @ b (M, N2) -> (N1, N2), bit-reproducible."""
    L = _lib.lib()
    M, N1 = a.shape
    N2 = b.shape[1]
    out = torch.empty((N1, N2), dtype=torch.float32, device=a.device)
    nb = L.regtr_gemm_tn_any_ws_bytes(M, N1, N2)
    ws = _ws(max(nb, 1), a.device)
    (pa, lda), (pb, ldb) = _rows_ptr(a), _rows_ptr(b)
    check(L.regtr_gemm_tn_any(pa if M else None, lda, pb if M else None, ldb, M, N1, N2, ptr(out), N2, bptr(ws), nb, stream()),
          'regtr_gemm_tn_any')
    return out



# ------------------------------------------------------------------------------------------------ correspondence head / overlap loss backward
def head_tail_bwd(dcorr, dlogit, h2, f, w4, wc, out_g2=None, out_r=None):
    """Backward of CorrespondenceRegressor's narrow outputs corr = h2 w4^T + b4 and logit = f wc^T + bc in one pass (regtr_head_tail_bwd):
    dcorr (M, 3) | None, dlogit (M,) | None, h2 (M, D) the activation stored after coor_mlp[2]'s ReLU, f (M, D) the head's input, w4
    (3, D), wc (D,) or (1, D) -> (g2 (M, D) = (dcorr w4) where h2 > 0 else 0, r (M, D) = dlogit wc, dw4 (3, D), db4 (3,), dwc (D,), dbc
    (1,), db2 (D,) = the column sums of g2).  An absent gradient's outputs are zeros.  out_g2 / out_r: the buffers to write, or None
    for new ones.  D a multiple of 64.  Bit-reproducible.  Nothing here synchronises."""
    L = _lib.lib()
    M, D = h2.shape
    wc = wc.reshape(-1)
    if tuple(f.shape) != (M, D) or tuple(w4.shape) != (3, D) or wc.numel() != D:
        raise RuntimeError(f'head_tail_bwd: f must be ({M}, {D}), w4 (3, {D}) and wc ({D},), got {tuple(f.shape)}, {tuple(w4.shape)}, {tuple(wc.shape)}')
    if dcorr is not None and tuple(dcorr.shape) != (M, 3):
        raise RuntimeError(f'head_tail_bwd: dcorr must be ({M}, 3), got {tuple(dcorr.shape)}')
    if dlogit is not None and dlogit.numel() != M:
        raise RuntimeError(f'head_tail_bwd: dlogit must have {M} elements, got {tuple(dlogit.shape)}')
    g2 = torch.empty((M, D), dtype=torch.float32, device=h2.device) if out_g2 is None else out_g2
    r = torch.empty((M, D), dtype=torch.float32, device=h2.device) if out_r is None else out_r
    for o in (g2, r):
        if tuple(o.shape) != (M, D):
            raise RuntimeError(f'head_tail_bwd: an output buffer must be ({M}, {D}), got {tuple(o.shape)}')
    sums = torch.zeros(5 * D + 4, dtype=torch.float32, device=h2.device)        # M = 0: nothing is launched and the sums are 0
    nb = L.regtr_head_tail_bwd_ws_bytes(M, D)
    ws = _ws(max(nb, 1), h2.device)
    base = ptr(sums)
    check(L.regtr_head_tail_bwd(ptr(dcorr), ptr(dlogit), ptr(h2), ptr(f), ptr(w4), ptr(wc), M, D, ptr(g2), ptr(r), base, base + 16 * D,
                                base + 12 * D, base + 16 * D + 12, base + 16 * D + 16, bptr(ws), nb, stream()), 'regtr_head_tail_bwd')
    return (g2, r, sums[:3 * D].view(3, D), sums[4 * D:4 * D + 3], sums[3 * D:4 * D], sums[4 * D + 3:4 * D + 4], sums[4 * D + 4:])


def bce_logits_bwd(logit, gt, grad):
    """Backward of nn.BCEWithLogitsLoss() (mean) on packed points (regtr_bce_logits_bwd): logit, gt (n,), grad a 0-dim float32 device
    tensor -> d logit (n,) = grad (sigmoid(logit) - gt) / n."""
    n = logit.numel()
    if gt.numel() != n:
        raise RuntimeError(f'bce_logits_bwd: logit and gt must have the same number of elements, got {n} and {gt.numel()}')
    out = torch.empty(logit.shape, dtype=torch.float32, device=logit.device)
    check(_lib.lib().regtr_bce_logits_bwd(ptr(logit) if n else None, ptr(gt) if n else None, ptr(grad.reshape(1)), n,
                                          ptr(out) if n else None, stream()), 'regtr_bce_logits_bwd')
    return out


# ------------------------------------------------------------------------------------------------ training augmentation (csrc/augment.hip)
PERTURB_MODES = {'none': 0, 'small': 1, 'large': 2}
_U64 = (1 << 64) - 1


def cloud_centroids(xyz, seg_off):
    """xyz (N, 3) packed clouds (seg_off (C+1,) int32) -> (C, 3): per-cloud means, float64 sums in a fixed order (regtr_cloud_centroids)."""
    n, C = xyz.shape[0], seg_off.numel() - 1
    out = torch.empty((C, 3), dtype=torch.float32, device=xyz.device)
    check(_lib.lib().regtr_cloud_centroids(ptr(xyz) if n else None, iptr(seg_off), C, n, ptr(out), stream()), 'regtr_cloud_centroids')
    return out


def augment_draws(pose, centroids, seed, step, perturb_mode='small', perturb_std=0.1, swap=True):
    """The per-pair decisions of RigidPerturb / RandomSwap (regtr_augment_draws): pose (B, 3, 4) or (B, 4, 4), centroids (2B, 3) of the
    input clouds (src slots, then tgt slots; read in mode 'small' only) -> (xform (2B, 3, 4), pose_out (B, 3, 4), flags (B, 2) int32:
    perturb_source, swap)."""
    B = pose.shape[0]
    pose = pose.contiguous()
    dev = pose.device
    xform = torch.empty((2 * B, 3, 4), dtype=torch.float32, device=dev)
    pose_out = torch.empty((B, 3, 4), dtype=torch.float32, device=dev)
    flags = torch.empty((B, 2), dtype=torch.int32, device=dev)
    check(_lib.lib().regtr_augment_draws(ptr(pose), pose.shape[-2] * pose.shape[-1], ptr(centroids), B, int(seed) & _U64,
                                         int(step) & 0xffffffff, PERTURB_MODES[perturb_mode], float(perturb_std), int(bool(swap)),
                                         ptr(xform), ptr(pose_out), iptr(flags), stream()), 'regtr_augment_draws')
    return xform, pose_out, flags


def shuffle_keys(seg_off, n, seed, step):
    """One int64 sort key per row of packed clouds, (cloud_slot << 32) | philox word (regtr_shuffle_keys); torch.sort(stable=True) of it
    is the shuffle."""
    keys = torch.empty(n, dtype=torch.int64, device=seg_off.device)
    check(_lib.lib().regtr_shuffle_keys(iptr(seg_off), seg_off.numel() - 1, n, int(seed) & _U64, int(step) & 0xffffffff,
                                        ptr(keys, torch.int64) if n else None, stream()), 'regtr_shuffle_keys')
    return keys


def augment_gather(xyz, mask, in_off, perm, out_off, in_slot, n_out, xform, noise, seed, step):
    """The one pass over the points (regtr_augment_gather): xyz (N, 3), mask (N,) uint8 or None, in_off / out_off (C+1,) int32, perm (N,)
    int64 or None, in_slot (C,) int32, xform (C, 3, 4) or None -> (out_xyz (n_out, 3), out_mask (n_out,) uint8 or None)."""
    n_in, C = xyz.shape[0], in_off.numel() - 1
    out = torch.empty((n_out, 3), dtype=torch.float32, device=xyz.device)
    out_mask = None if mask is None else torch.empty(n_out, dtype=torch.uint8, device=xyz.device)
    check(_lib.lib().regtr_augment_gather(ptr(xyz) if n_in else None, bptr(mask), iptr(in_off), n_in, ptr(perm, torch.int64),
                                          iptr(out_off), iptr(in_slot), C, int(n_out), ptr(xform), float(noise), int(seed) & _U64,
                                          int(step) & 0xffffffff, ptr(out) if n_out else None, bptr(out_mask) if n_out else None,
                                          stream()), 'regtr_augment_gather')
    return out, out_mask


# ------------------------------------------------------------------------------------------------ ModelNet training augmentation (csrc/augment_modelnet.hip)
def modelnet_draws(n_clouds, seed, step, rot_mag, trans_mag, device):
    """The per-cloud decisions of RandomCrop's directions and RandomTransformSE3_euler (regtr_modelnet_draws) -> (dirs (2B, 3): the crop
    direction of every slot (source slots, then reference slots), xform (B, 3, 4), pose (B, 3, 4) = xform^-1)."""
    dirs = torch.empty((2 * n_clouds, 3), dtype=torch.float32, device=device)
    xform = torch.empty((n_clouds, 3, 4), dtype=torch.float32, device=device)
    pose = torch.empty((n_clouds, 3, 4), dtype=torch.float32, device=device)
    check(_lib.lib().regtr_modelnet_draws(n_clouds, int(seed) & _U64, int(step) & 0xffffffff, float(rot_mag), float(trans_mag), ptr(dirs),
                                          ptr(xform), ptr(pose), stream()), 'regtr_modelnet_draws')
    return dirs, xform, pose


def crop_select_lds_points():
    """The largest cloud whose distance keys regtr_crop_select keeps in LDS; a larger one re-reads global memory per digit pass."""
    return int(_lib.lib().regtr_crop_select_lds_points())


def crop_select(xyz, raw_off, max_len, dirs, sel_lo, sel_t, slot_off, n_slot_rows):
    """RandomCrop.crop of every slot (regtr_crop_select): xyz (N, 3) packed raw clouds (raw_off (B+1,) int32), dirs (2B, 3), sel_lo (2B,)
    int32 / sel_t (2B,) float64 the percentile's lower rank and interpolation weight, slot_off (2B+1,) int32 -> (centroid (2B, 3),
    thr (2B,) float64, count (2B,) int32, flag (2B,) int32, keep (n_slot_rows,) uint8)."""
    B = raw_off.numel() - 1
    dev = xyz.device
    centroid = torch.empty((2 * B, 3), dtype=torch.float32, device=dev)
    thr = torch.empty(2 * B, dtype=torch.float64, device=dev)
    count = torch.empty(2 * B, dtype=torch.int32, device=dev)
    flag = torch.empty(2 * B, dtype=torch.int32, device=dev)
    keep = torch.empty(n_slot_rows, dtype=torch.uint8, device=dev)
    check(_lib.lib().regtr_crop_select(ptr(xyz), iptr(raw_off), xyz.shape[0], B, int(max_len), ptr(dirs), iptr(sel_lo), _lib.dptr(sel_t),
                                       iptr(slot_off), int(n_slot_rows), ptr(centroid), _lib.dptr(thr), iptr(count), iptr(flag),
                                       bptr(keep), stream()), 'regtr_crop_select')
    return centroid, thr, count, flag, keep


def modelnet_keys(slot_off, n_slot_rows, k_out, keep, seed, step):
    """The resample keys of every slot's raw rows and the shuffle keys of its k_out output rows in one int64 array
    (regtr_modelnet_keys); torch.sort(stable=True) of it is both orders."""
    n_slots = slot_off.numel() - 1
    keys = torch.empty(n_slot_rows + n_slots * k_out, dtype=torch.int64, device=slot_off.device)
    check(_lib.lib().regtr_modelnet_keys(iptr(slot_off), n_slots, int(n_slot_rows), int(k_out), bptr(keep), int(seed) & _U64,
                                         int(step) & 0xffffffff, ptr(keys, torch.int64), stream()), 'regtr_modelnet_keys')
    return keys


def modelnet_gather(xyz, raw_off, slot_off, n_slot_rows, k_out, perm, count, keep, xform, scale, clip, seed, step):
    """The one pass over the output rows (regtr_modelnet_gather) -> (out_xyz (2B k_out, 3), out_mask (2B k_out,) uint8, out_row
    (2B k_out,) int32: the raw row every output row came from)."""
    B = raw_off.numel() - 1
    n_out = 2 * B * k_out
    out = torch.empty((n_out, 3), dtype=torch.float32, device=xyz.device)
    out_mask = torch.empty(n_out, dtype=torch.uint8, device=xyz.device)
    out_row = torch.empty(n_out, dtype=torch.int32, device=xyz.device)
    check(_lib.lib().regtr_modelnet_gather(ptr(xyz), iptr(raw_off), xyz.shape[0], B, iptr(slot_off), int(n_slot_rows), int(k_out),
                                           ptr(perm, torch.int64), iptr(count), bptr(keep), ptr(xform), float(scale), float(clip),
                                           int(seed) & _U64, int(step) & 0xffffffff, ptr(out), bptr(out_mask), iptr(out_row), stream()),
          'regtr_modelnet_gather')
    return out, out_mask, out_row


# ------------------------------------------------------------------------------------------------ validation / test metrics (csrc/metrics.hip)
NEAREST_QUERY_TILE = 768      # queries per workgroup of regtr_nearest (NR_QTILE in csrc/metrics.hip; tests straddle it)


def nearest_lds_points():
    """Supports per LDS tile of regtr_nearest; a longer support cloud is scanned in several tiles."""
    return int(_lib.lib().regtr_nearest_lds_points())


def _host_offsets(off, n, what):
    """Exclusive offsets given on the HOST (a sequence, numpy array or CPU tensor: the lengths of packed clouds are known there) as a list
    of ints, checked: they start at 0, never decrease and end at n."""
    if isinstance(off, torch.Tensor):
        if off.device.type != 'cpu':
            raise RuntimeError(f'{what}: offsets are host data (a sequence or a CPU tensor), got a tensor on {off.device}')
        off = off.tolist()
    off = [int(o) for o in off]
    if len(off) < 1 or off[0] != 0 or off[-1] != n or any(b < a for a, b in zip(off, off[1:])):
        raise RuntimeError(f'{what}: offsets must run from 0 to {n} without decreasing, got {off[:4]} ... {off[-1:]} ({len(off)} entries)')
    return off


def _check_cloud(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise RuntimeError(f'{what} must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    if t.dtype is not torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f'{what} must be a float32 (n, 3) cloud, got {t.dtype} {tuple(t.shape)}')
    return t.contiguous()


def _pose12(pose, C, what):
    """(C, 3, 4) / (C, 4, 4) / (C, 12) float32 device poses -> contiguous (C, 12), or None."""
    if pose is None:
        return None
    if pose.device.type != 'cuda' or pose.dtype is not torch.float32:
        raise RuntimeError(f'{what} must be a float32 GPU tensor, got {pose.dtype} on {pose.device}')
    if pose.dim() == 3 and pose.shape[1:] in ((3, 4), (4, 4)):
        pose = pose[:, :3, :].reshape(pose.shape[0], 12)
    if pose.dim() != 2 or tuple(pose.shape) != (C, 12):
        raise RuntimeError(f'{what} must hold one 3x4 transform per cloud ({C}), got {tuple(pose.shape)}')
    return pose.contiguous()


def nearest(q_xyz, q_off, s_xyz, s_off, q_pose=None, s_pose=None, return_idx=True, return_offsets=False):
    """For every query point the nearest point of the support cloud of the same index (regtr_nearest): q_xyz (Nq, 3), s_xyz (Ns, 3) packed
    ragged clouds, q_off / s_off their (C+1) exclusive offsets on the HOST, q_pose / s_pose optional (C, 3, 4) transforms applied first
    -> (d2 (Nq,) float32, idx (Nq,) int32 within the support cloud, or None).  Float32 rounded per operation, lowest index on ties, NaN
    never chosen.  return_offsets: also the (2, C+1) int32 device tensor of q_off and s_off this call uploaded (one copy for both), for
    the caller's next launch over the same clouds.  Refused: CPU tensors, clouds that are not float32 (n, 3), offset vectors of different lengths, an empty support cloud."""
    q_xyz, s_xyz = _check_cloud(q_xyz, 'nearest: q_xyz'), _check_cloud(s_xyz, 'nearest: s_xyz')
    nq, ns = q_xyz.shape[0], s_xyz.shape[0]
    qo, so = _host_offsets(q_off, nq, 'nearest: q_off'), _host_offsets(s_off, ns, 'nearest: s_off')
    if len(qo) != len(so):
        raise RuntimeError(f'nearest: q_off and s_off must describe the same number of clouds, got {len(qo) - 1} and {len(so) - 1}')
    C = len(qo) - 1
    empty = [c for c in range(C) if so[c + 1] == so[c]]
    if empty:
        raise RuntimeError(f'nearest: support cloud(s) {empty[:4]} are empty; a query has no nearest point in an empty cloud')
    dev = q_xyz.device
    q_pose, s_pose = _pose12(q_pose, C, 'nearest: q_pose'), _pose12(s_pose, C, 'nearest: s_pose')
    offs = torch.tensor([qo, so], dtype=torch.int32).to(dev, non_blocking=True)
    d2 = torch.empty(nq, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, dtype=torch.int32, device=dev) if return_idx else None
    max_q = max((b - a for a, b in zip(qo, qo[1:])), default=0)
    check(_lib.lib().regtr_nearest(ptr(q_xyz) if nq else None, iptr(offs[0]), nq, ptr(s_xyz) if ns else None, iptr(offs[1]), ns, C, max_q,
                                   ptr(q_pose), ptr(s_pose), ptr(d2) if nq else None, iptr(idx) if nq else None, stream()), 'regtr_nearest')
    return (d2, idx, offs) if return_offsets else (d2, idx)


def segment_mean(v, off):
    """v (N,) float32, off (C+1,) int32 device offsets -> (C,) float64 per-segment means, float64 sums in a fixed order
    (regtr_segment_mean); an empty segment gives 0."""
    n, C = v.numel(), off.numel() - 1
    out = torch.empty(max(C, 0), dtype=torch.float64, device=v.device)
    check(_lib.lib().regtr_segment_mean(ptr(v) if n else None, iptr(off), C, n, _lib.dptr(out) if C > 0 else None, stream()),
          'regtr_segment_mean')
    return out


def pose_metrics(pred, gt):
    """pred (L, B, 3, 4) or (B, 3, 4) float32, gt (B, 3, 4) or (B, 4, 4) float32 -> (out (L, B, 8) float64: rot_err_deg, trans_err (of
    pred o gt^-1, the reference's se3_compare), err_r_deg, err_t (of gt^-1 o pred), t_mse, t_mae, r_mse, r_mae; composed (L, B, 3, 4)
    float32 = pred o gt^-1) (regtr_pose_metrics).  With a (B, 3, 4) pred the results lose the leading dimension."""
    layered = pred.dim() == 4
    p = pred if layered else pred[None]
    if p.dim() != 4 or tuple(p.shape[2:]) != (3, 4) or gt.dim() != 3 or tuple(gt.shape[1:]) not in ((3, 4), (4, 4)) or gt.shape[0] != p.shape[1]:
        raise RuntimeError(f'pose_metrics: pred must be ([L,] B, 3, 4) and gt (B, 3, 4) or (B, 4, 4), got {tuple(pred.shape)} and {tuple(gt.shape)}')
    L, B = p.shape[0], p.shape[1]
    p, gt = p.contiguous(), gt.contiguous()
    out = torch.empty((L, B, 8), dtype=torch.float64, device=p.device)
    comp = torch.empty((L, B, 3, 4), dtype=torch.float32, device=p.device)
    n = L * B
    check(_lib.lib().regtr_pose_metrics(ptr(p) if n else None, ptr(gt) if n else None, gt.shape[1] * gt.shape[2], L, B,
                                        _lib.dptr(out) if n else None, ptr(comp) if n else None, stream()), 'regtr_pose_metrics')
    return (out, comp) if layered else (out[0], comp[0])


# ------------------------------------------------------------------------------------------------ optimiser step (csrc/optim.hip over csrc/multi_tensor.h)
_T = torch.Tensor
_dtype_of = operator.attrgetter('dtype')


@functools.lru_cache(maxsize=None)
def _table_dtype(name):
    """numpy's layout of one row of a host table (include/regtr_hip.h): 'optim' regtr_optim_tensor_t, 'guarded'
    regtr_optim_guarded_tensor_t, 'bucket' regtr_bucket_tensor_t -- built on first use (numpy is imported lazily)."""
    import numpy as np
    pgmvn = [(k, np.uint64) for k in 'pgmv'] + [('n', np.int64)]
    fields, size = {'optim': (pgmvn + [('scalars', np.float64, (7,))], 96),
                    'guarded': (pgmvn + [('hyper', np.float64, (5,)), ('step_index', np.int32)], 88),
                    'bucket': ([('g', np.uint64), ('n', np.int64), ('offset', np.int64)], 24)}[name]
    dtype = np.dtype(fields, align=True)
    assert dtype.itemsize == size
    return dtype


def _optim_all_ok(lists):
    """True when every tensor of every list is a float32 tensor on the launch device (C-level passes: this runs over ~600 tensors on
    every optimiser step); False sends the caller to the per-tensor checks, which say what is wrong."""
    try:
        dev = context.current().device_index
        dev = dev if dev is not None else torch.cuda.current_device()
        for lst in lists:
            if set(map(_T.get_device, lst)) != {dev} or set(map(_dtype_of, lst)) != {torch.float32}:
                return False
    except (RuntimeError, TypeError, AttributeError, AssertionError):
        return False
    return True


def _optim_table(grads, params=None, exp_avgs=None, exp_avg_sqs=None, scalars=None, what='optim'):
    """The host array of regtr_optim_tensor_t the multi-tensor entry points read (include/regtr_hip.h), built afresh on every call, and
    the list of gradient tensors it points at (kept alive by the caller until the launches are enqueued).  Every tensor is checked HERE,
    with a Python exception: a GPU tensor on the launch device, float32; p, m, v contiguous; g of p's shape, m and v of p's element count
    (a non-contiguous g is made contiguous)."""
    import numpy as np
    n = len(grads)
    state = params is not None
    if state and not (len(params) == len(exp_avgs) == len(exp_avg_sqs) == len(scalars) == n):
        raise RuntimeError(f'{what}: params, grads, exp_avgs, exp_avg_sqs and scalars must have one entry per tensor')
    ok = n > 0 and _optim_all_ok((grads, params, exp_avgs, exp_avg_sqs) if state else (grads,))
    if ok and state:
        ns = list(map(_T.numel, grads))
        ok = (all(map(_T.is_contiguous, params)) and all(map(_T.is_contiguous, exp_avgs)) and all(map(_T.is_contiguous, exp_avg_sqs))
              and list(map(_T.numel, exp_avgs)) == ns == list(map(_T.numel, exp_avg_sqs)) and list(map(_T.size, grads)) == list(map(_T.size, params)))
    if not ok:
        _optim_explain(grads, params, exp_avgs, exp_avg_sqs, what)
    keep = grads if all(map(_T.is_contiguous, grads)) else [g if g.is_contiguous() else g.contiguous() for g in grads]
    tab = np.zeros(n, dtype=_table_dtype('optim'))
    tab['g'] = list(map(_T.data_ptr, keep))
    tab['n'] = list(map(_T.numel, keep))
    if state:
        tab['p'] = list(map(_T.data_ptr, params))
        tab['m'] = list(map(_T.data_ptr, exp_avgs))
        tab['v'] = list(map(_T.data_ptr, exp_avg_sqs))
        if n:
            tab['scalars'] = np.asarray(scalars, dtype=np.float64).reshape(n, 7)
    return tab, keep


def _optim_explain(grads, params, exp_avgs, exp_avg_sqs, what):
    """The per-tensor checks, with the reason: raises, or returns when every tensor is acceptable after all."""
    dev = context.current().device_index

    def checked(t, name, i, contiguous):
        nonlocal dev
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f'{what}: {name}[{i}] must be a GPU tensor (got {getattr(t, "device", type(t))}); there is no CPU fallback')
        if dev is None:
            dev = torch.cuda.current_device()
        if t.dtype is not torch.float32:
            raise RuntimeError(f'{what}: {name}[{i}] must be float32, got {t.dtype} (the kernels reinterpret nothing)')
        if t.get_device() != dev:
            raise RuntimeError(f'{what}: {name}[{i}] is on {t.device} but the launch device is cuda:{dev}; wrap the call in '
                               'regtr_amd._lib.on_device(tensor.device)')
        if contiguous and not t.is_contiguous():
            raise RuntimeError(f'{what}: {name}[{i}] must be contiguous (the kernel writes it in place)')
        return t

    for i in range(len(grads)):
        g = checked(grads[i], 'grads', i, False)
        if params is not None:
            p = checked(params[i], 'params', i, True)
            m, v = checked(exp_avgs[i], 'exp_avgs', i, True), checked(exp_avg_sqs[i], 'exp_avg_sqs', i, True)
            if g.shape != p.shape or m.numel() != p.numel() or v.numel() != p.numel():
                raise RuntimeError(f'{what}: tensor {i}: the gradient {tuple(g.shape)} must have the parameter\'s shape {tuple(p.shape)} and the '
                                   f'moments {tuple(m.shape)}, {tuple(v.shape)} its element count')


def optim_slices():
    """(elements per float64 partial of grad_sumsq, elements per workgroup of adam_step, tensors per launch) -- tests straddle them."""
    L = _lib.lib()
    return int(L.regtr_optim_norm_slice()), int(L.regtr_optim_step_slice()), int(L.regtr_optim_chunk_tensors())


@functools.lru_cache(maxsize=None)
def _optim_norm_slice():
    return int(_lib.lib().regtr_optim_norm_slice())


def _sumsq(tab, keep):
    sl = _optim_norm_slice()
    n_part = int(((tab['n'] + (sl - 1)) // sl).sum())
    dev = keep[0].device if keep else torch.device('cuda', torch.cuda.current_device())
    partials = _ws_as(n_part, torch.float64, dev)
    check(_lib.lib().regtr_grad_sumsq(tab.ctypes.data if len(keep) else None, len(keep), dptr(partials) if n_part else None, n_part, stream()),
          'regtr_grad_sumsq')
    return partials


def grad_sumsq(grads):
    """First half of the global gradient norm (regtr_grad_sumsq): grads, a list of float32 GPU tensors -> (P,) float64 partial sums of
    squares, one per norm slice of every tensor in list order -- a function of the tensors' lengths alone.  Refused with a Python
    exception: CPU tensors, tensors that are not float32.  A non-contiguous gradient is made contiguous."""
    return _sumsq(*_optim_table(grads, what='grad_sumsq'))


def grad_norm_finish(partials, max_norm):
    """Second half (regtr_grad_norm_finish): (P,) float64 partials -> (2,) float32 device tensor [total_norm, clip_coef], clip_coef =
    min(1, max_norm / (total_norm + 1e-6)) as torch.nn.utils.clip_grad_norm_; max_norm <= 0: no clipping (coef 1).  No host read."""
    out = torch.empty(2, dtype=torch.float32, device=partials.device)
    n = partials.numel()
    check(_lib.lib().regtr_grad_norm_finish(dptr(partials) if n else None, n, float(max_norm), ptr(out), stream()), 'regtr_grad_norm_finish')
    return out


def _adam_step(tab, n, clip_coef, decoupled):
    check(_lib.lib().regtr_adam_step(tab.ctypes.data if n else None, n, ptr(clip_coef), 1 if decoupled else 0, stream()), 'regtr_adam_step')


def adam_step(params, grads, exp_avgs, exp_avg_sqs, scalars, clip_coef=None, decoupled=True):
    """torch's single-tensor AdamW (decoupled) / Adam step on every tensor in place (regtr_adam_step).  scalars: per tensor (lr,
    weight_decay, beta1, beta2, eps, bias_correction1 = 1 - beta1^t, sqrt(bias_correction2) = sqrt(1 - beta2^t)), host float64.
    clip_coef: a 1-element float32 device tensor the kernel multiplies every gradient by (grad_norm_finish(...)[1:]), None = 1; the
    gradients themselves are not modified.  The kernel writes through raw pointers: the CALLER advances the tensors' version counters
    (regtr_amd.optim.FusedAdamW does).  Refused with a Python exception: CPU tensors; tensors that are not float32; a non-contiguous
    parameter or moment; a gradient whose shape, or a moment whose element count, differs from its parameter's.  A non-contiguous
    gradient is made contiguous."""
    tab, keep = _optim_table(grads, params, exp_avgs, exp_avg_sqs, scalars, what='adam_step')
    if clip_coef is not None and clip_coef.numel() != 1:
        raise RuntimeError(f'adam_step: clip_coef must hold one float32, got {tuple(clip_coef.shape)}')
    _adam_step(tab, len(keep), clip_coef, decoupled)


def clip_adam_step(params, grads, exp_avgs, exp_avg_sqs, scalars, max_norm, decoupled=True):
    """grad_sumsq, grad_norm_finish(max_norm) and adam_step with the coefficient it left on the device, over ONE table of the tensors
    (checked once) -> the (2,) float32 device tensor [total_norm before clipping, clip_coef].  What FusedAdamW.step runs."""
    tab, keep = _optim_table(grads, params, exp_avgs, exp_avg_sqs, scalars, what='clip_adam_step')
    norm_coef = grad_norm_finish(_sumsq(tab, keep), max_norm)
    _adam_step(tab, len(keep), norm_coef[1:], decoupled)
    return norm_coef


# ------------------------------------------------------------------------------------------------ the guarded step (skip_nonfinite)
def optim_guarded_chunk():
    """Tensors per launch of adam_step_guarded -- tests straddle it."""
    return int(_lib.lib().regtr_optim_guarded_chunk_tensors())


def new_guard(device):
    """A zeroed guard word: (4,) int32 on the device, {ok, applied_steps, skipped_steps, reserved} (include/regtr_hip.h)."""
    return torch.zeros(4, dtype=torch.int32, device=device)


def _scalar_arg(t, name, dtype, numel=1):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype is not dtype or t.numel() != numel or not t.is_contiguous():
        raise RuntimeError(f'{name} must be a contiguous GPU tensor of {numel} {dtype} value(s), got {getattr(t, "shape", type(t))} '
                           f'{getattr(t, "dtype", "")} on {getattr(t, "device", "?")}')
    return t


def grad_norm_finish_guarded(partials, max_norm, guard, grad_scale=None):
    """grad_norm_finish under the guard (regtr_grad_norm_finish_guarded): -> (2,) float32 [total_norm * grad_scale, clip_coef]; guard (4,)
    int32 device tensor: guard[0] = ok (the scaled norm and the scale are finite), guard[1] += ok, guard[2] += 1 - ok.  grad_scale: a
    1-element float32 device tensor or None (= 1; then, and with exactly 1.0, the output has grad_norm_finish's bits).  No host read."""
    _scalar_arg(guard, 'grad_norm_finish_guarded: guard', torch.int32, 4)
    _scalar_arg(grad_scale, 'grad_norm_finish_guarded: grad_scale', torch.float32)
    out = torch.empty(2, dtype=torch.float32, device=partials.device)
    n = partials.numel()
    check(_lib.lib().regtr_grad_norm_finish_guarded(dptr(partials) if n else None, n, float(max_norm), ptr(grad_scale), ptr(out),
                                                    guard.data_ptr(), stream()), 'regtr_grad_norm_finish_guarded')
    return out


def _guarded_table(tab, hypers, step_index):
    import numpy as np
    n = len(tab)
    gtab = np.zeros(n, dtype=_table_dtype('guarded'))
    for k in ('p', 'g', 'm', 'v', 'n'):
        gtab[k] = tab[k]
    if n:
        gtab['hyper'] = hypers
        gtab['step_index'] = step_index
    return gtab


def _guarded_tables(params, grads, exp_avgs, exp_avg_sqs, hypers, step_index, what):
    import numpy as np
    n = len(grads)
    if len(hypers) != n or len(step_index) != n:
        raise RuntimeError(f'{what}: hypers and step_index must have one entry per tensor')
    hyp = np.asarray(hypers, dtype=np.float64).reshape(n, 5)
    tab, keep = _optim_table(grads, params, exp_avgs, exp_avg_sqs, np.concatenate([hyp, np.ones((n, 2))], axis=1), what=what)
    return tab, _guarded_table(tab, hyp, step_index), keep


def _adam_step_guarded(gtab, n, steps, step_scalars, guard, clip_coef, grad_scale, decoupled):
    check(_lib.lib().regtr_adam_step_guarded(gtab.ctypes.data if n else None, n, ptr(steps), ptr(step_scalars), steps.numel(), ptr(clip_coef),
                                             ptr(grad_scale), guard.data_ptr(), 1 if decoupled else 0, stream()), 'regtr_adam_step_guarded')


def _guarded_args(steps, guard, grad_scale, what, step_scalars=None):
    """-> the workspace for the per-tensor step scalars, (2 len(steps),) float32: the caller's, or a fresh one."""
    if not isinstance(steps, torch.Tensor) or not steps.is_cuda or steps.dtype is not torch.float32 or not steps.is_contiguous():
        raise RuntimeError(f'{what}: steps must be a contiguous float32 GPU vector; there is no CPU fallback')
    if step_scalars is None:
        step_scalars = torch.empty(2 * steps.numel(), dtype=torch.float32, device=steps.device)
    elif (not isinstance(step_scalars, torch.Tensor) or step_scalars.device != steps.device or step_scalars.dtype is not torch.float32
          or not step_scalars.is_contiguous() or step_scalars.numel() != 2 * steps.numel()):
        raise RuntimeError(f'{what}: step_scalars must be a contiguous float32 vector of 2 x len(steps) on the steps\' device')
    _scalar_arg(guard, f'{what}: guard', torch.int32, 4)
    _scalar_arg(grad_scale, f'{what}: grad_scale', torch.float32)
    return step_scalars


def adam_step_guarded(params, grads, exp_avgs, exp_avg_sqs, hypers, step_index, steps, guard, clip_coef=None, grad_scale=None,
                      decoupled=True, step_scalars=None):
    """adam_step under the guard (regtr_adam_step_guarded).  guard[0] == 0: nothing is written.  Else steps[step_index[i]] += 1 for every
    tensor, then adam_step's update with g' = (g grad_scale) clip_coef and the bias corrections formed ON THE DEVICE from the advanced
    count.  hypers: per tensor (lr, weight_decay, beta1, beta2, eps), host float64; step_index: distinct positions in `steps`, a float32
    device vector; guard: (4,) int32; clip_coef, grad_scale: 1-element float32 device tensors or None (= 1); step_scalars: the (2
    len(steps),) float32 workspace of the per-tensor scalars (None: allocated here).  The tensor checks and the version-counter note of
    adam_step apply."""
    step_scalars = _guarded_args(steps, guard, grad_scale, 'adam_step_guarded', step_scalars)
    if clip_coef is not None and clip_coef.numel() != 1:
        raise RuntimeError(f'adam_step_guarded: clip_coef must hold one float32, got {tuple(clip_coef.shape)}')
    _, gtab, keep = _guarded_tables(params, grads, exp_avgs, exp_avg_sqs, hypers, step_index, 'adam_step_guarded')
    _adam_step_guarded(gtab, len(keep), steps, step_scalars, guard, clip_coef, grad_scale, decoupled)


def clip_adam_step_guarded(params, grads, exp_avgs, exp_avg_sqs, hypers, step_index, steps, guard, max_norm, grad_scale=None,
                           decoupled=True, step_scalars=None):
    """grad_sumsq, grad_norm_finish_guarded(max_norm, grad_scale) and adam_step_guarded over ONE table of the tensors (checked once) ->
    the (2,) float32 device tensor [total_norm * grad_scale before clipping, clip_coef].  What FusedAdamW(skip_nonfinite=True).step
    runs."""
    step_scalars = _guarded_args(steps, guard, grad_scale, 'clip_adam_step_guarded', step_scalars)
    tab, gtab, keep = _guarded_tables(params, grads, exp_avgs, exp_avg_sqs, hypers, step_index, 'clip_adam_step_guarded')
    norm_coef = grad_norm_finish_guarded(_sumsq(tab, keep), max_norm, guard, grad_scale)
    _adam_step_guarded(gtab, len(keep), steps, step_scalars, guard, norm_coef[1:], grad_scale, decoupled)
    return norm_coef


def adam_bias_scalars(lr, beta1, beta2, steps):
    """(n, 2) float32: for every count of the float32 device vector `steps` the two scalars the guarded step forms from it on the device,
    [(float)(lr / (1 - beta1^t)), (float)sqrt(1 - beta2^t)] (regtr_adam_bias_scalars: the kernel's own device function)."""
    if not isinstance(steps, torch.Tensor) or not steps.is_cuda or steps.dtype is not torch.float32 or not steps.is_contiguous():
        raise RuntimeError('adam_bias_scalars: steps must be a contiguous float32 GPU vector; there is no CPU fallback')
    out = torch.empty(steps.numel(), 2, dtype=torch.float32, device=steps.device)
    n = steps.numel()
    with _lib.on_device(steps.device):
        check(_lib.lib().regtr_adam_bias_scalars(float(lr), float(beta1), float(beta2), ptr(steps) if n else None, n, ptr(out) if n else None,
                                                 stream()), 'regtr_adam_bias_scalars')
    return out


def grad_finite_flag(grads, guard):
    """The per-micro-batch flag of the guarded bucket: one grad_sumsq pass over `grads` and a guarded finish (no clip, no scale) into the
    scratch guard word `guard` -- guard[0] = 1 exactly when the float32 norm of the gradients is finite; guard[1] / guard[2] count the
    finite / non-finite calls.  No host read."""
    _scalar_arg(guard, 'grad_finite_flag: guard', torch.int32, 4)
    return grad_norm_finish_guarded(_sumsq(*_optim_table(grads, what='grad_finite_flag')), 0.0, guard)


# ------------------------------------------------------------------------------------------------ gradient bucket (csrc/grad_bucket.hip)
def grad_pack_slice():
    """Elements per workgroup of grad_pack -- tests straddle it."""
    return int(_lib.lib().regtr_grad_pack_slice())


def grad_pack(grads, offsets, bucket, scale, accumulate, sizes=None, flag=None, n_good=None):
    """One launch per 48 tensors (regtr_grad_pack): bucket[offsets[t] + i] = scale grads[t][i], or with accumulate
    fmaf(scale, grads[t][i], bucket[offsets[t] + i]).  grads: float32 GPU tensors or None (None: zeros under assign, untouched under
    accumulate; its length then comes from sizes[t]); offsets: ascending multiples of 4, the segments inside the bucket and disjoint;
    bucket: a contiguous float32 GPU tensor.  Checked once, on the current stream, no host wait.  Elements of the bucket outside every
    segment are not written.  Refused with a Python exception: CPU tensors, tensors that are not float32 or sit on another device; what
    the library refuses (include/regtr_hip.h).  A non-contiguous gradient is made contiguous.
    flag (a guard word, (4,) int32 on the device; None: the unguarded launch above): regtr_grad_pack_guarded -- flag[0] != 0 the same
    arithmetic, flag[0] == 0 zeros under assign and nothing under accumulate; n_good (a 1-element float32 device tensor outside every
    segment, or None) then receives (accumulate ? n_good : 0) + (flag[0] != 0), unscaled."""
    import numpy as np
    n = len(grads)
    if len(offsets) != n or (sizes is not None and len(sizes) != n):
        raise RuntimeError('grad_pack: grads, offsets (and sizes) must have one entry per tensor')
    if not isinstance(bucket, torch.Tensor) or not bucket.is_cuda:
        raise RuntimeError(f'grad_pack: the bucket must be a GPU tensor (got {getattr(bucket, "device", type(bucket))}); there is no CPU fallback')
    have = [g for g in grads if g is not None]
    with _lib.on_device(bucket.device):
        if have and not _optim_all_ok((have,)):
            _optim_explain(have, None, None, None, 'grad_pack')
        keep = [g if g is None or g.is_contiguous() else g.contiguous() for g in grads]
        tab = np.zeros(n, dtype=_table_dtype('bucket'))
        if n:
            if sizes is None and len(have) != n:
                raise RuntimeError('grad_pack: a None gradient needs its length in sizes')
            tab['g'] = [0 if g is None else g.data_ptr() for g in keep]
            tab['n'] = [int(sizes[i]) if g is None else g.numel() for i, g in enumerate(keep)]
            tab['offset'] = offsets
            if sizes is not None and tab['n'].tolist() != [int(s) for s in sizes]:
                raise RuntimeError('grad_pack: a gradient\'s element count differs from its entry in sizes')
        if flag is not None:
            _scalar_arg(flag, 'grad_pack: flag', torch.int32, 4)
            _scalar_arg(n_good, 'grad_pack: n_good', torch.float32)
            check(_lib.lib().regtr_grad_pack_guarded(tab.ctypes.data if n else None, n, ptr(bucket), bucket.numel(), float(scale),
                                                     1 if accumulate else 0, flag.data_ptr(), ptr(n_good), stream()),
                  'regtr_grad_pack_guarded')
            return
        if n_good is not None:
            raise RuntimeError('grad_pack: n_good needs a flag')
        check(_lib.lib().regtr_grad_pack(tab.ctypes.data if n else None, n, ptr(bucket), bucket.numel(), float(scale), 1 if accumulate else 0,
                                         stream()), 'regtr_grad_pack')


# ------------------------------------------------------------------------------------------------ the cloud bank
def gather_segments(feats, bank_seg, cloud_of, dst_seg, n_out, max_len, pe=None, xyz=None, out=None):
    """Whole clouds of a packed bank in a new order, one launch (regtr_gather_segments): destination cloud d is bank cloud cloud_of[d],
    its rows copied from bank_seg[cloud_of[d]] ... to dst_seg[d] ....  feats (N, D) float32 with D % 4 == 0, pe (N, D) and xyz (N, 3)
    optional; bank_seg (C + 1,), cloud_of (n_dst,), dst_seg (n_dst [+ 1],) int32 device tensors; n_out = the selected clouds' rows,
    max_len = the longest selected cloud, both known to the host.  -> (feats', pe' | None, xyz' | None) with n_out rows each; out: the
    same triple preallocated.  Bit-exact copies; nothing here synchronises."""
    for t in (feats, bank_seg, cloud_of, dst_seg, pe, xyz):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device.type != 'cuda'):
            raise RuntimeError(f'gather_segments: every tensor must be on the GPU (got {getattr(t, "device", type(t))}); there is no CPU fallback')
    N, D = feats.shape
    if (pe is not None and tuple(pe.shape) != (N, D)) or (xyz is not None and tuple(xyz.shape) != (N, 3)):
        raise RuntimeError(f'gather_segments: feats (N, D), pe (N, D), xyz (N, 3) expected, got {tuple(feats.shape)}, '
                           f'{None if pe is None else tuple(pe.shape)}, {None if xyz is None else tuple(xyz.shape)}')
    n_dst, n_out, max_len = cloud_of.numel(), int(n_out), int(max_len)
    if dst_seg.numel() < n_dst or bank_seg.numel() < 1:
        raise RuntimeError(f'gather_segments: dst_seg needs {n_dst} entries and bank_seg at least one, got {dst_seg.numel()}, {bank_seg.numel()}')
    if out is None:
        new = lambda src, w: None if src is None else torch.empty((n_out, w), dtype=torch.float32, device=feats.device)
        out = (new(feats, D), new(pe, D), new(xyz, 3))
    o_f, o_p, o_x = out
    if tuple(o_f.shape) != (n_out, D) or (pe is not None and tuple(o_p.shape) != (n_out, D)) or (xyz is not None and tuple(o_x.shape) != (n_out, 3)):
        raise RuntimeError(f'gather_segments: the outputs must have {n_out} rows of the inputs\' widths')
    check(_lib.lib().regtr_gather_segments(ptr(feats), ptr(pe), ptr(xyz), D, iptr(bank_seg), bank_seg.numel() - 1, N, iptr(cloud_of),
                                           iptr(dst_seg), n_dst, n_out, max_len, ptr(o_f), ptr(o_p) if pe is not None else None,
                                           ptr(o_x) if xyz is not None else None, stream()), 'regtr_gather_segments')
    return o_f, (o_p if pe is not None else None), (o_x if xyz is not None else None)
