"""GPU: every launch regime of csrc/preprocess.hip (grid subsample, cell grid, both radius-search kernels), bit exact against the C++
oracle and, where its brute force is too slow, against the linear-time restatement of tests/preprocess_ref.py.

Every parametrized case carries the label tests/dispatch.py derives for its shape and asserts it before it runs, so a retuned constant
fails the case and does not silently move it; tests/test_dispatch_routes.py fails when a label of dispatch.PREPROCESS_KERNELS is reached
by no case here.  There is no tolerance in this file: indices, counts, the max count, segment offsets and the uint32 view of the
barycentres are compared with np.array_equal.  The entry points are called through the C ABI on sentinel-filled outputs with guard rows:
rows between the live count and the capacity, and the guard rows behind it, must come back untouched."""
import numpy as np
import pytest
import torch

from tests import dispatch
from tests import preprocess_ref as PR

pytestmark = pytest.mark.gpu

ISENT = -777
FSENT = 777.0
GUARD = 5


def _lib():
    from regtr_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _seg(lens):
    return _dev(np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int32))


def _pad_rows(pts, cap, fill=1e9):
    """(cap, 3) device tensor whose first rows are pts; the rows behind the live count hold a value no kernel may read into a result."""
    out = np.full((max(cap, 1), 3), fill, np.float32)
    out[:len(pts)] = pts
    return _dev(out)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device='cuda')


def _check(status, what):
    assert status == 0, f'{what}: status {status}'


def subsample(pts, lens, n_cap, dl, row_order=0, out_cap=None, ws=None):
    """regtr_grid_subsample_ordered -> (rows [total, 3] float32, segment offsets).  Output rows from the total on, guard rows included,
    must be untouched."""
    L = _lib()
    nc = len(lens)
    oc = n_cap if out_cap is None else out_cap
    xyz, seg = _pad_rows(pts, n_cap), _seg(lens)
    out = torch.full((oc + GUARD, 3), FSENT, dtype=torch.float32, device='cuda')
    off = torch.full((nc + 1 + GUARD,), ISENT, dtype=torch.int32, device='cuda')
    nb = L.regtr_grid_subsample_ordered_ws_bytes(n_cap, nc, row_order)
    assert nb == dispatch.grid_subsample_ws_bytes(n_cap, nc, row_order)
    ws = _ws(nb) if ws is None else ws
    assert ws.numel() >= nb
    _check(L.regtr_grid_subsample_ordered(xyz.data_ptr(), seg.data_ptr(), nc, n_cap, float(dl), row_order, 0, oc, out.data_ptr(),
                                          off.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'regtr_grid_subsample_ordered')
    off, out = off.cpu().numpy(), out.cpu().numpy()
    assert (off[nc + 1:] == ISENT).all()
    total = int(off[nc])
    assert 0 <= total <= oc and (out[total:] == np.float32(FSENT)).all(), 'rows behind the total were written'
    return out[:total], off[:nc + 1]


def check_subsample(pts, lens, n_cap, dl, row_order=0, ws=None):
    got, off = subsample(pts, lens, n_cap, dl, row_order, ws=ws)
    ref_p, ref_l = PR.oracle_subsample(pts, lens, dl, ref_order=bool(row_order))
    assert np.array_equal(np.diff(off), ref_l)
    assert np.array_equal(got.view(np.uint32), ref_p.view(np.uint32)), 'barycentres / row order not bit exact'
    return got, ref_l


class Grid:
    """regtr_cellgrid_build over `s` (live rows) at capacity ns_cap, then queries through either kernel."""

    def __init__(self, s, s_lens, ns_cap, r, ws=None):
        L = _lib()
        self.n, self.cap, self.nc, self.r = len(s), ns_cap, len(s_lens), float(r)
        self.xyz, self.seg = _pad_rows(s, ns_cap), _seg(s_lens)
        self.nbytes = L.regtr_cellgrid_ws_bytes(ns_cap, self.nc)
        assert self.nbytes == dispatch.cellgrid_ws_bytes(ns_cap)
        self.ws = _ws(self.nbytes) if ws is None else ws
        assert self.ws.numel() >= self.nbytes
        _check(L.regtr_cellgrid_build(self.xyz.data_ptr(), self.seg.data_ptr(), self.nc, ns_cap, self.r, self.ws.data_ptr(),
                                      self.ws.numel(), _stream()), 'regtr_cellgrid_build')

    def _out(self, rows, K):
        return (torch.full((rows + GUARD, K), ISENT, dtype=torch.int32, device='cuda'),
                torch.full((rows + GUARD,), ISENT, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'))

    @staticmethod
    def _take(idx, cnt, mx, live):
        idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
        assert (idx[live:] == ISENT).all() and (cnt[live:] == ISENT).all(), 'rows behind the live count were written'
        return idx[:live], cnt[:live], int(mx.item())

    def query(self, q, q_lens, nq_cap, K, order=0):
        idx, cnt, mx = self._out(nq_cap, K)
        qx, qseg = _pad_rows(q, nq_cap), _seg(q_lens)
        _check(_lib().regtr_radius_query(qx.data_ptr(), qseg.data_ptr(), nq_cap, self.seg.data_ptr(), self.cap, self.nc, self.r, K, order,
                                         self.ws.data_ptr(), self.ws.numel(), idx.data_ptr(), cnt.data_ptr(), mx.data_ptr(), _stream()),
               'regtr_radius_query')
        return self._take(idx, cnt, mx, len(q))

    def query_supports(self, K, order=0):
        """The general kernel over the grid's own supports."""
        idx, cnt, mx = self._out(self.cap, K)
        _check(_lib().regtr_radius_query(self.xyz.data_ptr(), self.seg.data_ptr(), self.cap, self.seg.data_ptr(), self.cap, self.nc, self.r,
                                         K, order, self.ws.data_ptr(), self.ws.numel(), idx.data_ptr(), cnt.data_ptr(), mx.data_ptr(),
                                         _stream()), 'regtr_radius_query')
        return self._take(idx, cnt, mx, self.n)

    def query_self(self, K, order=0):
        idx, cnt, mx = self._out(self.cap, K)
        _check(_lib().regtr_radius_query_self(self.seg.data_ptr(), self.cap, self.nc, self.r, K, order, self.ws.data_ptr(), self.ws.numel(),
                                              idx.data_ptr(), cnt.data_ptr(), mx.data_ptr(), _stream()), 'regtr_radius_query_self')
        return self._take(idx, cnt, mx, self.n)


def _same(got, ref_idx, ref_cnt, what, rows=None):
    idx, cnt, mx = got
    if rows is not None:
        idx, cnt = idx[rows], cnt[rows]
    else:
        assert mx == (int(ref_cnt.max()) if len(ref_cnt) else 0), what
    assert np.array_equal(cnt, ref_cnt), f'{what}: counts'
    assert np.array_equal(idx, ref_idx), f'{what}: neighbour indices not bit exact'


# ------------------------------------------------------------------------------------------------ scan forms through the subsample
# (point capacity, live points, route): one tile; the last chained capacity and the first three-launch one; one sum per thread of
# k_scan_bsums and the first capacity whose carry loop runs twice; live n << capacity in the chained and in the three-launch form
SUB_SCAN_CASES = [(1000, 1000, 'sub/scan/chained1'), (65536, 65536, 'sub/scan/chained'), (65537, 65537, 'sub/scan/three/per1'),
                  (262144, 262144, 'sub/scan/three/per1'), (262145, 262145, 'sub/scan/three/perN'),
                  (65536, 5000, 'sub/scan/chained'), (65537, 5000, 'sub/scan/three/per1'), (262145, 3001, 'sub/scan/three/perN')]


@pytest.mark.parametrize('n_cap,n_live,route', SUB_SCAN_CASES)
def test_subsample_scan_forms(n_cap, n_live, route):
    assert dispatch.route_subsample(n_cap) == route
    pts, lens = PR.lattice_clouds(n_live, 100 + n_live % 97)
    assert lens[1] == 0 and (pts < 0).any()
    got, ref_l = check_subsample(pts, lens, n_cap, 0.05)
    assert len(got) < 0.8 * n_live                                            # voxels hold several members
    print(f'subsample {n_cap=} {n_live=} {route}: {len(got)} voxels')


# ------------------------------------------------------------------------------------------------ scan forms through the cell grid
# (support capacity = live supports, route): the scan runs over the allocated table of 1.5 ns rounded up to a power of two
GRID_SCAN_CASES = [(600, 'grid/scan/chained1'), (43690, 'grid/scan/chained'), (43692, 'grid/scan/three/per1'),
                   (174762, 'grid/scan/three/per1'), (174764, 'grid/scan/three/perN')]


@pytest.mark.parametrize('ns,route', GRID_SCAN_CASES)
def test_cellgrid_scan_forms(ns, route):
    assert dispatch.route_cellgrid(ns) == route
    K = 16
    pts, lens, r = PR.uniform_clouds(ns, 7 + ns % 11)
    got = Grid(pts, lens, ns, r).query_supports(K)
    ref_idx, ref_cnt = PR.binned_radius(pts, pts, lens, lens, r, K)
    _same(got, ref_idx, ref_cnt, 'all rows vs the binned reference')
    rows = np.arange(0, ns, max(ns // 2000, 1))[:2000]
    ql = np.array([(rows < lens[0]).sum(), (rows >= lens[0]).sum()], np.int32)
    o_idx, o_cnt = PR.oracle_radius(pts[rows], pts, ql, lens, r, K)
    _same(got, o_idx, o_cnt, 'strided rows vs the oracle', rows)
    assert (ref_cnt > K).any() and (ref_cnt < K).any()                        # truncated rows and padded rows


# ------------------------------------------------------------------------------------------------ self-query chunking
# (support capacity, live supports, route): slots per wave 4 and 8 (a level far below its capacity), 16 (capacity = live), 32 and 64
# in one step (tables of 2^20 and 2^21 slots), 64 in two steps (2^22 slots).  The last three are the first live counts of their
# regimes; the first of them lies below 350 000 supports, where every row is compared with the reference
SELF_CASES = [(8000, 2000, 'self/spw4/pass1'), (8000, 4000, 'self/spw8/pass1'), (8000, 8000, 'self/spw16/pass1'),
              (349526, 349526, 'self/spw32/pass1'), (699052, 699052, 'self/spw64/pass1'), (1398102, 1398102, 'self/spw64/passN')]


@pytest.mark.parametrize('ns_cap,ns,route', SELF_CASES)
def test_self_query_chunking(ns_cap, ns, route):
    assert dispatch.route_radius_self(ns_cap, ns) == route
    if ns > 8000:
        assert dispatch.route_radius_self(ns_cap - 1, ns - 1) != route       # the smallest size of its regime
    K = 16
    pts, lens, r = PR.uniform_clouds(ns, 31 + ns % 13)
    grid = Grid(pts, lens, ns_cap, r)
    got = grid.query_self(K)
    if ns <= 8000:
        ref_idx, ref_cnt = PR.oracle_radius(pts, pts, lens, lens, r, K)
        _same(got, ref_idx, ref_cnt, 'self kernel, all rows vs the oracle')
    elif ns < 350000:
        ref_idx, ref_cnt = PR.binned_radius(pts, pts, lens, lens, r, K)
        _same(got, ref_idx, ref_cnt, 'self kernel, all rows vs the binned reference')
    else:
        rows = np.arange(3, ns, 16)                                           # one query in 16 over the whole index range
        ref_idx, ref_cnt = PR.binned_radius(pts, pts, lens, lens, r, K, q_rows=rows)
        _same(got, ref_idx, ref_cnt, 'self kernel, strided rows vs the binned reference', rows)
    per = grid.query_supports(K)                                              # and ALL rows against the per-query kernel
    assert got[2] == per[2] and np.array_equal(got[1], per[1]) and np.array_equal(got[0], per[0]), 'self kernel != per-query kernel'
    assert 10 <= got[1].mean() <= 30


# ------------------------------------------------------------------------------------------------ per-query kernel: runs of queries, empty waves
# (query capacity, live queries, route, trailing waves empty)
RQ_CASES = [(70001, 70001, 'rq/per_waveN', True), (131072, 131072, 'rq/per_waveN', False), (16000, 1000, 'rq/per_wave1', True),
            (1001, 1001, 'rq/per_wave1', True)]


@pytest.mark.parametrize('nq_cap,nq,route,empty', RQ_CASES)
def test_radius_query_wave_runs(nq_cap, nq, route, empty):
    assert dispatch.route_radius_query(nq_cap, nq) == (route, empty)
    K = 16
    s, s_lens, r = PR.uniform_clouds(20011, 5)
    rng = np.random.default_rng(nq)
    pick = np.sort(rng.integers(0, len(s), nq))
    q = (s[pick] + rng.normal(0, 0.2, (nq, 3))).astype(np.float32)
    q_lens = np.array([(pick < s_lens[0]).sum(), (pick >= s_lens[0]).sum()], np.int32)
    got = Grid(s, s_lens, len(s), r).query(q, q_lens, nq_cap, K)
    ref_idx, ref_cnt = PR.binned_radius(q, s, q_lens, s_lens, r, K)
    _same(got, ref_idx, ref_cnt, 'all rows vs the binned reference')
    rows = np.arange(0, nq, max(nq // 1500, 1))
    ql = np.array([(rows < q_lens[0]).sum(), (rows >= q_lens[0]).sum()], np.int32)
    _same(got, *PR.oracle_radius(q[rows], s, ql, s_lens, r, K), 'strided rows vs the oracle', rows)


# ------------------------------------------------------------------------------------------------ row regimes
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('K', PR.ROW_KS)
@pytest.mark.parametrize('kernel', ['rq', 'self'])
def test_row_regimes(kernel, K, order):
    """One generator of small clustered clouds (tests/preprocess_ref.py: row_case) through both kernels, both orders and five list
    capacities.  The reference counts must show listed lengths 0 (general kernel), 1, 31, 32, 33, 40, 64, 65, 72 (a multiple of 8 and
    non-multiples above 32), balls that shrink once and at least twice at this K's capacity, and -- the self kernel -- cells with
    at most 256 and with more candidates, a shrink among the latter.  The blobs of 256 and 257 points, each alone in its 27 cells, are
    the exact staging boundary: the generator produces it deterministically."""
    c = PR.row_case()
    labels, listed = PR.row_case_labels(K, kernel)
    cap = dispatch.radius_cap(K)
    capc = {256: 'cap256', 320: 'cap_mid', 512: 'cap_limit' if K == 448 else 'cap512'}[cap]
    assert {'rank/two_lane', 'rank/general/pad0', 'rank/general/pad', f'shrink1/{capc}', f'shrink2/{capc}'} <= labels, sorted(labels)
    if K == 16:
        assert {1, 31, 32, 33, 40, 64, 65, 72} <= listed and (kernel == 'self' or 0 in listed), sorted(listed)
    grid = Grid(c['s'], c['s_lens'], len(c['s']), c['r'])
    if kernel == 'self':
        assert {'cand/staged', 'cand/unstaged', 'cand/unstaged/shrink'} <= labels
        tot = PR.candidate_totals(c['s'], c['s'], c['s_lens'], c['s_lens'], c['r'])
        assert {256, 257} <= set(tot.tolist())
        got = grid.query_self(K, order)
        ref = PR.oracle_radius(c['s'], c['s'], c['s_lens'], c['s_lens'], c['r'], K, order)
    else:
        tot = PR.candidate_totals(c['q'], c['s'], c['q_lens'], c['s_lens'], c['r'])
        _, cnt = PR.oracle_radius(c['q'], c['s'], c['q_lens'], c['s_lens'], c['r'], 1)
        assert ((cnt == 0) & (tot == 0)).any() and ((cnt == 0) & (tot > 0)).any()    # an empty row without and with candidates
        got = grid.query(c['q'], c['q_lens'], len(c['q']), K, order)
        ref = PR.oracle_radius(c['q'], c['s'], c['q_lens'], c['s_lens'], c['r'], K, order)
    _same(got, *ref, f'{kernel} K={K} order={order}')


# ------------------------------------------------------------------------------------------------ many clouds
@pytest.mark.parametrize('n_clouds', [130, 260])
def test_many_clouds(n_clouds):
    """rg_find_segment_wave steps 64 clouds at a time and k_bbox leaves its register path when a wave straddles clouds: 130 and 260
    clouds of 0 .. 90 points (first, last and runs of consecutive clouds empty), every row of the subsample (both row orders), the self
    table and the pool table against the oracle."""
    pts, lens, r, dl = PR.many_clouds(n_clouds)
    assert lens[0] == 0 and lens[-1] == 0 and (lens[62:67] == 0).all() and lens.max() == 90 and (lens == 0).sum() > n_clouds // 10
    assert dispatch.route_subsample(len(pts), 1) == 'sub/scan/chained+sub/ref_order'
    sub, sub_l = check_subsample(pts, lens, len(pts), dl)
    check_subsample(pts, lens, len(pts), dl, row_order=1)
    K = 16
    grid = Grid(pts, lens, len(pts), r)
    ref = PR.oracle_radius(pts, pts, lens, lens, r, K)
    _same(grid.query_self(K), *ref, 'self table')
    _same(grid.query_supports(K), *ref, 'conv table, per-query kernel')
    _same(grid.query(sub, sub_l, len(sub), K), *PR.oracle_radius(sub, pts, sub_l, lens, r, K), 'pool table')
    _same(grid.query(sub, sub_l, len(sub), K, order=1), *PR.oracle_radius(sub, pts, sub_l, lens, r, K, 1), 'pool table, order 1')
    assert (ref[1] > K).any()


# ------------------------------------------------------------------------------------------------ workspace independence
def _fill_ws(ws, how, big_build):
    if how == 'zeros':
        ws.zero_()
    elif how == 'ones':
        ws.fill_(0xFF)
    else:
        big_build()


@pytest.mark.parametrize('cap', [4800, 70000])
def test_cellgrid_ignores_workspace_leftovers(cap):
    """One caller-held workspace: filled with 0x00, with 0xFF, then with what a build over 8 x as many supports at the same capacity
    leaves; the build + both queries over cap / 8 live supports give the reference's table each time.  (4800: the chained scan's
    zeroed state; 70000: the three-launch scan.)"""
    n, K = cap // 8, 16
    big, big_lens, r = PR.uniform_clouds(cap, 1)
    pts, lens, _ = PR.uniform_clouds(n, 2)
    ws = _ws(_lib().regtr_cellgrid_ws_bytes(cap, 2))
    ref = PR.oracle_radius(pts, pts, lens, lens, r, K)
    outs = []
    for how in ('zeros', 'ones', 'big'):
        _fill_ws(ws, how, lambda: Grid(big, big_lens, cap, r, ws=ws).query_self(K))
        grid = Grid(pts, lens, cap, r, ws=ws)
        outs.append((grid.query_self(K), grid.query_supports(K)))
        for got in outs[-1]:
            _same(got, *ref, f'workspace pre-filled with {how}')
    assert dispatch.live_table(n) < dispatch.live_table(cap)                  # the big build's table reaches beyond the small one's


@pytest.mark.parametrize('cap', [4800, 70000])
def test_subsample_ignores_workspace_leftovers(cap):
    n = cap // 8
    big, big_lens = PR.lattice_clouds(cap, 1)
    pts, lens = PR.lattice_clouds(n, 2)
    for row_order in (0, 1):
        ws = _ws(_lib().regtr_grid_subsample_ordered_ws_bytes(cap, 3, row_order))
        for how in ('zeros', 'ones', 'big'):
            _fill_ws(ws, how, lambda: subsample(big, big_lens, cap, 0.05, row_order, ws=ws))
            check_subsample(pts, lens, cap, 0.05, row_order, ws=ws)


# ------------------------------------------------------------------------------------------------ out_cap
def test_subsample_out_cap_saturates():
    """k_out_offsets saturates the segment offsets at out_cap and k_barycentres drops the rows beyond it: the first out_cap rows are the
    unsaturated result's, the guard rows stay untouched (checked in `subsample`), and out_cap == the voxel count reads as full."""
    n = 30000
    pts, lens = PR.lattice_clouds(n, 9)
    ref_p, ref_l = PR.oracle_subsample(pts, lens, 0.05)
    ref_off = np.concatenate([[0], np.cumsum(ref_l)]).astype(np.int32)
    V = int(ref_off[-1])
    assert ref_off[1] < V - 700 < V                                           # the cut falls inside the last cloud
    for out_cap in (V - 700, int(ref_off[1]) - 10, V, V + 1):
        got, off = subsample(pts, lens, n, 0.05, out_cap=out_cap)
        assert np.array_equal(off, np.minimum(ref_off, out_cap)), out_cap
        assert len(got) == min(V, out_cap) and np.array_equal(got.view(np.uint32), ref_p[:out_cap].view(np.uint32)), out_cap
