"""References and seeded case generators for the preprocessing route tests (tests/test_gpu_preprocess_routes.py on the GPU,
tests/test_dispatch_routes.py on the host).  numpy and the project's C++ oracle only: nothing here touches the GPU or the library.

  * oracle_radius / oracle_subsample: oracle/regtr_oracle.cpp (brute force per cloud; the subsample is linear time).  order 1 (the first K
    supports of the ball by index) is taken from the oracle's complete (d2, index) list, re-sorted by index.
  * binned_radius: a linear-time restatement for sizes the brute force cannot serve.  Supports are binned into cubic cells of any side
    >= r (a margin of 1e-5 r covers the float32 rounding of d2), the 27 cells around a query hold every support of its ball, distances are evaluated in the reference's float32 order
    ((0 + dx dx) + dy dy) + dz dz with a strict `<` against the float32 r r, rows ascend by (d2 bits, index) -- by index alone for
    order 1 -- and are padded with the live support count.  tests/test_dispatch_routes.py holds it equal to the oracle element for
    element on every small case below.
  * candidate_totals: how many supports the kernels' OWN cell rule (dispatch.cell_index) puts in the 27 cells of a query.  A label, never
    a result.
  * the generators: seeded numpy, so the host test sees the very data the GPU test runs."""
import functools

import numpy as np

from tests import dispatch

F32 = np.float32


def cloud_ids(lens):
    return np.repeat(np.arange(len(lens)), np.asarray(lens, np.int64))


def _lens(lens):
    return np.asarray(lens, np.int32)


# ------------------------------------------------------------------------------------------------ the oracle
def oracle_radius(q, s, q_lens, s_lens, r, K, order=0):
    """-> (idx (nq, K) int32 padded with len(s), count (nq,) int32) by oracle.native.radius_neighbors."""
    from oracle import native
    q_lens, s_lens = _lens(q_lens), _lens(s_lens)
    idx, cnt, _ = native.radius_neighbors(q, s, q_lens, s_lens, r, K)
    if order == 0 or len(q) == 0:
        return idx, cnt
    W = max(int(cnt.max()), K)
    full = native.radius_neighbors(q, s, q_lens, s_lens, r, W)[0]       # the whole ball of every query; the padding (= len(s)) sorts last
    return np.ascontiguousarray(np.sort(full, axis=1)[:, :K]), cnt


def oracle_subsample(pts, lens, dl, ref_order=False):
    from oracle import native
    return native.grid_subsample(pts, _lens(lens), dl, ref_order=ref_order)


# ------------------------------------------------------------------------------------------------ linear-time restatement
class _Bins:
    """Supports sorted by (cloud, integer cell); lookup of the 27 cells around query cells."""

    def __init__(self, cells, cloud, n_clouds):
        self.lo = cells.min(0) - 2                                      # two cells of margin: a query next to the box has neighbours in it
        self.dim = (cells.max(0) + 2 - self.lo + 1).astype(np.int64)
        assert float(n_clouds) * float(self.dim[0]) * float(self.dim[1]) * float(self.dim[2]) < 2.0 ** 62
        key = self.key(cells, cloud)
        self.order = np.argsort(key, kind='stable')
        self.keys, self.start, self.count = np.unique(key[self.order], return_index=True, return_counts=True)

    def key(self, cells, cloud):
        c = cells - self.lo
        return ((cloud.astype(np.int64) * self.dim[0] + c[:, 0]) * self.dim[1] + c[:, 1]) * self.dim[2] + c[:, 2]

    def runs(self, cells, cloud):
        """(start, count) int64 arrays [n, 27] of the sorted-support runs in the 27 cells around each query cell."""
        n = len(cells)
        start = np.zeros((n, 27), np.int64)
        count = np.zeros((n, 27), np.int64)
        inside = ((cells >= self.lo + 1) & (cells <= self.lo + self.dim - 2)).all(1)     # beyond the margin: no support near
        cin = np.where(inside[:, None], cells, self.lo + 1)
        for k in range(27):
            d = np.array([k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1], np.int64)
            key = self.key(cin + d, cloud)
            pos = np.searchsorted(self.keys, key)
            hit = inside & (pos < len(self.keys))
            hit[hit] = self.keys[pos[hit]] == key[hit]
            start[hit, k] = self.start[pos[hit]]
            count[hit, k] = self.count[pos[hit]]
        return start, count


def _expand(start, count):
    """Flat (row, position) of every element of the runs [start, start + count) of every row."""
    tot = count.sum(1)
    row = np.repeat(np.arange(len(tot)), tot)
    flat_start = np.repeat(start.ravel(), count.ravel())
    first = np.cumsum(count.ravel()) - count.ravel()
    within = np.arange(int(tot.sum())) - np.repeat(first, count.ravel())
    return row, flat_start + within


def binned_radius(q, s, q_lens, s_lens, r, K, order=0, cell=None, q_rows=None, chunk=40000):
    """-> (idx (n, K) int32 padded with len(s), count (n,) int32) for the query rows q_rows (default all).  cell: side of the bins,
    any value >= r (1 + 1e-5) (default 1.001 r)."""
    q, s = np.ascontiguousarray(q, F32), np.ascontiguousarray(s, F32)
    r = F32(r)
    r2 = r * r                                                          # float32 product, as the reference forms it
    side = float(r) * 1.001 if cell is None else float(cell)
    assert side >= float(r) * (1 + 1e-5)           # float32 rounding of d2 can admit a support a few ulp beyond r
    ns = len(s)
    q_cloud_all, s_cloud = cloud_ids(q_lens), cloud_ids(s_lens)
    assert len(q_cloud_all) == len(q) and len(s_cloud) == ns
    rows = np.arange(len(q)) if q_rows is None else np.asarray(q_rows, np.int64)
    idx = np.full((len(rows), K), ns, np.int32)
    cnt = np.zeros(len(rows), np.int32)
    if ns == 0 or len(rows) == 0:
        return idx, cnt
    bins = _Bins(np.floor(s.astype(np.float64) / side).astype(np.int64), s_cloud, len(_lens(s_lens)))
    qcol, scol = [np.ascontiguousarray(q[:, a]) for a in range(3)], [np.ascontiguousarray(s[:, a]) for a in range(3)]
    for c0 in range(0, len(rows), chunk):
        rr = rows[c0:c0 + chunk]
        qq = q[rr]
        start, count = bins.runs(np.floor(qq.astype(np.float64) / side).astype(np.int64), q_cloud_all[rr])
        row, pos = _expand(start, count)
        sup = bins.order[pos]
        d2 = F32(0)
        for a in range(3):                                              # ((0 + dx dx) + dy dy) + dz dz, every step rounded to float32
            d = qcol[a][rr[row]] - scol[a][sup]
            d2 = d2 + d * d
        assert d2.dtype == F32
        keep = d2 < r2
        row, sup, d2 = row[keep], sup[keep], d2[keep]
        major = row << 32                                               # one key for (row, d2 bits): d2 >= 0, so its bits order as its value
        if order == 0:
            major = major | d2.view(np.uint32).astype(np.int64)
        o = np.lexsort((sup, major))
        row, sup = row[o], sup[o]
        n_in = np.bincount(row, minlength=len(rr))
        cnt[c0:c0 + chunk] = n_in
        rank = np.arange(len(row)) - np.repeat(np.cumsum(n_in) - n_in, n_in)
        ok = rank < K
        idx[c0 + row[ok], rank[ok]] = sup[ok]
    return idx, cnt


def candidate_totals(q, s, q_lens, s_lens, r):
    """Supports in the 27 cells (the KERNELS' cell rule) around each query: the `total` both radius kernels loop over."""
    ns = len(s)
    if ns == 0 or len(q) == 0:
        return np.zeros(len(q), np.int64)
    bins = _Bins(dispatch.cell_index(s, r), cloud_ids(s_lens), len(_lens(s_lens)))
    return bins.runs(dispatch.cell_index(q, r), cloud_ids(q_lens))[1].sum(1)


# ------------------------------------------------------------------------------------------------ generators
def uniform_clouds(n, seed, per_ball=20.0):
    """n uniform points in two cubes (45 % / 55 %) at a density of ~per_ball supports in a ball of radius 1: (pts, lens, r = 1)."""
    rng = np.random.default_rng(seed)
    lens = np.array([n * 45 // 100, n - n * 45 // 100], np.int32)
    rho = per_ball / (4.0 / 3.0 * np.pi)
    parts = [(rng.random((m, 3), dtype=F32) - F32(0.5)) * F32((max(m, 1) / rho) ** (1.0 / 3.0)) for m in lens]
    return np.concatenate(parts).astype(F32), lens, 1.0


def lattice_clouds(n, seed, step=0.013):
    """n points on a lattice with negative coordinates (exact ties; about two members per 0.05 voxel, many voxels with several) in 3
    clouds, the middle one empty: (pts, lens)."""
    rng = np.random.default_rng(seed)
    half = max(int(round((n / 2.0) ** (1.0 / 3.0) * 0.05 / 2 / step)), 4)
    lens = np.array([n * 2 // 5, 0, n - n * 2 // 5], np.int32)
    pts = (rng.integers(-half, half, (n, 3)).astype(F32) * F32(step)).astype(F32)
    pts[lens[0]:] += F32(0.4)
    return pts, lens


def many_clouds(n_clouds, seed=3):
    """Clouds of 0 .. 90 points sharing one region of space (the same cells occur in many clouds); the first and the last cloud are empty,
    there are runs of consecutive empty clouds, one straddling a 64-cloud boundary.  (pts, lens, r, dl)."""
    rng = np.random.default_rng(seed + n_clouds)
    lens = rng.integers(1, 91, n_clouds).astype(np.int32)
    lens[[0, n_clouds - 1]] = 0
    lens[10:14] = 0
    lens[62:67] = 0
    if n_clouds > 200:
        lens[126:131] = 0
    lens[rng.choice(np.arange(20, n_clouds - 1), n_clouds // 10, replace=False)] = 0
    lens[17], lens[18] = 90, 1
    pts = (np.round(rng.random((int(lens.sum()), 3)) * 0.25 / 0.004) * 0.004 - 0.1).astype(F32)       # lattice: ties and duplicates
    return pts, lens, 0.1, 0.05


# isolated blobs whose points all lie within r of each other: every candidate of a row is in its ball, so the list lengths, the
# candidate totals and the shrinks of those rows follow from the blob size alone, whatever order a cell holds its supports in
BLOB_SIZES = (1, 31, 32, 33, 40, 64, 65, 72, 193, 256, 257, 300, 460, 512, 576, 720)
ROW_R = 0.1
ROW_KS = (16, 40, 160, 300, 448)


@functools.lru_cache(maxsize=None)
def row_case():
    """The row-regime case: cloud 0 = the blobs, 1.0 apart; cloud 1 = empty; cloud 2 = a clustered lattice cloud with duplicates.
    -> dict(s, s_lens, q, q_lens, blob_of (per support of cloud 0), n_miss): q = every third support, then per cloud queries with no
    support in the ball: far from everything (no candidate either) and just outside a blob (candidates, none in the ball)."""
    from tests.util import synth_cloud
    rng = np.random.default_rng(21)
    r = ROW_R
    blobs, blob_of = [], []
    for b, m in enumerate(BLOB_SIZES):
        centre = np.array([b % 4, (b // 4) % 4, 0.37 * b]) * 1.0 - 2.0
        p = centre + rng.random((m, 3)) * (r * 0.5)
        if m >= 40:
            p[m // 2:m // 2 + 4] = p[:4]                                # duplicates: d2 ties broken by index
        blobs.append(p)
        blob_of += [b] * m
    c0 = np.concatenate(blobs).astype(F32)
    c2 = synth_cloud(rng, 1500, extent=1.0, lattice=0.01) + F32(7.0)
    c2 = np.concatenate([c2, c2[:200]]).astype(F32)
    s = np.concatenate([c0, c2])
    s_lens = np.array([len(c0), 0, len(c2)], np.int32)
    last = blobs[-1]
    corner = last[np.argmax(last.sum(1))]                               # every blob point lies behind it along (1, 1, 1): q = corner + d is
    above = [corner + d for d in (0.06, 0.065, 0.07)]                   # sqrt(3) d > r from all of them, yet within one cell of the corner
    miss0 = np.concatenate([c0[:3] + F32(40.0), np.array(above, F32)])
    miss2 = (c2[:4] + F32(55.0)).astype(F32)
    q = np.concatenate([c0[::3], miss0, c2[::3], miss2]).astype(F32)
    q_lens = np.array([len(c0[::3]) + len(miss0), 0, len(c2[::3]) + len(miss2)], np.int32)
    return dict(s=s, s_lens=s_lens, q=q, q_lens=q_lens, blob_of=np.array(blob_of), r=r)


def blob_rounds(m):
    """In-ball counts per 64-candidate round of a row of an m-point blob."""
    return [64] * (m // 64) + ([m % 64] if m % 64 else [])


@functools.lru_cache(maxsize=None)
def row_case_labels(K, kernel):
    """The data-dependent labels the rows of row_case() reach at this K, from REFERENCE counts: rows of blobs from the blob size; any other
    row only when its ball leaves no doubt (count + 64 <= cap: no shrink whatever the order of its candidates).  kernel: 'rq' (queries q)
    or 'self' (queries = supports).  -> (labels, listed lengths seen)."""
    c = row_case()
    q, ql = (c['q'], c['q_lens']) if kernel == 'rq' else (c['s'], c['s_lens'])
    cap = dispatch.radius_cap(K)
    _, cnt = oracle_radius(q, c['s'], ql, c['s_lens'], c['r'], 1)
    tot = candidate_totals(q, c['s'], ql, c['s_lens'], c['r'])
    labels, listed = set(), set()
    n0 = int(c['s_lens'][0])
    is_blob_row = np.zeros(len(q), bool)
    if kernel == 'self':
        is_blob_row[:n0] = True
        size = np.array(BLOB_SIZES)[c['blob_of']]
    else:
        nb = len(c['s'][:n0][::3])
        is_blob_row[:nb] = True
        size = np.array(BLOB_SIZES)[c['blob_of'][::3]]
    for m in np.unique(size):
        rows = np.nonzero(is_blob_row)[0][size == m]
        assert (cnt[rows] == m).all() and (tot[rows] == m).all(), (m, cnt[rows], tot[rows])     # the blob really is one ball, alone in its cells
        labels |= dispatch.row_labels(int(m), blob_rounds(int(m)), K)
        listed.add(dispatch.shrinks(blob_rounds(int(m)), cap, K)[1])
    for i in np.nonzero(~is_blob_row & (cnt + 64 <= cap))[0]:
        n, t = int(cnt[i]), int(tot[i])
        labels |= dispatch.row_labels(t, [n] if t else [], K)
        listed.add(n)
    if kernel == 'rq':
        labels.discard('cand/staged'); labels.discard('cand/unstaged'); labels.discard('cand/unstaged/shrink')   # the general kernel never stages
    return frozenset(labels), frozenset(listed)
