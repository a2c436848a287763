"""GPU (and one host test of the generators): the wave-level grouping of the hash-grid build (csrc/preprocess.hip: wave_group in k_insert,
k_scatter_members, k_scatter_cells).  Lanes of a wave that hold the same (key, cloud) issue their table transactions once, through the group's leader; these cases place the
groups where that can go wrong, at 1, 63, 64, 65 and 130 points (below, at and above one wave; three waves, the last one partial):

  one          every point in one voxel / cell: one group per wave, reservations of 64 + 64 + 2 into one list
  distinct     every point in a voxel of its own: groups of one.  130 keys in a table of 256 slots (63 .. 65 keys in 128): the chance that
               no two of them share a home slot is below exp(-130 * 129 / 512) < 1e-14, so linear probing chains occur
  abab         two keys alternating A B A B: groups that are no runs, and that meet again in the next wave
  straddle     runs of 48 rows, one of them over rows 56 .. 103: a group that straddles a wave boundary
  two_clouds   the same voxel keys in two clouds that meet in the middle of a wave: equal keys, different clouds, must not merge
  stale        live count 70 rows below the capacity, the rows behind it holding copies of live points
  empty_around an empty cloud before and behind the only non-empty one

No tolerance: the uint32 view of the barycentres, the segment lengths, the neighbour indices, the counts and the max count are compared
with np.array_equal against the C++ oracle (tests/preprocess_ref.py).  The public ops are driven (ops.grid_subsample, ops.CellGrid and its
query through both radius kernels)."""
import functools

import numpy as np
import pytest
import torch

from tests import preprocess_ref as PR
from tests.util import seg_of, to_dev

DL = 0.05           # voxel side; the radius grid's cells are R (1 + 1e-6): the same lattice
R = 0.05
K = 16
SIZES = (1, 63, 64, 65, 130)
PATTERNS = ('one', 'distinct', 'abab', 'straddle', 'two_clouds', 'stale', 'empty_around')
STALE_ROWS = 70


def _voxel_ids(pattern, n):
    """-> (voxel id per row, cloud lengths)."""
    a = np.arange(n)
    if pattern == 'one':
        return np.zeros(n, np.int64), [n]
    if pattern == 'distinct':
        return a, [n]
    if pattern == 'abab':
        return a % 2, [n]
    if pattern == 'straddle':
        return (a + 40) // 48, [n]
    if pattern == 'two_clouds':
        n0 = n // 2
        return np.concatenate([np.arange(n0) % 3, np.arange(n - n0) % 3]), [n0, n - n0]
    if pattern == 'stale':
        return a % 7, [n]
    if pattern == 'empty_around':
        return a % 5, [0, n, 0]
    raise ValueError(pattern)


@functools.lru_cache(maxsize=None)
def case(pattern, n):
    """-> dict(pts (n, 3) f32, lens, n_cap, rows (n_cap, 3) f32, voxels: distinct (cloud, voxel) pairs) and the oracle's results, computed
    once.  A point of voxel v lies at (v + u) DL with u in [0.2, 0.8)^3: well inside its voxel and its cell, whatever the origin."""
    rng = np.random.default_rng(1000 * PATTERNS.index(pattern) + n)
    ids, lens = _voxel_ids(pattern, n)
    lens = np.asarray(lens, np.int32)
    v = np.stack([ids % 5, (ids // 5) % 5, ids // 25], 1).astype(np.float64) - 3.0          # negative coordinates too
    pts = ((v + 0.2 + 0.6 * rng.random((n, 3))) * DL).astype(np.float32)
    n_cap = n + (STALE_ROWS if pattern == 'stale' else 0)
    rows = pts[np.arange(n_cap) % n].copy()                               # behind the live count: copies of live points
    voxels = len(set(zip(PR.cloud_ids(lens).tolist(), ids.tolist())))
    sub_p, sub_l = PR.oracle_subsample(pts, lens, DL)
    assert int(sub_l.sum()) == voxels, 'the generator did not place the voxels it names'
    idx, cnt = PR.oracle_radius(pts, pts, lens, lens, R, K)
    return dict(pts=pts, lens=lens, n_cap=n_cap, rows=rows, voxels=voxels, sub_p=sub_p, sub_l=sub_l, idx=idx, cnt=cnt)


def test_cases_hold_the_patterns_they_name():
    assert case('one', 130)['voxels'] == 1 and case('distinct', 130)['voxels'] == 130 and case('abab', 130)['voxels'] == 2
    ids, _ = _voxel_ids('straddle', 130)
    assert ids[56] == ids[103] and ids[55] != ids[56] and ids[103] != ids[104]              # one run over rows 56 .. 103
    c = case('two_clouds', 130)
    assert c['lens'].tolist() == [65, 65] and c['voxels'] == 6 and c['sub_l'].tolist() == [3, 3]     # the boundary falls inside wave 1
    assert (case('one', 130)['cnt'] > K).all() and (case('distinct', 130)['cnt'] < K).all()  # truncated rows and padded rows
    assert case('stale', 64)['n_cap'] == 64 + STALE_ROWS


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('pattern', PATTERNS)
def test_grid_subsample(pattern, n):
    from regtr_amd import ops
    c = case(pattern, n)
    out, out_seg = ops.grid_subsample(to_dev(c['rows']), seg_of(c['lens']), c['n_cap'], DL)
    seg = out_seg.cpu().numpy()
    assert np.array_equal(np.diff(seg), c['sub_l'])
    got = out[:seg[-1]].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), c['sub_p'].view(np.uint32)), 'barycentres / row order not bit exact'


@pytest.mark.gpu
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('pattern', PATTERNS)
def test_cell_grid_radius_query(pattern, n):
    from regtr_amd import ops
    c = case(pattern, n)
    xyz, seg = to_dev(c['rows']), seg_of(c['lens'])
    grid = ops.CellGrid(xyz, seg, c['n_cap'], R)
    keep = ops.SELF_QUERY_MIN_POINTS
    try:
        for min_pts, what in ((1 << 30, 'per-query kernel'), (0, 'self kernel')):
            ops.SELF_QUERY_MIN_POINTS = min_pts
            idx, cnt, mx = grid.query(xyz, seg, c['n_cap'], K, want_count=True)
            assert np.array_equal(cnt[:n].cpu().numpy(), c['cnt']), what
            assert int(mx.item()) == int(c['cnt'].max()), what
            assert np.array_equal(idx[:n].cpu().numpy(), c['idx']), f'{what}: neighbour indices not bit exact'
    finally:
        ops.SELF_QUERY_MIN_POINTS = keep
    torch.cuda.synchronize()
