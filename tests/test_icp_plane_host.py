"""CPU: the host-side contract of regtr_estimate_normals / regtr_icp_plane_step (exports, header, refusals) and the numpy restatement
tests/icp_plane_ref.py itself, the oracle of tests/test_gpu_icp_plane.py: its normals against np.cov + eigh on unquantised doubles, its
6 x 6 step against a least-squares solve of the stacked Jacobian, and its loop on the synthetic room the feature was proposed on."""
import os
import re
import sys

import numpy as np
import pytest

from tests import icp_plane_ref as P
from tests import icp_ref as R
from tests.util import ROOT

FAKE = 0x1000                                                 # a non-NULL, 4096-aligned pointer no refused call may look at
GT = R.pose_of([1, 2, 3], 25.0, [0.3, -0.2, 0.5])
NR = 0.0625                                                   # the normal cases' radius: a power of two, so lattice differences quantise exactly


def _lib():
    from regtr_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_exported_declared_and_bound():
    from regtr_amd import build
    L = _lib()
    txt = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    table = txt[:txt.index('#ifndef REGTR_HIP_H')]
    decl = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name in ('regtr_estimate_normals', 'regtr_icp_plane_step'):
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
        assert re.search(r'\b%s\s*\(' % name, decl), f'{name} is not declared in include/regtr_hip.h'
        assert re.search(r'%s\s+\(no reference counterpart\)' % name, table), f'{name} is missing from the mapping table'
    assert 'icp_plane.hip' in build.SOURCES and build.EXTRA.get('icp_plane.hip') == ['-ffp-contract=off']
    assert not [n for n in L.SIGNATURES if 'plane' in n and n.endswith('_bytes')], 'the launcher has no size query: its arrays are the caller\'s'


def _normals(**kw):
    lib = _lib().lib()
    a = dict(xyz=FAKE, off=FAKE, n=900, C=2, radius=0.1, grid_radius=0.1, grid_ws=FAKE, grid_bytes=lib.regtr_cellgrid_ws_bytes(900, 2),
             normals=FAKE, valid=FAKE, moments=None, stream=None)
    a.update(kw)
    return lib.regtr_estimate_normals(*a.values())


def _step(**kw):
    lib = _lib().lib()
    a = dict(src=FAKE, src_off=FAKE, n_src=1000, max_len=600, nrm=FAKE, nvalid=FAKE, tgt_off=FAKE, n_tgt=900, B=2, max_dist=0.1,
             grid_radius=0.1, grid_ws=FAKE, grid_bytes=lib.regtr_cellgrid_ws_bytes(900, 2), pose=FAKE, pose64=FAKE, it=0, stats_only=0,
             rf=1e-6, rr=1e-6, stats=FAKE, iters_run=FAKE, done=FAKE, idx=None, partial=FAKE, stream=None)
    a.update(kw)
    return lib.regtr_icp_plane_step(*a.values())


def test_refusals_launch_nothing():
    """REGTR_ERR_ARG (-2) / REGTR_ERR_WORKSPACE (-3) before anything is looked at or launched (a launch on a GPU-less host, or a read of
    a fake pointer, would end differently)."""
    for bad in (dict(n=-1), dict(C=0), dict(C=-3), dict(radius=0.0), dict(radius=-1.0), dict(radius=float('nan')), dict(grid_radius=0.0),
                dict(grid_radius=0.05), dict(off=None), dict(grid_ws=None), dict(xyz=None), dict(normals=None), dict(valid=None),
                dict(xyz=FAKE + 2), dict(off=FAKE + 1), dict(normals=FAKE + 3), dict(valid=FAKE + 2), dict(moments=FAKE + 4),
                dict(grid_ws=FAKE + 8)):
        assert _normals(**bad) == -2, bad
    assert _normals(grid_bytes=1024) == -3
    assert _normals(n=0, xyz=None, normals=None, valid=None) == 0, 'no row: REGTR_OK, nothing launched'
    for bad in (dict(n_src=-1), dict(n_tgt=-1), dict(B=0), dict(B=-1), dict(B=65536), dict(max_len=-1), dict(max_len=1001), dict(max_len=0),
                dict(it=-1), dict(max_dist=0.0), dict(max_dist=-0.1), dict(max_dist=float('nan')), dict(grid_radius=0.0), dict(grid_radius=0.05),
                dict(src=None), dict(src_off=None), dict(nrm=None), dict(nvalid=None), dict(tgt_off=None), dict(grid_ws=None), dict(pose=None),
                dict(pose64=None), dict(stats=None), dict(iters_run=None), dict(done=None), dict(partial=None),
                dict(src=FAKE + 1), dict(src_off=FAKE + 2), dict(nrm=FAKE + 2), dict(nvalid=FAKE + 1), dict(tgt_off=FAKE + 3), dict(grid_ws=FAKE + 4),
                dict(pose=FAKE + 2), dict(pose64=FAKE + 4), dict(stats=FAKE + 4), dict(iters_run=FAKE + 2), dict(done=FAKE + 1), dict(idx=FAKE + 2),
                dict(partial=FAKE + 4)):
        assert _step(**bad) == -2, bad
    assert _step(grid_bytes=1024) == -3
    assert _step(n_src=0, max_len=0, src=None) == 0, 'no source row: REGTR_OK, nothing launched'


def test_python_refuses_unknown_methods_and_cpu_tensors():
    import torch
    from regtr_amd import refine
    c = torch.zeros((5, 3))
    with pytest.raises(ValueError, match='method'):
        refine.icp([c], [c], torch.eye(4)[None], 0.1, method='point_to_line')
    with pytest.raises(RuntimeError):
        refine.icp([c], [c], torch.eye(4)[None], 0.1, method='point_to_plane')
    with pytest.raises(RuntimeError):
        refine.estimate_normals([c], 0.1)
    assert refine.METHODS == ('point_to_point', 'point_to_plane')


# ------------------------------------------------------------------------------------------------ the restatement: normals
def test_the_quantisation_scale():
    for radius in (0.05, 0.0625, 0.125, 1.0, 3.7, 1e-3):
        s = P.qscale(radius)
        assert np.log2(s) == np.round(np.log2(s)) and radius * s <= 2.0 ** 20 < radius * s * 2


def normal_clouds():
    """The clouds of the normals test, lengths [1, 2, 3, 40, 257, 1500] (tests/test_gpu_icp_plane.py runs them in one call, with
    radius NR).  Coordinates of the exact cases are multiples of 2^-10: their differences quantise without rounding."""
    rng = np.random.RandomState(4)
    u = 2.0 ** -10
    c1 = np.array([[0.5, 0.25, -1.0]])                                              # isolated: invalid
    c2 = np.array([[1.0, 1.0, 1.0], [1.0 + 8 * u, 1.0, 1.0]])                         # two neighbours: invalid
    c3 = np.array([[0.0, 0.0, 0.0], [16 * u, 0.0, 0.0], [0.0, 24 * u, 0.0]])          # the smallest valid neighbourhood
    # 40: exactly collinear (10), duplicated points of a small triangle (9), the same nine shifted by 100 m (9), an exact radius case (4),
    #     far-apart isolated points (8)
    line = np.stack([np.arange(10) * 12 * u, np.zeros(10), np.full(10, 2.0)], 1)
    tri = np.array([[5.0, 5.0, 5.0], [5.0 + 20 * u, 5.0, 5.0 + 4 * u], [5.0, 5.0 + 28 * u, 5.0 - 8 * u]])
    dup = np.concatenate([tri, tri, tri])
    edge = np.array([[9.0, 0.0, 0.0], [9.0 + NR, 0.0, 0.0], [9.0, 32 * u, 0.0], [9.0 + 16 * u, 16 * u, 8 * u]])     # row 1 exactly at radius of row 0
    iso = np.stack([20.0 + np.arange(8) * 1.0, np.zeros(8), np.zeros(8)], 1)
    c40 = np.concatenate([line, dup, dup + np.array([100.0, 0.0, 0.0]), edge, iso])
    # 257: an exact z = 0 lattice of 16 x 16 points, spacing 16 u (radius 64 u: two rings of neighbours), and one point far away
    g = np.arange(16) * 16 * u
    lat = np.stack(np.meshgrid(g, g, indexing='ij'), -1).reshape(-1, 2)
    c257 = np.concatenate([np.concatenate([lat, np.zeros((256, 1))], 1), [[50.0, 50.0, 50.0]]])
    # 1500: a tilted plane with float32-rounded coordinates (700), a sphere patch (700), and 100 of the tilted plane's points again: the
    #       same space as cloud 257's lattice is occupied by part of it, and the two must not mix
    ab = rng.uniform(0, 0.5, size=(700, 2))
    tilt = np.array([0.3, -0.2, 0.1]) + ab[:, :1] * np.array([0.8, 0.0, 0.6]) + ab[:, 1:] * np.array([0.0, 1.0, 0.0])
    th, ph = rng.uniform(0.2, 0.7, 700), rng.uniform(0.0, 0.6, 700)
    sph = np.array([3.0, 0.0, 0.0]) + 0.8 * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], 1)
    over = np.concatenate([lat[:100] + 4 * u, np.full((100, 1), 4 * u)], 1)      # inside the lattice cloud's space, another cloud
    c1500 = np.concatenate([tilt, sph, over])
    clouds = [np.asarray(c, dtype=np.float32) for c in (c1, c2, c3, c40, c257, c1500)]
    assert [len(c) for c in clouds] == [1, 2, 3, 40, 257, 1500]
    return clouds


@pytest.fixture(scope='module')
def normal_refs():
    clouds = normal_clouds()
    return clouds, [P.normals(c, NR) for c in clouds]


def test_the_normal_cases_are_what_they_claim(normal_refs):
    clouds, refs = normal_refs
    v = [r['valid'] for r in refs]
    assert not v[0].any() and not v[1].any() and v[2].all()
    assert not v[3][:10].any(), 'exactly collinear: invalid'
    assert v[3][10:28].all() and np.all(refs[3]['moments'][10:28, 0] == 9), 'duplicates count, and the 100 m copy sees its own nine only'
    assert np.array_equal(refs[3]['moments'][10:19], refs[3]['moments'][19:28]), 'a shift by 100 m changes no moment'
    assert refs[3]['moments'][28, 0] == 3 and refs[3]['moments'][29, 0] == 2, 'a neighbour exactly at the radius is outside (strict <)'
    assert not v[3][32:].any() and np.all(refs[3]['moments'][32:, 0] == 1)
    assert v[4][:256].all() and not v[4][256]
    n = refs[4]['normals'][:256]
    assert np.all(n[:, :2] == 0) and np.all(np.abs(n[:, 2]) == 1), 'an exact z = 0 lattice: the normal is exactly (0, 0, +-1)'
    assert np.all(refs[4]['moments'][:256, 0] >= 9) and refs[5]['moments'][1400:, 0].max() <= 100, 'two clouds in one space do not mix'
    # no decision near its threshold, and few rows with a small eigen-gap
    for r in refs:
        lam, m = r['lam'], r['moments']
        ratio = lam[:, 1] / np.maximum(lam[:, 2], 1e-300)
        assert not np.any((m[:, 0] >= 3) & (ratio > 2.0 ** -41) & (ratio < 2.0 ** -39))
        ok = r['valid'] != 0
        assert np.mean((lam[ok, 1] - lam[ok, 0]) < 1e-6 * lam[ok, 2]) <= 0.01 if ok.any() else True


def test_normals_agree_with_cov_and_eigh_on_unquantised_doubles(normal_refs):
    clouds, refs = normal_refs
    worst = 0.0
    for c, r in zip(clouds, refs):
        p = c.astype(np.float64)
        nb = P.neighbours(c, NR)
        for i in np.nonzero(r['valid'])[0]:
            C = np.cov(p[nb[i]].T, bias=True)
            lam, vec = np.linalg.eigh(C)
            if lam[1] - lam[0] < 1e-3 * lam[2]:
                continue
            ang = float(P.angle(vec[:, 0], r['normals'][i]))
            bound = P.quantisation_angle_bound(r['lam'][i:i + 1], NR)[0] + P.normal_angle_bound(r['lam'][i:i + 1])[0]
            worst = max(worst, ang / bound)
            assert ang <= bound, (i, ang, bound)
    assert 0 < worst <= 1


# ------------------------------------------------------------------------------------------------ the restatement: one step
@pytest.fixture(scope='module')
def corner():
    src, tgt, perm, noise = P.box_corner(17, 0.02, 5, GT)
    return src, tgt, perm, noise, P.normals(tgt, 0.05)


CORNER_START = ([1, -1, 2], 1.0, [0.012, -0.012, 0.011])      # 1 degree / 2 cm
CORNER_MD = 0.05


def test_the_step_is_the_least_squares_solution_of_the_stacked_jacobian(corner):
    src, tgt, perm, noise, N = corner
    p0 = R.perturbed(GT, *CORNER_START).astype(np.float32)
    y = R.transform_f32(p0, src)
    idx, d2 = R.nearest(y, tgt, CORNER_MD)
    s = P.plane_sums(y, tgt, idx, d2, N['normals'], N['valid'])
    sol = P.plane_solve(s)
    assert not sol['stop'] and s['n_sys'] == s['n'] == len(src)
    Y, q, n = y.astype(np.float64), tgt.astype(np.float64)[idx], N['normals'].astype(np.float64)[idx]
    J = np.concatenate([np.cross(Y, n), n], axis=1)
    r = np.einsum('ij,ij->i', n, Y - q)
    x = np.linalg.lstsq(J, -r, rcond=None)[0]
    assert np.allclose(sol['x'], x, rtol=0, atol=1e-9 * np.abs(x).max() / sol['lmin'] * 1e-4), np.abs(sol['x'] - x).max()
    dT = P.delta(x)
    assert np.allclose(dT[:, :3] @ dT[:, :3].T, np.eye(3), atol=1e-15) and np.linalg.det(dT[:, :3]) > 0
    small = P.delta(np.array([1e-8, 0, 0, 0, 0, 0]))
    assert abs(small[2, 1] - 1e-8) < 1e-20 and abs(small[1, 2] + 1e-8) < 1e-20, 'x0 turns about the x axis'


def walls():
    """An axis-aligned wall (J^T J has zero diagonal entries) and a tilted one (a full diagonal: the LDL^T meets the small pivot)."""
    return [P.plane_patch(12, 12, 0.02, 3, (0, 0, 0.5), (1, 0, 0), (0, 1, 0)).astype(np.float32),
            P.plane_patch(12, 12, 0.02, 4, (0.1, 0.2, 0.5), (0.8, 0, 0.6), (0, 1, 0)).astype(np.float32)]


def test_a_single_wall_is_degenerate_and_too_few_rows_stop():
    for k, wall in enumerate(walls()):
        N = P.normals(wall, 0.05)
        assert N['valid'].all()
        o = P.icp_plane(wall, wall, np.eye(4)[:3], 0.05, N['normals'], N['valid'], iters=5)
        assert o['iters_run'] == 0 and o['done'] and o['n_inliers'] == len(wall) and o['history'][0]['n_sys'] == len(wall)
        piv = o['history'][0]['pivot_min']
        assert piv is None if k == 0 else piv < 2.0 ** -30, 'a zero diagonal entry; a pivot far below the threshold'
    few = P.icp_plane(wall[:5], wall, np.eye(4)[:3], 0.05, N['normals'], N['valid'], iters=5)
    assert few['iters_run'] == 0 and few['done'] and few['n_inliers'] == 5
    none = P.icp_plane(wall, wall, np.eye(4)[:3], 0.05, N['normals'], np.zeros_like(N['valid']), iters=5)
    assert none['iters_run'] == 0 and none['done'] and none['n_inliers'] == len(wall) and none['history'][0]['n_sys'] == 0


def test_the_box_corner_recovers_the_ground_truth_faster_than_point_to_point(corner):
    src, tgt, perm, noise, N = corner
    p0 = R.perturbed(GT, *CORNER_START)
    o = P.icp_plane(src, tgt, p0, CORNER_MD, N['normals'], N['valid'], iters=30)
    pp = R.icp(src, tgt, p0, CORNER_MD, iters=30)
    assert o['done'] and 2 <= o['iters_run'] <= pp['iters_run'] and np.array_equal(o['idx'], perm)
    dy = 4 * 2.0 ** -24 * (np.abs(src).sum(1).max() + np.abs(GT[:, 3]).max())
    b = P.step_bound(o['last_s'], o['last_sol'], o['last_prev'], o['pose64'], target_noise=noise, dy=dy)
    assert np.all(np.abs(o['pose'].astype(np.float64) - GT) <= b) and b.max() < 1e-3


# ------------------------------------------------------------------------------------------------ the restatement: the room
def test_the_room_converges_to_one_fixed_point_from_three_starts():
    """The case the feature was proposed on: synth_pair(1, 20000), max_dist 0.05, normals from all neighbours within 0.05 m, three
    seeded starts 1.5 degrees / 5 cm off (tools/icp_bench.py's perturb, consecutive draws of default_rng(0): the proposal does not name
    its seeds, so its counts of 9 / 8 / 9 cannot be re-drawn; these starts take 7 / 6 / 7 pose updates).  Every start stops within the
    proposal's nine iterations at one fixed point, 0.074 degrees / 2.0 mm from the ground truth, and is within 0.09 degrees / 2.5 mm
    after five."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        from icp_bench import perturb
    finally:
        sys.path.pop(0)
    from regtr_amd.synthetic import synth_pair
    src, tgt, gt = synth_pair(1, 20000, return_pose=True)
    gt = gt.astype(np.float64)
    N = P.normals(tgt, 0.05)
    cnt, lam = N['moments'][:, 0], N['lam']
    assert cnt.min() == 3 and cnt.max() == 34 and np.median(cnt) == 21 and N['valid'].all()
    assert abs(np.percentile((lam[:, 1] - lam[:, 0]) / lam[:, 2], 1) - 0.09) < 0.005
    rng = np.random.default_rng(0)
    ends = []
    for k in range(3):
        p0 = perturb(gt, rng)
        o = P.icp_plane(src, tgt, p0, 0.05, N['normals'], N['valid'], iters=30, nearest=P.kd_nearest)
        five = P.icp_plane(src, tgt, p0, 0.05, N['normals'], N['valid'], iters=5, nearest=P.kd_nearest)
        rot, trans = R.pose_errors(o['pose'], gt)
        r5, t5 = R.pose_errors(five['pose'], gt)
        assert o['done'] and o['iters_run'] <= 9, (k, o['iters_run'])
        assert abs(rot - 0.074) < 0.003 and abs(trans - 0.0020) < 0.0001, (k, rot, trans)
        assert r5 <= 0.09 and t5 <= 0.0025, (k, r5, t5)
        ends.append(o['pose'].astype(np.float64))
    for e in ends[1:]:
        rot, trans = R.pose_errors(e, ends[0])
        print(f'between two ends: {rot:.4f} deg, {trans * 1e3:.3f} mm')
        # (the stop rule ends each run a little short of the fixed point: the ends are a quarter of their distance to the ground truth
        #  apart at most, where point to point's ends were 0.035 .. 0.217 degrees / 1.8 .. 8.4 mm off it)
        assert rot < 0.074 / 4 and trans < 0.0020 / 4, 'one fixed point from all three starts'


# ------------------------------------------------------------------------------------------------ the GPU suite's batches
STEP_LENS = [255, 256, 257, 1, 700]
STEP_MD = 0.05


def step_batch():
    """Pairs with source lengths STEP_LENS for tests/test_gpu_icp_plane.py: rows of a box corner against all its images; pair 1 has an
    empty target, pair 2 targets whose normals are all invalid (zero).  -> srcs, tgts, poses, normals, valids (per target cloud)."""
    srcs, tgts, poses, nrms, valids = [], [], [], [], []
    for k, n in enumerate(STEP_LENS):
        gt = R.pose_of([1 + k, 2, 3 - k], 10.0 + 7 * k, [0.3 - 0.1 * k, -0.2, 0.05 * k])
        s, t, _, _ = P.box_corner(16, 0.02, 20 + k, gt)
        rows = np.sort(np.random.RandomState(40 + k).permutation(len(s))[:n])
        if k == 1:
            t = np.zeros((0, 3), np.float32)
        N = P.normals(t, 0.05) if len(t) else {'normals': np.zeros((0, 3), np.float32), 'valid': np.zeros(0, np.int32)}
        if k == 2:
            N = {'normals': np.zeros_like(N['normals']), 'valid': np.zeros_like(N['valid'])}
        srcs.append(s[rows]); tgts.append(t); nrms.append(N['normals']); valids.append(N['valid'])
        poses.append(R.perturbed(gt, [k % 3 == 0, 1, k % 2], 0.3, [0.003, -0.002 * (k % 3), 0.0025]).astype(np.float32))
    return srcs, tgts, poses, nrms, valids


def room_crop():
    """3000 source points of synth_pair(1) around the middle of the overlap, the target points of the same region, the ground truth and
    three starts 1.5 degrees / 5 cm off it (tools/icp_bench.py's perturb)."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        from icp_bench import perturb
    finally:
        sys.path.pop(0)
    from scipy.spatial import cKDTree
    from regtr_amd.synthetic import synth_pair
    src, tgt, gt = synth_pair(1, 20000, return_pose=True)
    gt = gt.astype(np.float64)
    img = src.astype(np.float64) @ gt[:, :3].T + gt[:, 3]
    d, _ = cKDTree(tgt).query(img)
    c = np.median(img[d < 0.02], 0)
    rows = np.sort(np.argsort(np.linalg.norm(img - c, axis=1))[:3000])
    rad = np.linalg.norm(img[rows] - c, axis=1).max()
    t3 = tgt[np.linalg.norm(tgt.astype(np.float64) - c, axis=1) < rad + 0.1]
    rng = np.random.default_rng(0)
    return src[rows], t3, gt, [perturb(gt, rng) for _ in range(3)]


def test_the_gpu_suites_step_batch_is_what_it_claims():
    srcs, tgts, poses, nrms, valids = step_batch()
    assert [len(s) for s in srcs] == STEP_LENS and len(tgts[1]) == 0 and not valids[2].any() and valids[0].all() and valids[4].all()
    for b in (0, 4):
        o = P.icp_plane(srcs[b], tgts[b], poses[b], STEP_MD, nrms[b], valids[b], iters=1)
        assert o['iters_run'] == 1 and o['n_inliers'] == len(srcs[b]) and o['last_sol']['lmin'] > 1e-4
    for b in (1, 2, 3):
        o = P.icp_plane(srcs[b], tgts[b], poses[b], STEP_MD, nrms[b], valids[b], iters=1)
        assert o['iters_run'] == 0 and o['done'] and o['n_inliers'] == (0 if b == 1 else len(srcs[b]))
