"""CPU: the ICP entry points' host-side contract (exports, header, workspace sizes, refusals) and the numpy restatement itself
(tests/icp_ref.py), which is the oracle of tests/test_gpu_icp.py: it recovers a known pose, converges from a wider start, its brute-force
neighbours agree with a KD-tree, and the test clouds keep every decision clear of rounding."""
import os
import re

import numpy as np
import pytest

from tests import icp_ref as R
from tests.util import ROOT

H = 0.05                                                      # point spacing of the test clouds
GT = R.pose_of([1, 2, 3], 25.0, [0.3, -0.2, 0.5])
SUB = ([0, 1, 1], 0.25, [0.003, -0.002, 0.0015])                  # a start that moves no point by half the smallest spacing
MD = 0.0625                                                   # the edge cases' max_dist: exactly representable, and so is its square
FAKE = 0x1000                                                 # a non-NULL pointer no refused call may look at


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
    for name in ('regtr_icp_ws_bytes', 'regtr_icp_step', 'regtr_icp_chunk'):
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
        assert re.search(r'\b%s\s*\(' % name, decl), f'{name} is not declared in include/regtr_hip.h'
        assert name in table, f'{name} is missing from the mapping table of include/regtr_hip.h'
    assert re.search(r'regtr_icp_step\s+\(no reference counterpart\)', table)
    assert 'icp.hip' in build.SOURCES and build.EXTRA.get('icp.hip') == ['-ffp-contract=off']
    assert int(re.search(r'#define REGTR_ABI_VERSION (\d+)', txt).group(1)) == 11, 'new entry points do not bump the ABI version'


def test_chunk_is_exported_to_python():
    from regtr_amd import refine
    assert refine.CHUNK == _lib().lib().regtr_icp_chunk() and refine.CHUNK >= 64 and refine.CHUNK % 64 == 0


def test_workspace_grows_with_the_chunk_count():
    from regtr_amd import refine
    lib = _lib().lib()
    C = refine.CHUNK
    one = lib.regtr_icp_ws_bytes(1, C)
    assert one >= 17 * 8 and lib.regtr_icp_ws_bytes(1, 1) == one == lib.regtr_icp_ws_bytes(1, 0)
    assert lib.regtr_icp_ws_bytes(1, C + 1) >= 2 * 17 * 8
    assert lib.regtr_icp_ws_bytes(1, 40 * C) >= 40 * 17 * 8 > lib.regtr_icp_ws_bytes(1, 4 * C) >= 4 * 17 * 8
    assert lib.regtr_icp_ws_bytes(64, 40 * C) >= 64 * 40 * 17 * 8
    assert lib.regtr_icp_ws_bytes(-1, C) == 0 and lib.regtr_icp_ws_bytes(2, -5) == 0


def _step(**kw):
    """regtr_icp_step with a valid argument list (fake, never dereferenced pointers), one entry replaced at a time."""
    lib = _lib().lib()
    a = dict(src=FAKE, src_off=FAKE, n_src=1000, max_len=600, tgt_off=FAKE, n_tgt=900, B=2, max_dist=0.1, grid_radius=0.1, grid_ws=FAKE,
             grid_bytes=lib.regtr_cellgrid_ws_bytes(900, 2), pose=FAKE, it=0, stats_only=0, rf=1e-6, rr=1e-6, stats=FAKE, iters_run=FAKE,
             done=FAKE, idx=None, d2=None, ws=FAKE, ws_bytes=lib.regtr_icp_ws_bytes(2, 600), stream=None)
    a.update(kw)
    return lib.regtr_icp_step(*a.values())


def test_refusals_launch_nothing():
    """REGTR_ERR_ARG (-2) / REGTR_ERR_WORKSPACE (-3) before anything is looked at or launched (a launch on this GPU-less host, or a
    read of a fake pointer, would end differently)."""
    for bad in (dict(n_src=-1), dict(n_tgt=-1), dict(B=-1), dict(max_len=-1), dict(it=-1), dict(B=65536), dict(max_len=1001),
                dict(max_len=0), dict(src=None), dict(src_off=None), dict(tgt_off=None), dict(grid_ws=None), dict(pose=None), dict(stats=None),
                dict(iters_run=None), dict(done=None), dict(ws=None), dict(max_dist=0.0), dict(max_dist=float('nan')), dict(grid_radius=0.0),
                dict(grid_radius=0.05), dict(max_dist=0.1 * (1 + 2e-6))):
        assert _step(**bad) == -2, bad
    assert _step(ws_bytes=16) == -3 and _step(grid_bytes=1024) == -3
    # no work: REGTR_OK with nothing written, whatever the pointers
    assert _step(B=0, src=None, pose=None, ws=None, ws_bytes=0, grid_ws=None) == 0
    assert _step(n_src=0, max_len=0, src=None, stats=None, ws=None, ws_bytes=0) == 0


def test_python_refuses_cpu_tensors():
    import torch
    from regtr_amd import refine
    c = torch.zeros((5, 3))
    with pytest.raises(RuntimeError):
        refine.icp([c], [c], torch.eye(4)[None], 0.1)
    with pytest.raises(RuntimeError):
        refine.evaluate_registration([c], [c], torch.eye(4)[None, :3], 0.1)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.fixture(scope='module')
def pair():
    src, tgt, perm, noise = R.overlapping_pair(2000, H, 1, GT, extra=500)
    return src, tgt, perm, noise


def test_one_iteration_recovers_the_ground_truth_within_the_derived_bound(pair):
    src, tgt, perm, noise = pair
    p0 = R.perturbed(GT, *SUB)
    moved = np.abs(R.transform_f32(p0, src).astype(np.float64) - tgt[perm]).max()
    assert moved < 0.5 * (1 - 2 * 0.3) * H, 'the start moves no point by half the smallest spacing'
    o = R.icp(src, tgt, p0, 2 * H, iters=1, margins=True)
    assert o['iters_run'] == 1 and o['n_inliers'] == 2000 and np.array_equal(o['history'][0]['idx'], perm) and np.array_equal(o['idx'], perm)
    b_gt, b_fit = R.pose_bound(o['last_m'], o['last_sol'], noise), R.pose_bound(o['last_m'], o['last_sol'])
    assert np.all(np.abs(o['pose64'] - GT) <= b_gt) and np.all(np.abs(o['pose'].astype(np.float64) - GT) <= b_gt)
    # the bound itself: one float32 rounding of each entry plus a small conditioning term
    assert np.all(b_fit[:, :3] < 2.0 ** -24 * 1.01) and np.all(b_fit[:, 3] < 2.0 ** -24 * 1.01 * np.abs(GT[:, 3]) + 1e-11)
    assert np.all(np.abs(o['pose'].astype(np.float64) - o['pose64']) <= b_fit)
    assert min(r['gap2'] for r in o['history']) > R.match_margin_needed(src, p0, 2 * H)
    assert min(r['gap_r'] for r in o['history']) > R.match_margin_needed(src, p0, 2 * H)
    rot, trans = R.pose_errors(o['pose'], GT)
    assert trans <= np.linalg.norm(b_gt[:, 3]) and np.radians(rot) <= 2 * np.linalg.norm(b_gt[:, :3]) + 2.0 ** -11.5      # (arccos near 1)


WIDE = dict(n=600, seed=1, extra=150, max_dist=1.0 * H, axis=[1, 0, 1], deg=6.0, dt=np.array([0.6, -0.5, 0.4]) * 0.8 * H)


def wide_case():
    src, tgt, perm, noise = R.overlapping_pair(WIDE['n'], H, WIDE['seed'], GT, extra=WIDE['extra'])
    return src, tgt, R.perturbed(GT, WIDE['axis'], WIDE['deg'], WIDE['dt']), WIDE['max_dist']


def test_a_wider_start_converges_with_fitness_never_falling():
    src, tgt, p0, md = wide_case()
    o = R.icp(src, tgt, p0, md, iters=30, margins=True)
    fit = [r['fitness'] for r in o['history']]
    assert 4 <= o['iters_run'] < 30 and o['done'], 'several iterations, then the stop rule'
    assert all(b >= a for a, b in zip(fit, fit[1:])) and fit[0] < 0.97 and fit[-1] == 1.0
    rot, trans = R.pose_errors(o['pose'], GT)
    assert rot < 0.01 and trans < 1e-6
    # every decision of the run is clear of rounding: a one-ulp difference in a pose entry moves no match, no inlier and no stop
    need = R.match_margin_needed(src, p0, md)
    assert min(r['gap2'] for r in o['history']) > need and min(r['gap_r'] for r in o['history']) > need
    assert min(min(r['stop_margin']) for r in o['history'] if 'stop_margin' in r) > 1e-8


def length_batch():
    from regtr_amd import refine
    C = refine.CHUNK
    lens = [1, 2, 3, 255, 256, 257, C - 1, C, C + 1, 2 * C + 5]
    srcs, tgts, poses, gts = [], [], [], []
    for k, n in enumerate(lens):
        gt = R.pose_of([1 + k, 2, 3 - k], 10.0 + 7 * k, [0.3 - 0.1 * k, -0.2, 0.05 * k])
        s, t, _, _ = R.overlapping_pair(n, H, 100 + k, gt, extra=17 + 5 * k)
        srcs.append(s); tgts.append(t); gts.append(gt)
        poses.append(R.perturbed(gt, [k % 3 == 0, 1, k % 2], 0.2, [0.002, -0.001 * (k % 3), 0.0015]))
    return lens, srcs, tgts, poses



def edge_batch():
    gt = R.pose_of([0, 0, 1], 20.0, [0.1, 0.2, -0.1])
    s0, t0, _, _ = R.overlapping_pair(300, H, 11, gt, extra=40)
    s7, t7, _, _ = R.overlapping_pair(260, H, 12, gt, extra=9)
    I = np.eye(4)[:3]
    e = np.zeros((0, 3), np.float32)
    # pair 4: identity pose; targets: an isolated one, a coincident couple, a cluster
    t4 = np.array([[10, 3, 0], [20, 0, 4], [20, 0, 4], [30, 0, 0], [30.01, 0, 0], [30, 0.01, 0], [30, 0, 0.01]], np.float32)
    s4 = np.array([[10 + MD, 3, 0],             # exactly at max_dist of target 0: strict <, no inlier
                   [10 + MD - 2.0 ** -10, 3, 0],   # just inside
                   [20.01, 0, 4],               # two coincident targets: the lower index wins
                   [30.3, 0, 0],                # inside the targets' box, all 27 cells empty
                   [1e4, -1e4, 1e4],            # far outside
                   [30.002, 0.001, 0], [30.009, 0, 0], [30, 0.009, 0.001], [30.001, 0.001, 0.0085]], np.float32)
    t5 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    s5 = np.array([[0.01, 0, 0], [1, 0.01, 0], [5, 5, 5]], np.float32)                      # two matches only
    line = np.stack([np.linspace(0, 1, 9), np.zeros(9), np.zeros(9)], 1).astype(np.float32)   # collinear matches
    srcs = [s0, e, s7[:50], e, s4, s5, line + np.float32(0.001), s7]
    tgts = [t0, t7, e, e, t4, t5, line, t7]
    p_sub = R.perturbed(gt, *SUB)
    poses = [p_sub, p_sub, p_sub, p_sub, I, I, I, p_sub]
    mds = MD
    return srcs, tgts, poses, mds



def test_the_gpu_suites_batches_keep_their_decisions_clear_of_rounding():
    """tests/test_gpu_icp.py compares matches and counts EXACTLY: on its batches no match, no inlier decision and no stop may hang on
    the last bit of a pose.  The deliberate exact cases (a target exactly at max_dist, coincident targets) sit in the first pass of an
    identity pose, whose transform is exact, and are resolved by the stated rules."""
    lens, srcs, tgts, poses = length_batch()
    for b in range(len(lens)):
        o = R.icp(srcs[b], tgts[b], poses[b], 1.2 * H, iters=6, margins=True)
        need = R.match_margin_needed(srcs[b], poses[b], 1.2 * H)
        assert min(r['gap2'] for r in o['history']) > need and min(r['gap_r'] for r in o['history']) > need, (b, lens[b])
        assert all(min(r['stop_margin']) > 1e-8 for r in o['history'] if 'stop_margin' in r), (b, lens[b])
    srcs, tgts, poses, md = edge_batch()
    for b in range(len(srcs)):
        o = R.icp(srcs[b], tgts[b], poses[b], md, iters=3, margins=True)
        need = R.match_margin_needed(srcs[b][np.abs(srcs[b]).max(1) < 100] if len(srcs[b]) else srcs[b], poses[b], md)
        for k, r in enumerate(o['history']):
            if b == 4 and k == 0:
                assert r['gap2'] == 0.0 and r['gap_r'] == 0.0, 'the deliberate tie and the exact radius'
            elif b == 4:          # (the coincident couple ties in every pass, whatever the pose: two identical d2, the lower index)
                assert r['gap2'] == 0.0 and r['gap_r'] > need, (k, r['gap_r'], need)
            elif len(srcs[b]) and len(tgts[b]):
                assert r['gap2'] > need and r['gap_r'] > need, (b, k, r['gap2'], r['gap_r'], need)
            assert min(r.get('stop_margin', (1,))) > 1e-8, (b, k)


def test_the_wide_case_restarted_at_its_result_stops_after_one_update():
    src, tgt, p0, md = wide_case()
    ref = R.icp(src, tgt, p0, md, iters=30)
    again = R.icp(src, tgt, ref['pose'], md, iters=30, margins=True)
    assert again['iters_run'] == 1 and again['done'] and min(again['history'][1]['stop_margin']) > 1e-8


def test_brute_force_neighbours_agree_with_a_kd_tree(pair):
    from scipy.spatial import cKDTree
    src, tgt, _, _ = pair
    y = R.transform_f32(R.perturbed(GT, [1, 0, 0], 2.0, [0.02, 0.0, -0.01]), src)
    idx, d2, gap2, gap_r = R.nearest(y, tgt, 0.8 * H, margins=True)
    assert gap2.min() > 1e-12 and gap_r.min() > 1e-12, 'tie-free data'
    dist, j = cKDTree(tgt.astype(np.float64)).query(y.astype(np.float64), k=1, distance_upper_bound=0.8 * H)
    want = np.where(np.isfinite(dist), j, -1)
    assert np.array_equal(idx, want) and 0 < (idx < 0).sum() < len(idx)
    assert np.allclose(np.sqrt(d2[idx >= 0]), dist[idx >= 0], rtol=1e-12, atol=0)


def test_ties_and_the_exact_radius_follow_the_stated_rules():
    tgt = np.array([[1, 0, 0], [0.5, 0, 0], [0.5, 0, 0], [-0.5, 0, 0], [0, 2, 0]], dtype=np.float32)
    q = np.array([[0, 0, 0], [0, 1, 0], [9, 9, 9]], dtype=np.float32)
    idx, d2 = R.nearest(q, tgt, 1.0)
    assert idx.tolist() == [1, -1, -1] and d2[0] == 0.25 and np.isinf(d2[1:]).all()      # lowest index of three at 0.5; d == max_dist is out
    idx, _ = R.nearest(q, tgt, np.nextafter(1.0, 2.0))
    assert idx.tolist() == [1, 4, -1]


def test_stop_rule_and_degenerate_inputs():
    src, tgt, _, _ = R.overlapping_pair(300, H, 3, GT)
    fixed = R.icp(src, tgt, GT, 0.5 * H, iters=30)
    assert fixed['iters_run'] == 1 and fixed['done'] and len(fixed['history']) == 2
    again = R.icp(src, tgt, fixed['pose'], 0.5 * H, iters=30)
    assert again['iters_run'] == 1 and np.array_equal(again['pose'], fixed['pose'])
    two = R.icp(src[:2], tgt, GT, 0.5 * H, iters=5)
    assert two['iters_run'] == 0 and two['done'] and two['n_inliers'] == 2 and np.array_equal(two['pose'], GT.astype(np.float32))
    line = np.stack([np.linspace(0, 1, 9), np.zeros(9), np.zeros(9)], 1).astype(np.float32)
    col = R.icp(line, line, np.eye(4)[:3], 0.01, iters=5)
    assert col['iters_run'] == 0 and col['done'] and col['n_inliers'] == 9
    nan = GT.copy()
    nan[1, 2] = np.nan
    bad = R.icp(src, tgt, nan, 0.5 * H, iters=5)
    assert bad['iters_run'] == 0 and bad['done'] and bad['n_inliers'] == 0 and bad['fitness'] == 0.0
    ev = R.icp(src, tgt, GT, 0.5 * H, iters=0)
    assert ev['iters_run'] == 0 and not ev['done'] and ev['n_inliers'] == 300 and ev['fitness'] == 1.0 and ev['inlier_rmse'] < 1e-6
    empty = R.icp(np.zeros((0, 3), np.float32), tgt, GT, 0.5 * H, iters=3)
    assert empty['n_inliers'] == 0 and empty['fitness'] == 0.0 and empty['inlier_rmse'] == 0.0 and empty['done']
