"""GPU (-m gpu): regtr_amd.refine (csrc/icp.hip) against the numpy restatement tests/icp_ref.py and against the project's own operators
(ops.se3_transform + overlap.nearest_in_radius; the composed route of refine.use_fused_icp(False)).

Matches, distances and counts are compared exactly; poses within the bound icp_ref.pose_bound derives from the restatement's own
singular values (about one float32 rounding per entry).  tests/test_icp_host.py checks on the CPU that the clouds used here keep every
decision -- best against second-best match, inside against outside max_dist, stop against go on -- clear of rounding."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import icp_ref as R
from tests.test_icp_host import GT, H, MD, SUB, edge_batch, length_batch, wide_case
from tests.util import ROOT, load_cfg, seeded_sd

pytestmark = pytest.mark.gpu

SENT = -7


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


def _clouds(arrs):
    return [_dev(np.asarray(a, dtype=np.float32).reshape(-1, 3)) for a in arrs]


def _poses(ps):
    return _dev(np.stack([np.asarray(p, dtype=np.float32)[:3] for p in ps]))


def _icp(srcs, tgts, poses, md, **kw):
    from regtr_amd import refine
    return refine.icp(_clouds(srcs), _clouds(tgts), _poses(poses), md, **kw)


def _off(arrs):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)


class Direct:
    """regtr_icp_step called directly over buffers with sentinel margins around pose, stats, idx, d2, iters_run and done."""

    PAD = 16

    def __init__(self, srcs, tgts, poses, md):
        from regtr_amd import _lib, ops
        self.L, self._lib = _lib.lib(), _lib
        self.B = len(srcs)
        self.src = _dev(np.concatenate([np.asarray(s, np.float32).reshape(-1, 3) for s in srcs]))
        self.tgt = _dev(np.concatenate([np.asarray(t, np.float32).reshape(-1, 3) for t in tgts]))
        self.s_off, self.t_off = _dev(_off(srcs).astype(np.int32)), _dev(_off(tgts).astype(np.int32))
        self.max_len = max(len(s) for s in srcs)
        self.md, self.r32 = float(md), float(np.float32(md))
        self.grid = ops.CellGrid(self.tgt, self.t_off, self.tgt.shape[0], self.r32)
        n, B, P = self.src.shape[0], self.B, self.PAD
        self.buf = {'pose': torch.full((B * 12 + 2 * P,), float(SENT), dtype=torch.float32, device='cuda'),
                    'stats': torch.full((B * 3 + 2 * P,), float(SENT), dtype=torch.float64, device='cuda'),
                    'idx': torch.full((n + 2 * P,), SENT, dtype=torch.int32, device='cuda'),
                    'd2': torch.full((n + 2 * P,), float(SENT), dtype=torch.float64, device='cuda'),
                    'iters_run': torch.full((B + 2 * P,), SENT, dtype=torch.int32, device='cuda'),
                    'done': torch.full((B + 2 * P,), SENT, dtype=torch.int32, device='cuda')}
        self.view = {k: v[P:v.numel() - P] for k, v in self.buf.items()}
        self.view['pose'].copy_(_poses(poses).reshape(-1))
        self.nb = self.L.regtr_icp_ws_bytes(B, self.max_len)
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device='cuda')

    def step(self, it, stats_only=False, rel=1e-6):
        v, p = self.view, lambda t: t.data_ptr()
        self._lib.check(self.L.regtr_icp_step(p(self.src), p(self.s_off), self.src.shape[0], self.max_len, p(self.t_off), self.tgt.shape[0],
                                              self.B, self.md, self.r32, p(self.grid.ws), self.grid.nbytes, p(v['pose']), it, int(stats_only),
                                              rel, rel, p(v['stats']), p(v['iters_run']), p(v['done']), p(v['idx']), p(v['d2']), p(self.ws),
                                              self.nb, None), 'regtr_icp_step')
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().copy() for k, t in v.items()}

    def margins_untouched(self):
        P = self.PAD
        return all(bool((b[:P] == SENT).all()) and bool((b[-P:] == SENT).all()) for b in self.buf.values())


def _check_pair(res, b, ref, src_off, tgt_off, what=''):
    """One pair of a device result against its restatement: counts and matches exact, stats to float64 summation accuracy, the pose
    within the derived bound (bit-equal to the start where the restatement never updates).  -> worst err / bound."""
    assert int(res.n_inliers[b]) == ref['n_inliers'], f'{what} pair {b}: n_inliers'
    assert int(res.iters_run[b]) == ref['iters_run'], f'{what} pair {b}: iters_run {int(res.iters_run[b])} != {ref["iters_run"]}'
    assert float(res.fitness[b]) == ref['fitness']
    assert abs(float(res.inlier_rmse[b]) - ref['inlier_rmse']) <= 1e-12 * max(ref['inlier_rmse'], 1e-30) + 1e-18
    if res.idx is not None:
        got = res.idx[src_off[b]:src_off[b + 1]].cpu().numpy()
        want = np.where(ref['idx'] >= 0, ref['idx'] + tgt_off[b], -1)
        assert np.array_equal(got, want), f'{what} pair {b}: idx'
    pose = res.pose[b].cpu().numpy()
    if ref['pose64'] is None:
        assert np.array_equal(pose.view(np.int32), ref['pose'].view(np.int32)), f'{what} pair {b}: a pose that must stay moved'
        return 0.0
    bound = R.pose_bound(ref['last_m'], ref['last_sol'])
    ratio = float((np.abs(pose.astype(np.float64) - ref['pose64']) / bound).max())
    assert ratio <= 1.0, f'{what} pair {b}: pose err / bound = {ratio}'
    return ratio


# ------------------------------------------------------------------------------------------------ 1. one iteration, both oracles
def test_one_iteration_equals_the_restatement_and_the_separate_operators():
    from regtr_amd import ops, overlap
    lens, srcs, tgts, poses = length_batch()
    md = 1.2 * H
    d = Direct(srcs, tgts, poses, md)
    out = d.step(0)
    assert d.margins_untouched()
    so, to = _off(srcs), _off(tgts)
    # the project's own operators on the same packed clouds
    y = ops.se3_transform(d.src, d.s_off, _poses(poses))
    own = overlap.nearest_in_radius(y, d.s_off, d.tgt, d.t_off, md).cpu().numpy()
    assert np.array_equal(out['idx'], own), 'idx differs from overlap.nearest_in_radius(ops.se3_transform(...))'
    worst = 0.0
    for b, n in enumerate(lens):
        ref = R.icp(srcs[b], tgts[b], poses[b], md, iters=1)
        h0 = ref['history'][0]
        rows = slice(so[b], so[b + 1])
        assert np.array_equal(out['idx'][rows], np.where(h0['idx'] >= 0, h0['idx'] + to[b], -1)), f'pair {b} ({n} rows): idx'
        y_ref = R.transform_f32(np.asarray(poses[b], np.float32), srcs[b])
        assert np.array_equal(y[rows].cpu().numpy().view(np.int32), y_ref.view(np.int32)), 'the transform is not the restatement\'s bits'
        _, d2_ref = R.nearest(y_ref, tgts[b], md)
        assert np.array_equal(out['d2'][rows], d2_ref), f'pair {b} ({n} rows): d2'
        assert out['stats'][3 * b + 2] == h0['n'] and out['stats'][3 * b] == h0['fitness']
        assert abs(out['stats'][3 * b + 1] - h0['rmse']) <= 1e-12 * h0['rmse'] + 1e-18
        pose = out['pose'][12 * b:12 * b + 12].reshape(3, 4)
        if n < 3:
            assert out['done'][b] == 1 and out['iters_run'][b] == 0 and ref['iters_run'] == 0
            assert np.array_equal(pose.view(np.int32), np.asarray(poses[b], np.float32).view(np.int32))
        else:
            assert out['done'][b] == 0 and out['iters_run'][b] == 1 and ref['iters_run'] == 1
            ratio = float((np.abs(pose.astype(np.float64) - ref['pose64']) / R.pose_bound(ref['last_m'], ref['last_sol'])).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f'pair {b} ({n} rows): pose err / bound = {ratio}'
    print(f'one iteration, lengths {lens}: worst pose err / bound = {worst:.3f}')


# ------------------------------------------------------------------------------------------------ 2. edges
def test_edges_follow_the_stated_rules_and_the_restatement():
    srcs, tgts, poses, md = edge_batch()
    res = _icp(srcs, tgts, poses, md, iters=3, return_idx=True)
    so, to = _off(srcs), _off(tgts)
    refs = [R.icp(srcs[b], tgts[b], poses[b], md, iters=3) for b in range(len(srcs))]
    for b, ref in enumerate(refs):
        _check_pair(res, b, ref, so, to, 'edges')
    n, it, fit = res.n_inliers.cpu().numpy(), res.iters_run.cpu().numpy(), res.fitness.cpu().numpy()
    assert n[1] == 0 and n[2] == 0 and n[3] == 0 and fit[1] == 0 and fit[3] == 0 and list(it[1:4]) == [0, 0, 0]       # empty clouds
    # the exact cases, in the pass of the identity pose (whose transform is exact): iters=0 returns that pass's matches
    ev = _icp(srcs, tgts, poses, md, iters=0, return_idx=True)
    i4 = ev.idx[so[4]:so[5]].cpu().numpy()
    assert i4[0] == -1, 'a target exactly at max_dist is no inlier (strict <)'
    assert i4[1] == to[4] + 0 and i4[2] == to[4] + 1, 'just inside; of two coincident targets the lower index'
    assert i4[3] == -1 and i4[4] == -1, '27 empty cells; far outside the grid'
    assert int(ev.n_inliers[4]) == 6 and np.array_equal(i4, np.where(refs[4]['history'][0]['idx'] >= 0, refs[4]['history'][0]['idx'] + to[4], -1))
    assert n[5] == 2 and it[5] == 0 and n[6] == 9 and it[6] == 0, 'two matches / collinear matches: the pose stays'
    for b in (5, 6):
        assert torch.equal(res.pose[b], _poses(poses)[b])
    assert it[0] >= 1 and it[7] >= 1 and n[0] == 300 and n[7] == 260


def test_a_nan_pose_freezes_its_pair_and_leaves_the_neighbours_alone():
    srcs, tgts, poses, md = edge_batch()
    keep = [0, 7]
    bad = np.asarray(poses[0], np.float32).copy()
    bad[1, 2] = np.nan
    a = _icp([srcs[0], srcs[7][:100], srcs[7]], [tgts[0], tgts[7], tgts[7]], [poses[0], bad, poses[7]], md, iters=4, return_idx=True)
    b = _icp([srcs[k] for k in keep], [tgts[k] for k in keep], [poses[k] for k in keep], md, iters=4, return_idx=True)
    for k, j in ((0, 0), (2, 1)):
        for f in ('pose', 'fitness', 'inlier_rmse', 'n_inliers', 'iters_run'):
            assert torch.equal(getattr(a, f)[k], getattr(b, f)[j]), f
    assert torch.equal(a.idx[:300], b.idx[:300]) and torch.equal(a.idx[400:] - len(tgts[7]), b.idx[300:])
    assert np.array_equal(a.pose[1].cpu().numpy().view(np.int32), bad.view(np.int32)), 'the frozen pose keeps its bits'
    assert int(a.n_inliers[1]) == 0 and int(a.iters_run[1]) == 0 and float(a.fitness[1]) == 0.0 and bool((a.idx[300:400] == -1).all())


# ------------------------------------------------------------------------------------------------ 3. the loop
@pytest.fixture(scope='module')
def wide():
    src, tgt, p0, md = wide_case()
    return src, tgt, p0, md, R.icp(src, tgt, p0, md, iters=30)


def test_the_loop_follows_the_restatement(wide):
    src, tgt, p0, md, ref = wide
    d = Direct([src], [tgt], [p0], md)
    ns, outs = [], []
    for k in range(31):
        o = d.step(k, stats_only=(k == 30))
        ns.append(int(o['stats'][2])); outs.append(o)
        if o['done'][0]:
            break
    assert d.margins_untouched()
    assert ns == [r['n'] for r in ref['history']], 'the n_inliers sequence'
    assert outs[-1]['iters_run'][0] == ref['iters_run'] and outs[-1]['done'][0] == 1 and ref['done']
    res = _icp([src], [tgt], [p0], md, iters=30, return_idx=True)
    ratio = _check_pair(res, 0, ref, [0, len(src)], [0, len(tgt)], 'loop')
    assert np.array_equal(res.pose[0].cpu().numpy(), outs[-1]['pose'].reshape(3, 4)), 'refine.icp is the loop of direct steps'
    rot, trans = R.pose_errors(res.pose[0].cpu().numpy(), GT)
    rr, rt = R.pose_errors(ref['pose'], GT)
    b = R.pose_bound(ref['last_m'], ref['last_sol'])
    assert abs(trans - rt) <= 2 * np.linalg.norm(b[:, 3]) and abs(np.radians(rot) - np.radians(rr)) <= 2 * np.linalg.norm(b[:, :3]) + 2.0 ** -11.5
    print(f'loop of {ref["iters_run"]} iterations: pose err / bound = {ratio:.3f}; rot / trans error against ground truth {rot:.2e} deg / {trans:.2e}')


def test_a_pair_at_its_fixed_point_is_done_at_iteration_one_and_never_written_again(wide):
    src, tgt, p0, md, ref = wide
    d = Direct([src, src], [tgt, tgt], [ref['pose'], p0], md)
    snaps = [d.step(k) for k in range(5)]
    assert snaps[0]['done'].tolist() == [0, 0] and snaps[1]['done'].tolist() == [1, 0] and snaps[4]['done'].tolist() == [1, 0]
    assert snaps[1]['iters_run'][0] == 1 and snaps[4]['iters_run'].tolist() == [1, 5]
    d.view['idx'][:len(src)].fill_(SENT)                # a done pair's rows are not written by later passes
    d.view['d2'][:len(src)].fill_(SENT)
    more = d.step(5)
    assert (more['idx'][:len(src)] == SENT).all() and (more['d2'][:len(src)] == SENT).all() and (more['idx'][len(src):] != SENT).all()
    for s in snaps[2:] + [more]:
        for f, w in (('pose', 12), ('stats', 3)):
            assert np.array_equal(s[f][:w].view(np.int64 if f == 'stats' else np.int32), snaps[1][f][:w].view(np.int64 if f == 'stats' else np.int32))
    assert not np.array_equal(snaps[4]['pose'][12:], snaps[1]['pose'][12:]), 'the second pair goes on'
    assert d.margins_untouched()


def test_zero_iterations_is_evaluate_registration(wide):
    from regtr_amd import refine
    src, tgt, p0, md, ref = wide
    r = _icp([src, src[:77]], [tgt, tgt], [p0, GT], md, iters=0)
    f, e, n = refine.evaluate_registration(_clouds([src, src[:77]]), _clouds([tgt, tgt]), _poses([p0, GT]), md)
    assert torch.equal(r.fitness, f) and torch.equal(r.inlier_rmse, e) and torch.equal(r.n_inliers, n)
    assert torch.equal(r.pose, _poses([p0, GT])) and r.iters_run.tolist() == [0, 0]
    h0 = ref['history'][0]
    assert int(n[0]) == h0['n'] and float(f[0]) == h0['fitness'] and int(n[1]) == 77 and float(f[1]) == 1.0
    assert f.dtype == torch.float64 and n.dtype == torch.int32 and r.pose.shape == (2, 3, 4)
    p44 = torch.eye(4, device='cuda').repeat(2, 1, 1)
    p44[:, :3] = _poses([p0, GT])
    assert torch.equal(refine.evaluate_registration(_clouds([src, src[:77]]), _clouds([tgt, tgt]), p44, md)[2], n), '(B, 4, 4) poses'


# ------------------------------------------------------------------------------------------------ 4. reproducibility and routes
def test_two_runs_are_bit_identical(wide):
    lens, srcs, tgts, poses = length_batch()
    a = _icp(srcs, tgts, poses, 1.2 * H, iters=6, return_idx=True)
    b = _icp(srcs, tgts, poses, 1.2 * H, iters=6, return_idx=True)
    for f in a._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_fused_and_composed_routes_agree(wide):
    from regtr_amd import refine
    src, tgt, p0, md, ref = wide
    s2, t2, _, _ = R.overlapping_pair(300, H, 11, GT, extra=40)
    srcs, tgts, poses = [src, s2, src[:2]], [tgt, t2, tgt], [p0, R.perturbed(GT, *SUB), GT]
    fused = _icp(srcs, tgts, poses, md, iters=3, return_idx=True)
    prev = refine.use_fused_icp(False)
    try:
        comp = _icp(srcs, tgts, poses, md, iters=3, return_idx=True)
    finally:
        refine.use_fused_icp(prev)
    assert prev is True
    assert torch.equal(fused.idx, comp.idx) and torch.equal(fused.n_inliers, comp.n_inliers) and torch.equal(fused.iters_run, comp.iters_run)
    assert torch.equal(fused.fitness, comp.fitness)
    for b in range(2):
        r = R.icp(srcs[b], tgts[b], poses[b], md, iters=3)
        bound = R.pose_bound(r['last_m'], r['last_sol']) + R.composed_bound(r['last_m'], r['last_sol'])
        diff = np.abs(fused.pose[b].cpu().numpy().astype(np.float64) - comp.pose[b].cpu().numpy())
        assert np.all(diff <= bound), f'pair {b}: fused against composed {(diff / bound).max()} of the bound'
        # the same matches under two poses that far apart: no transformed point, so no residual and no rmse, differs by more than
        # |dy| <= sqrt(3) max_r (sum_c bound[r, c] max|p| + bound[r, 3])   (+ the float32 roundings of the transform itself)
        pmax = float(np.abs(srcs[b]).max())
        dy = np.sqrt(3) * ((bound[:, :3].sum(1) * pmax + bound[:, 3]).max() + 4 * 2.0 ** -24 * (3 * pmax + np.abs(r['pose'][:, 3]).max()))
        assert abs(float(fused.inlier_rmse[b]) - float(comp.inlier_rmse[b])) <= dy, (b, float(fused.inlier_rmse[b]), float(comp.inlier_rmse[b]), dy)
    # a pair that is never updated keeps one pose on both routes: the same residuals, added in another order
    assert torch.equal(fused.pose[2], comp.pose[2]) and int(comp.iters_run[2]) == 0
    assert abs(float(fused.inlier_rmse[2]) - float(comp.inlier_rmse[2])) <= 1e-12 * float(fused.inlier_rmse[2])


# ------------------------------------------------------------------------------------------------ 5. recovery
def test_a_sub_spacing_start_recovers_the_ground_truth():
    src, tgt, perm, noise = R.overlapping_pair(2000, H, 1, GT, extra=500)
    p0 = R.perturbed(GT, *SUB)
    res = _icp([src], [tgt], [p0], 2 * H, iters=30, return_idx=True)
    ref = R.icp(src, tgt, p0, 2 * H, iters=30)
    _check_pair(res, 0, ref, [0, len(src)], [0, len(tgt)], 'recovery')
    assert np.array_equal(res.idx.cpu().numpy(), perm)
    b = R.pose_bound(ref['last_m'], ref['last_sol'], noise)
    pose = res.pose[0].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(pose - GT) <= b), (np.abs(pose - GT) / b).max()
    rot, trans = R.pose_errors(pose, GT)
    assert trans <= np.linalg.norm(b[:, 3]) and np.radians(rot) <= 2 * np.linalg.norm(b[:, :3]) + 2.0 ** -11.5
    assert float(res.fitness[0]) == 1.0 and float(res.inlier_rmse[0]) < 2 * noise * np.sqrt(3)


# ------------------------------------------------------------------------------------------------ 6. plumbing, 7. the default path
@pytest.fixture(scope='module')
def plumbing():
    from regtr_amd import RegTR, harness
    cfg = load_cfg('3dmatch')
    model = RegTR(cfg)
    model.load_state_dict(seeded_sd(cfg), strict=True)
    model = model.cuda().eval()
    pairs = harness.SyntheticPairs(5, points=20000)       # (test.py's synthetic pairs)
    dev = torch.device('cuda', torch.cuda.current_device())
    plain, ids, _ = harness.run_test(model, pairs, 2, dev)
    return cfg, model, pairs, dev, plain, ids


REFINE = {'max_dist': 0.05, 'iters': 5}


def _expected(pairs, plain):
    from regtr_amd import refine
    out = []
    for i in range(len(pairs)):
        it = pairs[i]
        r = refine.icp(_clouds([it['src_xyz']]), _clouds([it['tgt_xyz']]), _dev(plain[i:i + 1]), REFINE['max_dist'], iters=REFINE['iters'])
        out.append(r.pose[0].cpu().numpy())
    return np.stack(out)


def test_refine_pose_is_refine_icp(plumbing):
    from regtr_amd import refine
    cfg, model, pairs, dev, plain, _ = plumbing
    batch = {'src_xyz': _clouds([pairs[i]['src_xyz'] for i in range(2)]), 'tgt_xyz': _clouds([pairs[i]['tgt_xyz'] for i in range(2)])}
    pose = _dev(plain[:2])
    a = model.refine_pose(batch, pose)
    b = refine.icp(batch['src_xyz'], batch['tgt_xyz'], pose, 2 * cfg.first_subsampling_dl, iters=30)
    c = model.refine_pose(batch, pose, max_dist=0.05, iters=5)
    d = refine.icp(batch['src_xyz'], batch['tgt_xyz'], pose, 0.05, iters=5)
    for x, y in ((a, b), (c, d)):
        for f in ('pose', 'fitness', 'inlier_rmse', 'n_inliers', 'iters_run'):
            assert torch.equal(getattr(x, f), getattr(y, f)), f
    assert torch.equal(pose, _dev(plain[:2])), 'the caller\'s pose is not refined in place'


def test_run_test_refine_returns_the_refined_pose_of_every_pair(plumbing):
    from regtr_amd import harness
    from regtr_amd.workload import replicate
    cfg, model, pairs, dev, plain, ids = plumbing
    want = _expected(pairs, plain)
    got, ids2, timing = harness.run_test(model, pairs, 2, dev, refine=dict(REFINE))
    assert np.array_equal(ids, ids2) and np.array_equal(got.view(np.int32), want.view(np.int32))
    rf = timing['refine']
    assert set(rf) == {'fitness_before', 'inlier_rmse_before', 'fitness_after', 'inlier_rmse_after'} and all(np.isfinite(v) for v in rf.values())
    assert 0 <= rf['fitness_before'] <= 1 and 0 <= rf['fitness_after'] <= 1
    got3, _, _ = harness.run_test(replicate(model, cfg, 2, dev), pairs, 2, dev, refine=dict(REFINE))
    assert np.array_equal(got3.view(np.int32), want.view(np.int32)), 'replicas'
    with pytest.raises(NotImplementedError, match='raw clouds'):
        harness.run_test_shared(model, pairs, 2, dev, refine=dict(REFINE))


def _read_est(path):
    lines = open(path).read().strip().split('\n')
    return np.stack([np.array([[float(v) for v in lines[k + 1 + r].split('\t')] for r in range(3)]) for k in range(0, len(lines), 5)])


def test_cli_refine_writes_the_refined_poses(plumbing, tmp_path):
    cfg, model, pairs, dev, plain, _ = plumbing
    want = _expected(pairs, plain)
    ck = tmp_path / 'model.pth'
    torch.save({'state_dict': model.state_dict(), 'step': 0}, ck)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '--benchmark', '3DMatch', '--config',
                        os.path.join(ROOT, 'regtr_amd', 'conf', '3dmatch.yaml'), '--logdir', str(tmp_path / 'logs'), '--name', 't', '--resume', str(ck),
                        '--synthetic', '5', '--batch', '2', '--num_workers', '0', '--replicas', '1', '--no_warmup', '--refine', 'icp',
                        '--refine_dist', str(REFINE['max_dist']), '--refine_iters', str(REFINE['iters'])], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '[Refine] icp' in r.stderr or '[Refine] icp' in r.stdout
    run = os.listdir(tmp_path / 'logs')[0]
    est = _read_est(tmp_path / 'logs' / run / '3DMatch' / 'synthetic-scene000' / 'est.log')
    assert est.shape == (5, 3, 4) and np.array_equal(est.astype(np.float32), want), np.abs(est - want).max()


def test_without_refine_the_launches_and_bits_are_a_plain_run(plumbing):
    """run_test without refine: per entry point the calls of the model's plain forwards over the same batches (the launches of the
    parent commit), none of them an ICP entry point, and the poses of those forwards bit for bit."""
    from regtr_amd import _lib, harness
    cfg, model, pairs, dev, plain, ids = plumbing
    L = _lib.lib()
    counts = {}
    originals = {name: getattr(L, name) for name in _lib.SIGNATURES}

    def counted(name, fn):
        def call(*a):
            counts[name] = counts.get(name, 0) + 1
            return fn(*a)
        return call
    for name, fn in originals.items():
        setattr(L, name, counted(name, fn))
    try:
        got, ids2, timing = harness.run_test(model, pairs, 2, dev)
        in_run, counts = dict(counts), {}
        outs = []
        with torch.no_grad():
            for lo in range(0, 5, 2):
                its = [pairs[i] for i in range(lo, min(lo + 2, 5))]
                outs.append(model({'src_xyz': _clouds([it['src_xyz'] for it in its]), 'tgt_xyz': _clouds([it['tgt_xyz'] for it in its])})['pose'][-1])
        torch.cuda.synchronize()
        forwards = dict(counts)
    finally:
        for name, fn in originals.items():
            setattr(L, name, fn)
    assert in_run == forwards and sum(in_run.values()) > 100, {k: (in_run.get(k), forwards.get(k)) for k in set(in_run) ^ set(forwards)}
    assert not [k for k in in_run if 'icp' in k or k == 'regtr_nearest_in_radius']
    assert 'refine' not in timing
    assert np.array_equal(got.view(np.int32), torch.cat(outs).cpu().numpy().view(np.int32)) and np.array_equal(got.view(np.int32), plain.view(np.int32))
