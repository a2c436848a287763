"""GPU (-m gpu): regtr_amd.refine.estimate_normals and refine.icp(method='point_to_plane') (csrc/icp_plane.hip) against the numpy
restatement tests/icp_plane_ref.py, against point-to-point ICP on the same pose (matches and stats) and against the composed route.

Moments, valid flags, matches and counts are compared exactly; normals and poses within the bounds icp_plane_ref derives.  The rmse of
the restatement is a float64 sum in another order than the kernel's: it is compared to n u64 (the rmse of refine.icp(iters=0), the same
kernel arithmetic, bit for bit)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import icp_plane_ref as P
from tests import icp_ref as R
from tests.test_icp_plane_host import CORNER_MD, CORNER_START, GT, NR, STEP_MD, normal_clouds, room_crop, step_batch, walls
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


def _off(arrs):
    return np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)


def _given(nrms, valids):
    return ([_dev(np.asarray(n, np.float32).reshape(-1, 3)) for n in nrms], [_dev(np.asarray(v, np.int32).reshape(-1)) for v in valids])


def _plane(srcs, tgts, poses, md, nrms=None, valids=None, **kw):
    from regtr_amd import refine
    given = _given(nrms, valids) if nrms is not None else None
    return refine.icp(_clouds(srcs), _clouds(tgts), _poses(poses), md, method='point_to_plane', tgt_normals=given, **kw)


def _composed(fn):
    from regtr_amd import refine
    prev = refine.use_fused_icp(False)
    try:
        return fn()
    finally:
        refine.use_fused_icp(prev)


# ------------------------------------------------------------------------------------------------ 1. normals
@pytest.fixture(scope='module')
def normal_case():
    from regtr_amd import refine
    clouds = normal_clouds()
    refs = [P.normals(c, NR) for c in clouds]
    out = refine.estimate_normals(_clouds(clouds), NR, return_moments=True)
    again = refine.estimate_normals(_clouds(clouds), NR, return_moments=True)
    return clouds, refs, out, again


def test_normal_moments_and_valid_flags_equal_the_restatement(normal_case):
    clouds, refs, (nrm, valid, mom), _ = normal_case
    assert [tuple(n.shape) for n in nrm] == [(len(c), 3) for c in clouds] and nrm[0].dtype == torch.float32
    assert valid[0].dtype == torch.int32 and mom[0].dtype == torch.int64 and tuple(mom[-1].shape) == (1500, 10)
    for k, r in enumerate(refs):
        assert np.array_equal(mom[k].cpu().numpy(), r['moments']), f'cloud {k}: moments'
        assert np.array_equal(valid[k].cpu().numpy(), r['valid']), f'cloud {k}: valid'
        bad = valid[k] == 0
        assert bool((nrm[k][bad] == 0).all()), f'cloud {k}: an invalid normal is exactly 0'
    lat = nrm[4][:256].cpu().numpy()
    assert np.all(lat[:, :2] == 0) and np.all(np.abs(lat[:, 2]) == 1), 'an exact z = 0 lattice: exactly (0, 0, +-1)'
    assert torch.equal(nrm[3][10:19].abs(), nrm[3][19:28].abs()), 'the same nine points 100 m away: the same normals'


def test_normals_are_unit_eigenvectors_within_the_derived_bounds(normal_case):
    clouds, refs, (nrm, valid, mom), _ = normal_case
    worst = {'unit': 0.0, 'residual': 0.0, 'angle': 0.0}
    for k, r in enumerate(refs):
        ok = r['valid'] != 0
        if not ok.any():
            continue
        n = nrm[k].cpu().numpy().astype(np.float64)[ok]
        C, lam = r['C'][ok], r['lam'][ok]
        unit = np.abs(np.linalg.norm(n, axis=1) - 1)
        res = np.linalg.norm(np.einsum('nij,nj->ni', C, n) - lam[:, :1] * n, axis=1)
        rb = P.eigen_residual_bound(C)
        worst['unit'] = max(worst['unit'], float(unit.max() / (4 * 2.0 ** -24)))
        worst['residual'] = max(worst['residual'], float((res / rb).max()))
        assert np.all(unit <= 4 * 2.0 ** -24), f'cloud {k}: |n| - 1 up to {unit.max()}'
        assert np.all(res <= rb), f'cloud {k}: eigen-residual up to {(res / rb).max()} of its bound'
        exempt = (lam[:, 1] - lam[:, 0]) < 1e-6 * lam[:, 2]
        assert exempt.mean() <= 0.01, f'cloud {k}: {exempt.sum()} rows with a closed eigen-gap'
        ang, ab = P.angle(n, r['normals'][ok]), P.normal_angle_bound(lam)
        worst['angle'] = max(worst['angle'], float((ang / ab)[~exempt].max()))
        assert np.all(ang[~exempt] <= ab[~exempt]), f'cloud {k}: angle up to {(ang / ab)[~exempt].max()} of its bound'
    print('normals, worst / bound:', {k: round(v, 3) for k, v in worst.items()})


def test_two_normal_runs_are_bit_identical(normal_case):
    _, _, out, again = normal_case
    for a, b in zip(out, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 2. one step
class Direct:
    """regtr_icp_plane_step called directly over buffers with sentinel margins around pose, pose64, stats, idx, iters_run and done."""

    PAD = 16

    def __init__(self, srcs, tgts, poses, md, nrms, valids):
        from regtr_amd import _lib, ops
        self.L, self._lib = _lib.lib(), _lib
        self.B = len(srcs)
        cat = lambda arrs, w, dt: _dev(np.concatenate([np.asarray(a, dt).reshape((-1,) + w) for a in arrs]))
        self.src, self.tgt = cat(srcs, (3,), np.float32), cat(tgts, (3,), np.float32)
        self.nrm, self.valid = cat(nrms, (3,), np.float32), cat(valids, (), np.int32)
        self.s_off, self.t_off = _dev(_off(srcs).astype(np.int32)), _dev(_off(tgts).astype(np.int32))
        self.max_len = max(len(s) for s in srcs)
        self.md, self.r32 = float(md), float(np.float32(md))
        self.grid = ops.CellGrid(self.tgt, self.t_off, self.tgt.shape[0], self.r32)
        n, B, Pd = self.src.shape[0], self.B, self.PAD
        full = lambda m, v, dt: torch.full((m + 2 * Pd,), v, dtype=dt, device='cuda')
        self.buf = {'pose': full(B * 12, float(SENT), torch.float32), 'pose64': full(B * 12, float(SENT), torch.float64),
                    'stats': full(B * 3, float(SENT), torch.float64), 'idx': full(n, SENT, torch.int32),
                    'iters_run': full(B, SENT, torch.int32), 'done': full(B, SENT, torch.int32)}
        self.view = {k: v[Pd:v.numel() - Pd] for k, v in self.buf.items()}
        self.view['pose'].copy_(_poses(poses).reshape(-1))
        chunks = -(-self.max_len // int(self.L.regtr_icp_chunk()))
        self.partial = torch.full((B * chunks * P.NSUMS + 2 * Pd,), float(SENT), dtype=torch.float64, device='cuda')

    def step(self, it, stats_only=False, rel=1e-6):
        v, p = self.view, lambda t: t.data_ptr()
        self._lib.check(self.L.regtr_icp_plane_step(p(self.src), p(self.s_off), self.src.shape[0], self.max_len, p(self.nrm), p(self.valid),
                                                    p(self.t_off), self.tgt.shape[0], self.B, self.md, self.r32, p(self.grid.ws),
                                                    self.grid.nbytes, p(v['pose']), p(v['pose64']), it, int(stats_only), rel, rel,
                                                    p(v['stats']), p(v['iters_run']), p(v['done']), p(v['idx']),
                                                    p(self.partial[self.PAD:]), None), 'regtr_icp_plane_step')
        torch.cuda.synchronize()
        return {k: t.cpu().numpy().copy() for k, t in v.items()}

    def margins_untouched(self):
        Pd = self.PAD
        return all(bool((b[:Pd] == SENT).all()) and bool((b[-Pd:] == SENT).all()) for b in list(self.buf.values()) + [self.partial])


def test_one_step_matches_point_to_point_and_solves_within_the_derived_bound():
    from regtr_amd import refine
    srcs, tgts, poses, nrms, valids = step_batch()
    so, to = _off(srcs), _off(tgts)
    d = Direct(srcs, tgts, poses, STEP_MD, nrms, valids)
    out = d.step(0)
    assert d.margins_untouched()
    ev = refine.icp(_clouds(srcs), _clouds(tgts), _poses(poses), STEP_MD, iters=0, return_idx=True)       # point to point, the same pose
    assert np.array_equal(out['idx'], ev.idx.cpu().numpy()), 'idx differs from point-to-point ICP under the same pose'
    st = out['stats'].reshape(-1, 3)
    assert np.array_equal(st[:, 2], ev.n_inliers.cpu().numpy().astype(np.float64)), 'n_match'
    assert np.array_equal(st[:, 0].view(np.int64), ev.fitness.cpu().numpy().view(np.int64)), 'fitness bits'
    assert np.array_equal(st[:, 1].view(np.int64), ev.inlier_rmse.cpu().numpy().view(np.int64)), 'inlier_rmse bits'
    one = _plane(srcs, tgts, poses, STEP_MD, nrms, valids, iters=1, return_idx=True)
    comp = _composed(lambda: _plane(srcs, tgts, poses, STEP_MD, nrms, valids, iters=1, return_idx=True))
    worst = {'fused': 0.0, 'composed': 0.0}
    for b, n in enumerate(len(s) for s in srcs):
        ref = P.icp_plane(srcs[b], tgts[b], poses[b], STEP_MD, nrms[b], valids[b], iters=1)
        h0 = ref['history'][0]
        assert np.array_equal(out['idx'][so[b]:so[b + 1]], np.where(h0['idx'] >= 0, h0['idx'] + to[b], -1)), f'pair {b} ({n} rows): idx'
        assert st[b, 2] == h0['n'] and st[b, 0] == h0['fitness'] and abs(st[b, 1] - h0['rmse']) <= n * P.U64 * h0['rmse'] + 1e-18
        pose = out['pose'][12 * b:12 * b + 12].reshape(3, 4)
        p64 = out['pose64'][12 * b:12 * b + 12].reshape(3, 4)
        if ref['iters_run'] == 0:
            assert out['done'][b] == 1 and out['iters_run'][b] == 0 and int(one.iters_run[b]) == 0 and int(comp.iters_run[b]) == 0
            start = np.asarray(poses[b], np.float32)
            assert np.array_equal(pose.view(np.int32), start.view(np.int32)) and np.array_equal(p64, start.astype(np.float64))
            assert torch.equal(one.pose[b], _poses(poses)[b]) and torch.equal(comp.pose[b], _poses(poses)[b])
            continue
        assert out['done'][b] == 0 and out['iters_run'][b] == 1
        bound = P.step_bound(ref['last_s'], ref['last_sol'], ref['last_prev'], ref['pose64'])
        assert np.array_equal(pose, p64.astype(np.float32)), 'pose is the float32 rounding of pose64'
        assert np.array_equal(pose, one.pose[b].cpu().numpy()), 'refine.icp(iters=1) is one direct step'
        for name, got in (('fused', pose), ('composed', comp.pose[b].cpu().numpy())):
            ratio = float((np.abs(got.astype(np.float64) - ref['pose64']) / bound).max())
            worst[name] = max(worst[name], ratio)
            assert ratio <= 1.0, f'pair {b} ({n} rows), {name}: pose err / bound = {ratio}'
    assert torch.equal(comp.idx, one.idx) and torch.equal(comp.n_inliers, one.n_inliers)
    assert torch.equal(comp.iters_run, one.iters_run) and torch.equal(comp.fitness, one.fitness)
    assert list(out['iters_run']) == [1, 0, 0, 0, 1] and list(st[:, 2]) == [255, 0, 257, 1, 700]
    print('one step, worst pose err / bound:', {k: round(v, 4) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------------ 3. the loop
@pytest.fixture(scope='module')
def room():
    src, tgt, gt, starts = room_crop()
    return src, tgt, gt, starts, P.normals(tgt, 0.05)


@pytest.mark.parametrize('k', [0, 1, 2])
def test_the_loop_follows_the_restatement(room, k):
    """Pass by pass: every row whose decision the restatement finds clear of rounding has the restatement's match; as long as ALL rows
    of a pass have it, both sides solve the same system and the next poses agree within the accumulated bound, so the comparison goes
    on.  With every pass equal: the same iteration count, and the final pose within the loop's bound."""
    src, tgt, gt, starts, N = room
    p0 = starts[k]
    ref = P.icp_plane(src, tgt, p0, 0.05, N['normals'], N['valid'], iters=30, margins=True, nearest=P.kd_nearest)
    need = R.match_margin_needed(src, p0, 0.05)
    d = Direct([src], [tgt], [p0], 0.05, [N['normals']], [N['valid']])
    same, outs = True, []
    for it, rec in enumerate(ref['history']):
        o = d.step(it, stats_only=(it == 30))
        outs.append(o)
        clear = rec['gap_rows'] > need
        assert np.array_equal(o['idx'][clear], rec['idx'][clear]), f'start {k}, pass {it}: a clear match differs'
        same = np.array_equal(o['idx'], rec['idx']) and min(rec.get('stop_margin', (1,))) > 1e-8
        if not same:
            break
        assert int(o['stats'][2]) == rec['n'], f'start {k}, pass {it}: n_match'
    assert d.margins_untouched()
    print(f'start {k}: {len(outs)} of {len(ref["history"])} passes compared, all equal: {same}; restatement ran {ref["iters_run"]} iterations')
    if same:
        assert outs[-1]['iters_run'][0] == ref['iters_run'] and outs[-1]['done'][0] == int(ref['done'])
        err = np.abs(outs[-1]['pose'].reshape(3, 4).astype(np.float64) - ref['pose64'])
        assert np.all(err <= P.loop_bound(ref)), f'start {k}: pose err / bound = {(err / P.loop_bound(ref)).max()}'
        res = _plane([src], [tgt], [p0], 0.05, [N['normals']], [N['valid']], iters=30)
        assert np.array_equal(res.pose[0].cpu().numpy(), outs[-1]['pose'].reshape(3, 4)), 'refine.icp is the loop of direct steps'
        assert int(res.iters_run[0]) == ref['iters_run'] and int(res.n_inliers[0]) == ref['n_inliers']


# ------------------------------------------------------------------------------------------------ 4. the box corner
def test_the_box_corner_is_recovered_in_no_more_iterations_than_point_to_point():
    from regtr_amd import refine
    src, tgt, perm, noise = P.box_corner(17, 0.02, 5, GT)
    N = P.normals(tgt, 0.05)
    p0 = R.perturbed(GT, *CORNER_START)
    res = _plane([src], [tgt], [p0], CORNER_MD, [N['normals']], [N['valid']], iters=30, return_idx=True)
    own = _plane([src], [tgt], [p0], CORNER_MD, iters=30, normal_radius=0.05)                 # normals estimated on the device
    pp = refine.icp(_clouds([src]), _clouds([tgt]), _poses([p0]), CORNER_MD, iters=30)
    ref = P.icp_plane(src, tgt, p0, CORNER_MD, N['normals'], N['valid'], iters=30)
    assert np.array_equal(res.idx.cpu().numpy(), perm), 'every source row ends on its own image'
    dy = 4 * 2.0 ** -24 * (np.abs(src).sum(1).max() + np.abs(GT[:, 3]).max())
    b = P.step_bound(ref['last_s'], ref['last_sol'], ref['last_prev'], ref['pose64'], target_noise=noise, dy=dy)
    for r in (res, own):
        err = np.abs(r.pose[0].cpu().numpy().astype(np.float64) - GT)
        assert np.all(err <= b), (err / b).max()
        assert 2 <= int(r.iters_run[0]) <= int(pp.iters_run[0]), (int(r.iters_run[0]), int(pp.iters_run[0]))
        assert float(r.fitness[0]) == 1.0 and float(r.inlier_rmse[0]) < 2 * noise * np.sqrt(3)
    print(f'box corner: {int(res.iters_run[0])} point-to-plane iterations, {int(pp.iters_run[0])} point-to-point; err / bound '
          f'{(np.abs(res.pose[0].cpu().numpy().astype(np.float64) - GT) / b).max():.2e}')


# ------------------------------------------------------------------------------------------------ 5. edges
def test_a_single_plane_stops_at_once_and_keeps_its_pose():
    ws = walls()
    start = R.pose_of([0, 0, 1], 0.2, [0.002, 0.001, 0.0])
    for nr in (None, 0.05):
        res = _plane(ws, ws, [start, start], 0.05, iters=5, normal_radius=nr)
        assert res.iters_run.tolist() == [0, 0], 'one wall fixes no pose'
        assert np.array_equal(res.pose.cpu().numpy().view(np.int32), _poses([start, start]).cpu().numpy().view(np.int32))
        assert res.n_inliers.tolist() == [len(w) for w in ws]


def test_a_nan_pose_freezes_its_pair_and_leaves_the_neighbours_alone():
    srcs, tgts, poses, nrms, valids = step_batch()
    bad = np.asarray(poses[4], np.float32).copy()
    bad[1, 2] = np.nan
    pick = lambda xs, ks: [xs[k] for k in ks]
    a = _plane(pick(srcs, [0, 4, 4]), pick(tgts, [0, 4, 4]), [poses[0], bad, poses[4]], STEP_MD, pick(nrms, [0, 4, 4]), pick(valids, [0, 4, 4]),
               iters=4, return_idx=True)
    b = _plane(pick(srcs, [0, 4]), pick(tgts, [0, 4]), pick(poses, [0, 4]), STEP_MD, pick(nrms, [0, 4]), pick(valids, [0, 4]), iters=4,
               return_idx=True)
    for k, j in ((0, 0), (2, 1)):
        for f in ('pose', 'fitness', 'inlier_rmse', 'n_inliers', 'iters_run'):
            assert torch.equal(getattr(a, f)[k], getattr(b, f)[j]), f
    assert torch.equal(a.idx[:255], b.idx[:255]) and torch.equal(a.idx[955:] - len(tgts[4]), b.idx[255:])
    assert np.array_equal(a.pose[1].cpu().numpy().view(np.int32), bad.view(np.int32)), 'the frozen pose keeps its bits'
    assert int(a.n_inliers[1]) == 0 and int(a.iters_run[1]) == 0 and float(a.fitness[1]) == 0.0 and bool((a.idx[255:955] == -1).all())
    assert int(a.iters_run[0]) >= 1 and int(a.iters_run[2]) >= 1


def test_a_done_pair_is_never_written_again():
    srcs, tgts, poses, nrms, valids = step_batch()
    ref = P.icp_plane(srcs[4], tgts[4], poses[4], STEP_MD, nrms[4], valids[4], iters=30)
    assert ref['done'] and ref['iters_run'] >= 1
    # pair 0 starts at pair 4's result: done after its first update or two; pair 1 goes on from the batch's start
    d = Direct([srcs[4], srcs[4]], [tgts[4], tgts[4]], [ref['pose'], poses[4]], STEP_MD, [nrms[4]] * 2, [valids[4]] * 2)
    snaps = [d.step(k) for k in range(ref['iters_run'] + 3)]
    first = next(k for k, s in enumerate(snaps) if s['done'][0] == 1)
    assert first <= 3 and snaps[first]['iters_run'][0] == first
    n0 = len(srcs[4])
    d.view['idx'][:n0].fill_(SENT)
    more = d.step(len(snaps))
    assert (more['idx'][:n0] == SENT).all(), 'a done pair\'s idx rows are not written by later passes'
    for s in snaps[first + 1:] + [more]:
        for f, w in (('pose', 12), ('pose64', 12), ('stats', 3)):
            assert np.array_equal(s[f][:w].tobytes(), snaps[first][f][:w].tobytes()), f
        assert s['done'][0] == 1 and s['iters_run'][0] == first
    assert snaps[1]['iters_run'][1] == 2 and not np.array_equal(snaps[1]['pose'][12:], snaps[0]['pose'][12:]), 'the second pair goes on'
    assert d.margins_untouched()


# ------------------------------------------------------------------------------------------------ 6. workspace, 7. the default path
@pytest.mark.parametrize('fill', ['ones', 'random'])
def test_poisoned_workspaces_change_no_bit(fill):
    from tests.workspace_poison import PoisonedWorkspaces
    srcs, tgts, poses, nrms, valids = step_batch()
    plain = _plane(srcs, tgts, poses, STEP_MD, iters=4, return_idx=True)
    with PoisonedWorkspaces(fill) as hook:
        got = _plane(srcs, tgts, poses, STEP_MD, iters=4, return_idx=True)
        torch.cuda.synchronize()
    assert hook.check() >= 3 and hook.served(5 * 3 * P.NSUMS * 8) == 1 and hook.served(5 * 12 * 8) == 1, hook.sizes()
    for f in plain._fields:
        assert torch.equal(getattr(plain, f), getattr(got, f)), f


def test_the_default_method_launches_no_point_to_plane_kernel():
    from torch.profiler import ProfilerActivity, profile
    from regtr_amd import refine
    srcs, tgts, poses, nrms, valids = step_batch()
    names = {}
    for method in ('default', 'point_to_plane'):
        kw = {} if method == 'default' else {'method': method}
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            refine.icp(_clouds(srcs), _clouds(tgts), _poses(poses), STEP_MD, iters=2, **kw)
            torch.cuda.synchronize()
        names[method] = {e.key: e.count for e in prof.key_averages()}
    mine = lambda ks: sorted(k for k in ks if 'k_estimate_normals' in k or 'k_icp_plane' in k)
    assert not mine(names['default']), mine(names['default'])
    assert len(mine(names['point_to_plane'])) == 3, sorted(names['point_to_plane'])
    assert any('k_icp_accumulate' in k for k in names['default']) and not any('k_icp_accumulate' in k for k in names['point_to_plane'])


# ------------------------------------------------------------------------------------------------ 8. plumbing
@pytest.fixture(scope='module')
def plumbing():
    from regtr_amd import RegTR, harness
    cfg = load_cfg('3dmatch')
    model = RegTR(cfg)
    model.load_state_dict(seeded_sd(cfg), strict=True)
    model = model.cuda().eval()
    pairs = harness.SyntheticPairs(3, points=20000)
    dev = torch.device('cuda', torch.cuda.current_device())
    plain, ids, _ = harness.run_test(model, pairs, 2, dev)
    return cfg, model, pairs, dev, plain, ids


REFINE = {'max_dist': 0.05, 'iters': 5, 'method': 'point_to_plane', 'normal_radius': 0.06}


def _expected(pairs, plain):
    from regtr_amd import refine
    out = []
    for i in range(len(pairs)):
        it = pairs[i]
        r = refine.icp(_clouds([it['src_xyz']]), _clouds([it['tgt_xyz']]), _dev(plain[i:i + 1]), REFINE['max_dist'], iters=REFINE['iters'],
                       method='point_to_plane', normal_radius=REFINE['normal_radius'])
        out.append(r.pose[0].cpu().numpy())
    return np.stack(out)


def test_refine_pose_is_refine_icp(plumbing):
    from regtr_amd import refine
    cfg, model, pairs, dev, plain, _ = plumbing
    batch = {'src_xyz': _clouds([pairs[i]['src_xyz'] for i in range(2)]), 'tgt_xyz': _clouds([pairs[i]['tgt_xyz'] for i in range(2)])}
    pose = _dev(plain[:2])
    dl2 = 2 * cfg.first_subsampling_dl
    a = model.refine_pose(batch, pose, method='point_to_plane', iters=4)
    b = refine.icp(batch['src_xyz'], batch['tgt_xyz'], pose, dl2, iters=4, method='point_to_plane', normal_radius=dl2)
    c = model.refine_pose(batch, pose, max_dist=0.05, iters=3, method='point_to_plane', normal_radius=0.07)
    e = refine.icp(batch['src_xyz'], batch['tgt_xyz'], pose, 0.05, iters=3, method='point_to_plane', normal_radius=0.07)
    for x, y in ((a, b), (c, e)):
        for f in ('pose', 'fitness', 'inlier_rmse', 'n_inliers', 'iters_run'):
            assert torch.equal(getattr(x, f), getattr(y, f)), f
    assert not torch.equal(a.pose, pose[:, :3]) and torch.equal(pose, _dev(plain[:2])), 'refined, and not in place'


def test_run_test_refine_returns_the_refined_pose_of_every_pair(plumbing):
    from regtr_amd import harness
    cfg, model, pairs, dev, plain, ids = plumbing
    want = _expected(pairs, plain)
    got, ids2, timing = harness.run_test(model, pairs, 2, dev, refine=dict(REFINE))
    assert np.array_equal(ids, ids2) and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert set(timing['refine']) == {'fitness_before', 'inlier_rmse_before', 'fitness_after', 'inlier_rmse_after'}
    with pytest.raises(ValueError):
        harness.run_test(model, pairs, 2, dev, refine=dict(REFINE, robust='huber'))
    with pytest.raises(NotImplementedError, match='raw clouds'):
        harness.run_test_shared(model, pairs, 2, dev, refine=dict(REFINE))


def _read_est(path):
    lines = open(path).read().strip().split('\n')
    return np.stack([np.array([[float(v) for v in lines[k + 1 + r].split('\t')] for r in range(3)]) for k in range(0, len(lines), 5)])


def test_cli_refine_icp_plane_writes_the_refined_poses(plumbing, tmp_path):
    cfg, model, pairs, dev, plain, _ = plumbing
    want = _expected(pairs, plain)
    ck = tmp_path / 'model.pth'
    torch.save({'state_dict': model.state_dict(), 'step': 0}, ck)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '--benchmark', '3DMatch', '--config',
                        os.path.join(ROOT, 'regtr_amd', 'conf', '3dmatch.yaml'), '--logdir', str(tmp_path / 'logs'), '--name', 't', '--resume', str(ck),
                        '--synthetic', '3', '--batch', '2', '--num_workers', '0', '--replicas', '1', '--no_warmup', '--refine', 'icp_plane',
                        '--refine_dist', str(REFINE['max_dist']), '--refine_iters', str(REFINE['iters']), '--refine_normal_radius',
                        str(REFINE['normal_radius'])], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '[Refine] icp_plane' in r.stderr or '[Refine] icp_plane' in r.stdout
    run = os.listdir(tmp_path / 'logs')[0]
    est = _read_est(tmp_path / 'logs' / run / '3DMatch' / 'synthetic-scene000' / 'est.log')
    assert est.shape == (3, 3, 4) and np.array_equal(est.astype(np.float32), want), np.abs(est - want).max()
    bad = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), '--benchmark', '3DMatch', '--config',
                          os.path.join(ROOT, 'regtr_amd', 'conf', '3dmatch.yaml'), '--logdir', str(tmp_path / 'logs2'), '--name', 't', '--resume', str(ck),
                          '--synthetic', '3', '--refine', 'icp_plane', '--share_backbone'], cwd=tmp_path, env=env, capture_output=True, text=True,
                         timeout=600)
    assert bad.returncode != 0, '--share_backbone stays refused with --refine icp_plane'
