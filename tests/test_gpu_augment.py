"""GPU: the device augmentation (regtr_amd/augment.py, csrc/augment.hip) against its numpy restatement (tests/augment_ref.py) under the
same (seed, step), its bit-exact special cases, its consistency with the device's own overlap masks, and three AdamW steps on batches it
builds.

Two batches: toy clouds of src sizes [1, 70, 300] and tgt sizes [65, 257, 64] with max_pts = 64 (truncated, untruncated and exactly-full
clouds, a one-point cloud, the 64-lane and 256-thread boundaries), and the two-pair 3DMatch crop tests/test_gpu_backbone_grads.py trains
on.  STEP is searched on the CPU so that the toy batch at (SEED, STEP) and the crop batch at (SEED, STEP + 1) show all four perturb x swap
combinations between their five pairs (pair b's draws do not depend on the batch, so the two batches take different steps)."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.util import gold, load_cfg

pytestmark = pytest.mark.gpu

SRC_N, TGT_N, MAX_PTS = [1, 70, 300], [65, 257, 64], 64
CROP = '3dmatch_crop_b2'
SEED = 20240611
RADIUS = 0.0375


def _combos(step):
    a, b = R.pair_draws(SEED, step, 3), R.pair_draws(SEED, step + 1, 2)
    return {(bool(p), bool(s)) for d in (a, b) for p, s in zip(d['perturb_source'], d['swap'])}


def _pick_step():
    for step in range(1000):
        if len(_combos(step)) == 4:
            return step
    raise AssertionError('no step under 1000 covers the four combinations')


STEP = _pick_step()
_shared = {}


def _toy():
    """Three pairs whose tgt clouds are moved, slightly displaced copies of src points (some within RADIUS of a src point, some not)."""
    rng = np.random.default_rng(5)
    srcs, tgts, poses = [], [], []
    for ns, nt in zip(SRC_N, TGT_N):
        q = rng.standard_normal(4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        pose = np.concatenate([Rm, rng.uniform(-1, 1, (3, 1))], axis=1).astype(np.float32)
        src = rng.uniform(-1, 1, (ns, 3)).astype(np.float32)
        base = src[rng.integers(0, ns, nt)].astype(np.float64) + rng.uniform(-0.04, 0.04, (nt, 3))
        tgt = (base @ pose[:, :3].astype(np.float64).T + pose[:, 3]).astype(np.float32)
        srcs.append(src); tgts.append(tgt); poses.append(pose)
    return srcs, tgts, np.stack(poses)


def _case(name):
    """Host inputs of a batch: clouds, pose (B, 3, 4), masks (seeded random for the toy batch, the golden's for the crop)."""
    if name not in _shared:
        if name == 'toy':
            srcs, tgts, pose = _toy()
            rng = np.random.default_rng(6)
            sm, tm = [rng.random(len(s)) > 0.5 for s in srcs], [rng.random(len(t)) > 0.5 for t in tgts]
        else:
            g, f = gold(f'losses_{CROP}'), gold(CROP)
            srcs, tgts, pose = [f['src_0'], f['src_1']], [f['tgt_0'], f['tgt_1']], np.asarray(g['pose'], dtype=np.float32)[:, :3]
            sm, tm = [g[f'src_mask_{b}'] for b in range(2)], [g[f'tgt_mask_{b}'] for b in range(2)]
        _shared[name] = dict(src=srcs, tgt=tgts, pose=pose, sm=sm, tm=tm)
    return _shared[name]


def _batch(c, masks=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sm, tm = masks if masks is not None else (c['sm'], c['tm'])
    return {'src_xyz': [t(s) for s in c['src']], 'tgt_xyz': [t(x) for x in c['tgt']], 'pose': t(c['pose']),
            'src_overlap': [t(m) if not isinstance(m, torch.Tensor) else m for m in sm],
            'tgt_overlap': [t(m) if not isinstance(m, torch.Tensor) else m for m in tm]}


def _np(t):
    return t.detach().cpu().numpy()


def test_step_covers_the_four_combinations():
    assert _combos(STEP) == {(x, y) for x in (False, True) for y in (False, True)}


@pytest.mark.parametrize('name,mode', [('toy', 'small'), ('toy', 'large'), ('toy', 'none'), ('crop', 'small')])
def test_equals_the_restatement(name, mode):
    from regtr_amd.augment import augment_batch
    c = _case(name)
    B = len(c['src'])
    noise = 0.005
    max_pts = MAX_PTS if name == 'toy' else 2048
    step = STEP if name == 'toy' else STEP + 1
    out = augment_batch(_batch(c), SEED, step, augment_noise=noise, perturb_pose=mode, max_pts=max_pts)
    d = R.draws(SEED, step, ([len(s) for s in c['src']], [len(t) for t in c['tgt']]), perturb_pose=mode, max_pts=max_pts)
    aug = out['_augment']
    flags = _np(aug['flags'])
    assert np.array_equal(flags[:, 0].astype(bool), d['perturb_source']) and np.array_equal(flags[:, 1].astype(bool), d['swap'])
    assert np.array_equal(_np(aug['perm']), d['perm'])
    assert list(aug['in_slot']) == list(d['in_slot'])
    assert out['pose'].shape == (B, 3, 4)
    worst = 0.0
    for b in range(B):
        pair = {'src_xyz': c['src'][b], 'tgt_xyz': c['tgt'][b], 'pose': c['pose'][b], 'src_overlap': c['sm'][b], 'tgt_overlap': c['tm'][b]}
        db = R.pair_of(d, b)
        ref = R.apply(pair, db, augment_noise=noise, perturb_pose=mode)
        bd = R.bounds(pair, db, augment_noise=noise, perturb_pose=mode, device=True)
        ins = ('tgt', 'src') if db['swap'] else ('src', 'tgt')
        for k, in_key in zip(('src', 'tgt'), ins):
            got = _np(out[f'{k}_xyz'][b]).astype(np.float64)
            assert got.shape == ref[f'{k}_xyz'].shape == (min(len(pair[f'{in_key}_xyz']), max_pts), 3)
            assert np.array_equal(_np(out[f'{k}_overlap'][b]), ref[f'{k}_overlap']) and out[f'{k}_overlap'][b].dtype is torch.bool
            tol = bd['perturbed'] if (mode != 'none' and in_key == bd['which']) else bd['other']
            err = np.abs(got - ref[f'{k}_xyz']).max()
            print(f'{name} {mode} pair {b} {k}: |device - restatement| {err:.3e} bound {tol:.3e}')
            worst = max(worst, err / tol)
            assert err <= tol, (b, k, err, tol)
        gp = _np(out['pose'][b]).astype(np.float64)
        eR, et = np.abs(gp[:, :3] - ref['pose'][:, :3]).max(), np.abs(gp[:, 3] - ref['pose'][:, 3]).max()
        print(f'{name} {mode} pair {b} pose: R {eR:.3e} bound {bd["pose_R"]:.3e}, t {et:.3e} bound {bd["pose_t"]:.3e}')
        assert eR <= bd['pose_R'] and et <= bd['pose_t'], (b, eR, et, bd)
        xf = _np(aug['xform']).astype(np.float64)
        assert np.abs(xf[b] - ref['xform_src']).max() <= bd['perturbed'] and np.abs(xf[B + b] - ref['xform_tgt']).max() <= bd['perturbed']
    print(f'{name} {mode}: largest error / bound {worst:.3f}')


def test_identity_settings_return_the_inputs_bit_for_bit():
    from regtr_amd.augment import augment_batch
    c = _case('toy')
    src = [s.copy() for s in c['src']]
    src[1][3, 0], src[2][5, 2] = -0.0, -0.0                      # a negative zero stays one
    cc = dict(c, src=src)
    out = augment_batch(_batch(cc), SEED, STEP, augment_noise=0, perturb_pose='none', shuffle=False, swap=False, max_pts=MAX_PTS)
    for k in ('src', 'tgt'):
        for b in range(3):
            want = cc[k][b][:MAX_PTS]
            assert np.array_equal(_np(out[f'{k}_xyz'][b]).view(np.uint32), want.view(np.uint32)), (k, b)
            assert np.array_equal(_np(out[f'{k}_overlap'][b]), c['sm' if k == 'src' else 'tm'][b][:MAX_PTS])
    assert np.array_equal(_np(out['pose']), c['pose']) and out['_augment']['perm'] is None
    assert not _np(out['_augment']['flags']).any()


@pytest.mark.parametrize('mode', ['small', 'large'])
def test_without_noise_the_clouds_are_se3_transform_of_the_gathered_rows(mode):
    from regtr_amd import ops
    from regtr_amd.augment import augment_batch
    from tests.util import seg_of
    c = _case('toy')
    out = augment_batch(_batch(c), SEED, STEP, augment_noise=0, perturb_pose=mode, max_pts=MAX_PTS)
    aug = out['_augment']
    lens = SRC_N + TGT_N
    off = np.concatenate([[0], np.cumsum(lens)])
    x = torch.from_numpy(np.concatenate(c['src'] + c['tgt'])).cuda()
    got = out['src_xyz'] + out['tgt_xyz']
    for co, ci in enumerate(aug['in_slot']):
        n = min(lens[ci], MAX_PTS)
        rows = aug['perm'][off[ci]:off[ci] + n]
        want = ops.se3_transform(x[rows].contiguous(), seg_of([n]), aug['xform'][ci:ci + 1])
        assert torch.equal(got[co].view(torch.int32), want.view(torch.int32)), (co, ci)


def test_same_seed_and_step_are_bitwise_reproducible_and_another_step_is_not():
    from regtr_amd.augment import augment_batch
    c = _case('toy')
    a = augment_batch(_batch(c), SEED, STEP, max_pts=MAX_PTS)
    b = augment_batch(_batch(c), SEED, STEP, max_pts=MAX_PTS)
    o = augment_batch(_batch(c), SEED, STEP + 1, max_pts=MAX_PTS)
    for k in ('src_xyz', 'tgt_xyz', 'src_overlap', 'tgt_overlap'):
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
    assert torch.equal(a['pose'].view(torch.int32), b['pose'].view(torch.int32))
    assert torch.equal(a['_augment']['perm'], b['_augment']['perm']) and not torch.equal(a['_augment']['perm'], o['_augment']['perm'])
    assert not torch.equal(a['_augment']['perm'], augment_batch(_batch(c), SEED + 1, STEP, max_pts=MAX_PTS)['_augment']['perm'])


@pytest.mark.parametrize('name', ['toy', 'crop'])
def test_masks_of_the_augmented_pair_are_the_carried_masks(name):
    """Rigid consistency on the device: without jitter, the overlap masks computed from the AUGMENTED clouds under the AUGMENTED pose
    equal the masks carried through the chain -- except where a point's nearest distance sits within 1e-5 of the radius.
    The statement needs a ground-truth pose that IS rigid: RandomSwap inverts the pose by transposing its rotation (se3_torch.py:43-48), and
    the crop golden's pose has |R^T R - I| = 2.8e-4 (measured: two of 7699 points of a swapped pair, 1.4e-4 and 3.2e-4 from the radius,
    changed sides under it), so its rotation is first replaced by the nearest orthonormal one (SVD), rounded to float32."""
    from regtr_amd.augment import augment_batch
    from regtr_amd.overlap import compute_overlap_masks
    c = _case(name)
    u, _, vt = np.linalg.svd(c['pose'][:, :, :3].astype(np.float64))
    c = dict(c, pose=np.concatenate([u @ vt, c['pose'][:, :, 3:].astype(np.float64)], axis=2).astype(np.float32))
    assert np.abs(c['pose'][:, :, :3].transpose(0, 2, 1).astype(np.float64) @ c['pose'][:, :, :3] - np.eye(3)).max() < 4 * R.U
    B = len(c['src'])
    max_pts = max(len(x) for x in c['src'] + c['tgt'])           # no truncation: it would remove supports
    assert all(len(x) <= max_pts for x in c['src'] + c['tgt'])
    near, total, dist = [], 0, []
    for b in range(B):                                           # on the CPU: who is too close to the radius to call, and the 1 % cap
        sw = c['src'][b].astype(np.float64) @ c['pose'][b][:, :3].astype(np.float64).T + c['pose'][b][:, 3]
        ds, dt = R.nearest_dist(sw, c['tgt'][b]), R.nearest_dist(c['tgt'][b], sw)
        near.append((np.abs(ds - RADIUS) <= 1e-5, np.abs(dt - RADIUS) <= 1e-5))
        total += len(ds) + len(dt)
        dist.append((ds, dt))
    n_near = sum(int(a.sum() + b_.sum()) for a, b_ in near)
    assert n_near <= 0.01 * total, (n_near, total)
    batch = _batch(c)
    sm, tm = compute_overlap_masks(batch['src_xyz'], batch['tgt_xyz'], batch['pose'], RADIUS)
    assert 0 < sum(int(m.sum()) for m in sm) < sum(len(m) for m in sm)                       # a mixed mask, or the test shows nothing
    out = augment_batch(_batch(c, masks=(sm, tm)), SEED, STEP, augment_noise=0, perturb_pose='small', max_pts=max_pts)
    sm2, tm2 = compute_overlap_masks(out['src_xyz'], out['tgt_xyz'], out['pose'], RADIUS)
    d = R.draws(SEED, STEP, ([len(s) for s in c['src']], [len(t) for t in c['tgt']]), max_pts=max_pts)
    checked = 0
    for b in range(B):
        idx = {'src': d['src_idx'][b], 'tgt': d['tgt_idx'][b]}
        ins = ('tgt', 'src') if d['swap'][b] else ('src', 'tgt')
        for k, in_key, carried, again in (('src', ins[0], out['src_overlap'][b], sm2[b]), ('tgt', ins[1], out['tgt_overlap'][b], tm2[b])):
            keep = ~near[b][0 if in_key == 'src' else 1][idx[in_key]]
            bad = (_np(carried) != _np(again)) & keep
            print(f'{name} pair {b} {k} (input {in_key}): {int(bad.sum())} of {int(keep.sum())} differ; their |d - r|:',
                  np.abs(dist[b][0 if in_key == 'src' else 1][idx[in_key]][bad] - RADIUS)[:8])
            assert np.array_equal(_np(carried)[keep], _np(again)[keep]), (b, k)
            checked += int(keep.sum())
    assert checked >= 0.99 * total


def test_no_host_sync():
    from regtr_amd.augment import augment_batch
    c = _case('toy')
    batch = _batch(c)
    augment_batch(batch, SEED, STEP, max_pts=MAX_PTS)             # first call: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = augment_batch(batch, SEED, STEP + 1, max_pts=MAX_PTS)
        out2 = augment_batch(batch, SEED, STEP + 1, perturb_pose='large', shuffle=False, max_pts=MAX_PTS)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(torch.isfinite(x).all() for x in out['src_xyz'] + out2['tgt_xyz'])


def test_refusals():
    from regtr_amd.augment import augment_batch
    c = _case('toy')
    b = _batch(c)
    b['src_xyz'][0] = torch.empty((0, 3), device='cuda')
    with pytest.raises(RuntimeError, match='empty'):
        augment_batch(b, 0, 0)
    b = _batch(c)
    b['tgt_xyz'][1] = b['tgt_xyz'][1].cpu()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        augment_batch(b, 0, 0)
    b = _batch(c)
    b['src_overlap'][2] = b['src_overlap'][2][:-1]
    with pytest.raises(RuntimeError, match='one entry per point'):
        augment_batch(b, 0, 0)


def test_three_adamw_steps_on_train_batches():
    """train_batch on the crop -> training_step(train_backbone=True) -> AdamW, three steps with step = 0, 1, 2."""
    from regtr_amd.augment import train_batch
    from tests.test_gpu_losses import _model
    c = _case('crop')
    cfg = load_cfg('3dmatch')
    model = _model(cfg, gold(f'losses_{CROP}'))
    params = model.trainable_parameters(backbone=True)
    opt = torch.optim.AdamW(params, lr=1e-4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    srcs, tgts, pose = [t(s) for s in c['src']], [t(x) for x in c['tgt']], t(c['pose'])
    for step in range(3):
        batch = train_batch(srcs, tgts, pose, cfg, SEED, step)
        lens = [int(x.shape[0]) for x in batch['src_xyz'] + batch['tgt_xyz']]
        sw = R.pair_draws(SEED, step, 2)['swap']
        want = [len(c['tgt' if sw[b] else 'src'][b]) for b in range(2)] + [len(c['src' if sw[b] else 'tgt'][b]) for b in range(2)]
        assert lens == want                                       # (the crop's clouds are below max_pts = 30000)
        opt.zero_grad(set_to_none=True)
        pred, losses = model.training_step(batch, train_backbone=True)
        losses['total'].backward()
        opt.step()
        assert all(bool(torch.isfinite(v)) for v in losses.values()), {k: float(v) for k, v in losses.items()}
        meta = batch['kpconv_meta']
        assert [int(n) for n in meta['_lens_host'][0]] == lens
        coarse = [int(n) for n in meta['_lens_host'][-1]]
        assert [int(p.shape[0]) for p in pred['src_kp']] == coarse[:2] and [int(p.shape[0]) for p in pred['tgt_kp']] == coarse[2:]
        assert all(pred['src_kp_warped'][b][5].shape == (coarse[b], 3) for b in range(2))
    assert all(torch.isfinite(p).all() for p in params)


def test_harness_train_batches_counts_steps_and_is_reproducible():
    """harness.train_batches over a synthetic pair source (one loader thread): every pair once per epoch in the order drawn from (seed,
    epoch), `step` counting up across epochs, each batch equal to augment.train_batch on the same pairs."""
    from regtr_amd.augment import train_batch
    from regtr_amd.harness import SyntheticPairs, train_batches
    cfg = load_cfg('3dmatch')
    source = SyntheticPairs(3, points=1500)
    got = list(train_batches(source, cfg, 2, SEED, epochs=2, num_workers=0))
    assert [len(b['ids']) for b in got] == [2, 1, 2, 1]
    assert sorted(got[0]['ids'] + got[1]['ids']) == sorted(got[2]['ids'] + got[3]['ids']) == [0, 1, 2]
    again = list(train_batches(source, cfg, 2, SEED, epochs=2, num_workers=0))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for step, (a, b) in enumerate(zip(got, again)):
        items = [source[i] for i in a['ids']]
        direct = train_batch([t(i['src_xyz']) for i in items], [t(i['tgt_xyz']) for i in items],
                             t(np.stack([np.asarray(i['pose'], dtype=np.float32)[:3] for i in items])), cfg, SEED, step)
        assert a['ids'] == b['ids']
        for k in ('src_xyz', 'tgt_xyz', 'src_overlap', 'tgt_overlap'):
            assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a[k], b[k], direct[k])), (step, k)
        assert torch.equal(a['pose'], b['pose']) and torch.equal(a['pose'], direct['pose'])
