"""GPU: the device ModelNet augmentation (regtr_amd/augment.py: modelnet_train_batch, csrc/augment_modelnet.hip) -- regtr_crop_select
alone against numpy, the chain against its restatement (tests/modelnet_augment_ref.py) under the same (seed, step), reproducibility, no
host synchronisation, and the overlap masks."""
import numpy as np
import pytest
import torch

from tests import modelnet_augment_ref as M
from tests.util import load_cfg

pytestmark = pytest.mark.gpu

SEED, STEP = 20240611, 3
SIZES = [2048, 300, 65]          # kept 1433 > 717 (without replacement), 210 and 45 < 717 (with)
_shared = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))).cuda()


def _select(clouds, dirs, p_keep=0.7):
    """regtr_crop_select on raw clouds with given (2B, 3) float32 directions -> numpy (centroid, thr, count, flag, keep list)."""
    from regtr_amd import ops
    from regtr_amd.augment import crop_quantile
    lens = [len(c) for c in clouds]
    B = len(lens)
    sel = [crop_quantile(n, p_keep) for n in lens] * 2
    raw_off = np.concatenate([[0], np.cumsum(lens)])
    slot_off = np.concatenate([[0], np.cumsum(lens + lens)])
    out = ops.crop_select(_dev(np.concatenate(clouds), np.float32), _dev(raw_off, np.int32), max(lens), _dev(dirs, np.float32),
                          _dev([s[0] for s in sel], np.int32), _dev([s[1] for s in sel], np.float64), _dev(slot_off, np.int32),
                          int(slot_off[-1]))
    cen, thr, count, flag, keep = (_np(o) for o in out)
    return cen, thr, count, flag, [keep[slot_off[s]:slot_off[s + 1]].astype(bool) for s in range(2 * B)]


def _quantised(rng, n):
    """Multiples of 2^-20 in [-1, 1]: float64 sums are exact in any order, so the centroid has one correct value."""
    return (rng.integers(-2 ** 20, 2 ** 20 + 1, (n, 3)) * 2.0 ** -20).astype(np.float32)


def _check_select(clouds, dirs, exact_bits=True):
    cen, thr, count, flag, keep = _select(clouds, dirs)
    B = len(clouds)
    for s in range(2 * B):
        ref = M.crop(clouds[s % B], dirs[s].astype(np.float64))
        assert np.array_equal(cen[s].view(np.uint32), ref['centroid'].view(np.uint32)), s
        if exact_bits:
            assert thr[s:s + 1].view(np.int64)[0] == np.array([ref['thr']]).view(np.int64)[0], (s, thr[s], ref['thr'])
        assert thr[s] == ref['thr'] and np.array_equal(keep[s], ref['mask']) and count[s] == ref['mask'].sum() and flag[s] == ref['flag'], s
    return thr, count, flag, keep


def test_crop_select_against_numpy_at_every_size_and_route():
    from regtr_amd import ops
    cap = ops.crop_select_lds_points()
    assert cap == 7680
    rng = np.random.default_rng(1)
    sizes = [2, 3, 64, 65, 257, 2048, cap - 1, cap, cap + 1]
    clouds = [_quantised(rng, n) for n in sizes]
    dirs = M.sphere(rng.random(2 * len(sizes)), rng.random(2 * len(sizes))).astype(np.float32)
    _, count, flag, _ = _check_select(clouds, dirs)                      # one launch: every slot takes its own route by its n
    assert not flag.any() and all(0 < count[s] < sizes[s % len(sizes)] for s in range(2 * len(sizes)))
    _check_select(clouds[-1:], dirs[:2])                                 # the global route alone (the LDS sized at its cap)
    _check_select(clouds[5:6], dirs[2:4])                                # the LDS route alone, sized by the cloud


def test_crop_select_ties_zeros_and_the_all_coincident_cloud():
    rng = np.random.default_rng(2)
    ex, ez = np.array([1, 0, 0], dtype=np.float32), np.array([0, 0, 1], dtype=np.float32)
    # heavy ties AT the threshold: x takes three values, 40 % of the rows share the middle one, which holds ranks lo and lo + 1
    n = 300
    x = np.concatenate([np.full(60, -0.5), np.full(120, 0.25), np.full(120, 0.75)])
    tie = np.stack([x, rng.integers(-8, 9, n) / 16.0, rng.integers(-8, 9, n) / 16.0], axis=1).astype(np.float32)[rng.permutation(n)]
    # +-0 distances: z is +0 or -0 or +-1 so that the centred z (centroid 0) and the distance along ez are signed zeros around the ranks
    z = np.concatenate([np.full(40, -1.0), np.full(60, -0.0), np.full(60, 0.0), np.full(40, 1.0)])
    zero = np.stack([rng.integers(-8, 9, 200) / 16.0, rng.integers(-8, 9, 200) / 16.0, z], axis=1).astype(np.float32)[rng.permutation(200)]
    same = np.tile(np.array([[0.25, -0.5, 0.125]], dtype=np.float32), (65, 1))
    thr, count, flag, keep = _check_select([tie, zero, same], np.stack([ex, ez, ex, -ex, -ez, ez]), exact_bits=False)
    cen_x = M.centroid32(tie)[0]
    assert thr[0] == np.float32(0.25) - cen_x and count[0] == 120 and not keep[0][tie[:, 0] == 0.25].any()      # strict >: the ties are dropped
    assert thr[1] == 0.0 and count[1] == 40 and thr[4] == 0.0 and count[4] == 40
    assert list(flag) == [0, 0, 1, 0, 0, 1] and count[2] == count[5] == 65 and keep[2].all() and keep[5].all()


def _clouds():
    if 'clouds' not in _shared:
        rng = np.random.default_rng(9)
        _shared['clouds'] = [rng.uniform(-0.6, 0.6, (n, 3)).astype(np.float32) for n in SIZES]
    return _shared['clouds']


def _run(step=STEP, seed=SEED, **kw):
    from regtr_amd.augment import modelnet_train_batch
    return modelnet_train_batch([_dev(c) for c in _clouds()], load_cfg('modelnet'), seed, step, **kw)


@pytest.mark.parametrize('clip', [0.05, 0.01])
def test_chain_equals_the_restatement(clip):
    cfg = load_cfg('modelnet')
    B, k = len(SIZES), M.K
    out = _run(jitter_clip=clip)
    aug = out['_augment']
    d = M.draws(SEED, STEP, SIZES, cfg.rot_mag, cfg.trans_mag)
    dirs, cen = _np(aug['dirs']), _np(aug['centroid'])
    # float64 trigonometry on both sides, possibly differing in the last place, then a float32 rounding: 2 ulp of a unit vector's entry
    assert np.abs(dirs - d['dirs']).max() <= 2 * M.U and np.abs(_np(aug['xform']) - d['transform']).max() <= 2 * M.U
    thr, count, flag, rows = _np(aug['thr']), _np(aug['count']), _np(aug['flag']), _np(aug['rows'])
    perm = _np(aug['perm'])
    n_slot_rows = aug['slot_off'][-1]
    assert not flag.any() and out['pose'].shape == (B, 3, 4)
    clipped = 0
    for b, pts in enumerate(_clouds()):
        db = M.cloud_of(d, b)
        db.update(dir_src=dirs[b].astype(np.float64), dir_ref=dirs[B + b].astype(np.float64))        # the device's own directions ...
        ref = M.apply(pts, db, jitter_clip=clip, centroids=(cen[b], cen[B + b]))                      # ... and centroids
        assert np.abs(cen[b].astype(np.float64) - pts.astype(np.float64).mean(0)).max() <= 2 * M.U * np.abs(pts).max()
        bd = M.bounds(pts, db, 0.01, clip, device=True)
        for s, slot, o in (('src', b, 'src'), ('ref', B + b, 'tgt')):
            cr = ref[f'{s}_crop']
            assert thr[slot] == cr['thr'] and count[slot] == cr['mask'].sum(), (b, s)
            assert np.array_equal(_np(aug['keep'][slot]), cr['mask']), (b, s)
            assert np.array_equal(rows[slot], ref[f'{s}_rows']), (b, s)                                # resample and shuffle, exactly
            lo2 = n_slot_rows + slot * k
            assert np.array_equal(perm[lo2:lo2 + k] - lo2, db[f'perm_{s}']), (b, s)
            assert np.array_equal(_np(out[f'{o}_overlap'][b]), ref[f'{o}_overlap']) and out[f'{o}_overlap'][b].dtype is torch.bool
            got = _np(out[f'{o}_xyz'][b]).astype(np.float64)
            assert got.shape == (k, 3)
            err = np.abs(got - ref[f'{o}_xyz']).max()
            print(f'clip {clip} cloud {b} {s}: |device - restatement| {err:.3e} bound {bd[s]:.3e}')
            assert err <= bd[s], (b, s, err, bd[s])
            clipped += int((np.abs(db[f'noise_{s}']) > clip).sum())
        ep = np.abs(_np(out['pose'][b]).astype(np.float64) - ref['pose'])
        assert ep[:, :3].max() <= bd['pose_R'] and ep[:, 3].max() <= bd['pose_t'], (b, ep.max(), bd)
        m = int(count[b])
        assert (m >= k and len(np.unique(rows[b])) == k) or (m < k and len(np.unique(rows[b])) == m)   # both regimes
    if clip == 0.01:                                                                                  # the narrow clip is exercised
        assert clipped > 100


def test_bitwise_reproducible_and_another_step_differs():
    a, b, o = _run(), _run(), _run(step=STEP + 1)
    for key in ('src_xyz', 'tgt_xyz', 'src_overlap', 'tgt_overlap'):
        assert all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    assert torch.equal(a['pose'].view(torch.int32), b['pose'].view(torch.int32))
    for key in ('perm', 'rows', 'thr', 'count'):
        assert torch.equal(a['_augment'][key], b['_augment'][key]), key
    assert not torch.equal(a['_augment']['perm'], o['_augment']['perm']) and not torch.equal(a['pose'], o['pose'])
    assert not torch.equal(a['_augment']['perm'], _run(seed=SEED + 1)['_augment']['perm'])


def test_no_host_sync():
    from regtr_amd.augment import modelnet_train_batch
    cfg = load_cfg('modelnet')
    pts = [_dev(c) for c in _clouds()]
    modelnet_train_batch(pts, cfg, SEED, STEP)                      # first call: library load, the percentile positions' cache
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = modelnet_train_batch(pts, cfg, SEED, STEP + 1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(torch.isfinite(x).all() for x in out['src_xyz'] + out['tgt_xyz'])


def test_overlap_masks_are_the_other_crop_carried_through_the_rows():
    out = _run()
    aug = out['_augment']
    B = len(SIZES)
    mixed = 0
    for b in range(B):
        for key, slot, other in (('src_overlap', b, B + b), ('tgt_overlap', B + b, b)):
            want = aug['keep'][other][aug['rows'][slot].long()]
            assert torch.equal(out[key][b], want), (b, key)
            assert bool(aug['keep'][slot][aug['rows'][slot].long()].all())          # every output row is a kept row of its own crop
            mixed += int(0 < int(want.sum()) < len(want))
    assert mixed >= 4


def test_refusals_on_the_device():
    from regtr_amd.augment import modelnet_train_batch
    cfg = load_cfg('modelnet')
    ok = _dev(_clouds()[2])
    with pytest.raises(RuntimeError, match='empty'):
        modelnet_train_batch([ok, torch.empty((0, 3), device='cuda')], cfg, 0, 0)
    with pytest.raises(RuntimeError, match='n >= 2'):
        modelnet_train_batch([ok[:1]], cfg, 0, 0)
    with pytest.raises(RuntimeError, match=r'float32 \(n, 3\)'):
        modelnet_train_batch([ok.double()], cfg, 0, 0)
    with pytest.raises(RuntimeError, match=r'float32 \(n, 3\)'):
        modelnet_train_batch([ok[:, :2]], cfg, 0, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        modelnet_train_batch([ok.cpu()], cfg, 0, 0)


def test_harness_modelnet_train_batches():
    from regtr_amd.augment import modelnet_train_batch
    from regtr_amd.harness import modelnet_train_batches
    cfg = load_cfg('modelnet')
    source = _clouds()
    got = list(modelnet_train_batches(source, cfg, 2, SEED, epochs=2))
    assert [len(b['ids']) for b in got] == [2, 1, 2, 1] and sorted(got[0]['ids'] + got[1]['ids']) == [0, 1, 2]
    for step, b in enumerate(got):
        direct = modelnet_train_batch([_dev(source[i]) for i in b['ids']], cfg, SEED, step)
        for key in ('src_xyz', 'tgt_xyz', 'src_overlap', 'tgt_overlap'):
            assert all(torch.equal(x, y) for x, y in zip(b[key], direct[key])), (step, key)
        assert torch.equal(b['pose'], direct['pose'])
