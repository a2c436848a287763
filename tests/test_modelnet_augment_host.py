"""CPU: the ModelNet training augmentation's restatement (tests/modelnet_augment_ref.py) against the REAL reference chain's recorded run
(tests/golden/modelnet_augment_ref_chain.npz, tools/make_golden_modelnet_augment.py), the statistics of the Philox draws, the kept
count, and the host side of regtr_amd.augment.modelnet_train_batch."""
import numpy as np
import pytest
import torch

from tests import augment_ref as A
from tests import modelnet_augment_ref as M
from tests.util import gold, load_cfg

KEYS = ('dir_src', 'dir_ref', 'transform', 'src_rand_idx', 'ref_rand_idx', 'noise_src', 'noise_ref', 'perm_src', 'perm_ref')


def _cases():
    g = gold('modelnet_augment_ref_chain')
    for c in range(int(g['n_cases'])):
        yield c, g, g[f'points_{c}'], {k: g[f'{k}_{c}'] for k in KEYS}


def test_restatement_equals_the_recorded_reference_chain():
    """apply(recorded decisions), cropping with the recorded float32 centroid, equals the reference's outputs: crop masks, overlap masks
    and lengths exactly, clouds and pose within the derived float32 bound.  Pins the crop's percentile, the Euler order, the resample's
    indexing of the cropped cloud and the shuffle's order (the reference cloud's permutation is drawn first)."""
    for c, g, pts, d in _cases():
        cen = g[f'centroid_{c}']
        out = M.apply(pts, d, p_keep=float(g['p_keep']), jitter_clip=float(g['jitter_clip']), noise_on_output=False, centroids=(cen, cen))
        bd = M.bounds(pts, d, float(g['jitter_scale']), float(g['jitter_clip']))
        for s, o in (('src', 'src'), ('ref', 'tgt')):
            assert np.array_equal(out[f'{s}_mask'], g[f'{s}_mask_{c}']), (c, s)
            assert np.array_equal(out[f'{o}_overlap'], g[f'out_{s}_overlap_{c}']), (c, s)
            assert out[f'{o}_xyz'].shape == g[f'out_{s}_{c}'].shape == (M.K, 3)
            err = np.abs(out[f'{o}_xyz'] - g[f'out_{s}_{c}'].astype(np.float64)).max()
            print(f'case {c} {s}: |restatement - reference| {err:.3e} bound {bd[s]:.3e}')
            assert err <= bd[s], (c, s, err, bd[s])
        ep = np.abs(out['pose'] - g[f'out_pose_{c}'].astype(np.float64))
        assert ep[:, :3].max() <= bd['pose_R'] and ep[:, 3].max() <= bd['pose_t'], (c, ep.max(), bd)
        # the recorded angles give the recorded transform: Rx Ry Rz, to the float32 rounding of a last-place float64 difference
        T = M.euler_transform(g[f'angles_{c}'], g[f'transform_{c}'][:, 3].astype(np.float64))
        assert np.abs(T - g[f'transform_{c}']).max() <= A.U * 1.001
        # np.percentile itself gives the restatement's threshold
        for s in ('src', 'ref'):
            cr = out[f'{s}_crop']
            assert cr['thr'] == np.percentile(cr['dist'], M.crop_q(float(g['p_keep']))) and not cr['flag']


def test_fixture_covers_the_cases_and_keeps_the_threshold_margin():
    sizes, kept = [], []
    for c, g, pts, d in _cases():
        sizes.append(len(pts))
        cen = g[f'centroid_{c}']
        e = M.dist_bound(pts, same_centroid=True)
        for s in ('src', 'ref'):
            cr = M.crop(pts, d[f'dir_{s}'], float(g['p_keep']), centroid=cen)
            assert np.abs(cr['dist'] - cr['thr']).min() > 2 * e, (c, s)
            kept.append((len(pts), int(cr['mask'].sum())))
        assert len(d['src_rand_idx']) == len(d['ref_rand_idx']) == M.K == 717
    assert len(sizes) >= 8 and sizes.count(2048) >= 2 and any(n % 2 for n in sizes)
    assert any(n == 2048 and m > M.K for n, m in kept) and any(250 <= n <= 350 and m < M.K for n, m in kept)
    for c, g, pts, d in _cases():                                    # below k: every kept row once, then picks; above: distinct rows
        m = int(g[f'src_mask_{c}'].sum())
        idx = d['src_rand_idx']
        assert len(np.unique(idx)) == min(m, M.K) and (m >= M.K or sorted(idx[:m]) == list(range(m)))


def test_statistics_of_the_draws():
    steps = 10000
    dirs, ang, tr, picks = [], [], [], []
    for step in range(0, steps, 100):                                # 100 batches of 100 clouds: 10^4 draws of each kind
        q, a, t = (A.words(7, step, np.full(100, blk), np.arange(100), 3) for blk in (0, 1, 2))
        dirs.append(M.sphere(A.uniform(q[:, 0]), A.uniform(q[:, 1])))
        dirs.append(M.sphere(A.uniform(q[:, 2]), A.uniform(q[:, 3])))
        ang.append(A.uniform(a[:, :3]) * np.pi * 45.0 / 180.0)
        tr.append(-0.5 + 1.0 * A.uniform(t[:, :3]))
        picks.append(A.words(7, step, np.arange(100), np.full(100, 3), 5)[:, 0] % np.uint32(210))
    dirs, ang, tr, picks = np.concatenate(dirs), np.concatenate(ang), np.concatenate(tr), np.concatenate(picks)
    n = len(dirs)
    assert np.abs(np.linalg.norm(dirs, axis=1) - 1).max() < 1e-12
    # uniform on the sphere: mean 0 (component variance 1/3: 5 sigma = 5 sqrt(1/3n)), second moments I/3 (variance of x^2 is 4/45)
    assert np.abs(dirs.mean(0)).max() < 5 * np.sqrt(1 / (3 * n))
    assert np.abs(dirs.T @ dirs / n - np.eye(3) / 3).max() < 5 * np.sqrt(4 / (45 * n))
    assert ang.min() >= 0 and ang.max() < np.pi * 45.0 / 180.0 and abs(ang.mean() - np.pi / 8) < 5 * (np.pi / 4) / np.sqrt(12 * ang.size)
    assert tr.min() > -0.5 and tr.max() < 0.5 and abs(tr.mean()) < 5 / np.sqrt(12 * tr.size)
    # with-replacement picks among m = 210 rows: chi-square against uniform, 209 degrees of freedom (mean 209, sd 20.4): 5 sd
    cnt = np.bincount(picks, minlength=210)
    chi = ((cnt - len(picks) / 210) ** 2 / (len(picks) / 210)).sum()
    assert picks.max() < 210 and chi < 209 + 5 * np.sqrt(2 * 209), chi


@pytest.mark.parametrize('n', [2, 3, 64, 65, 257, 300, 2047, 2048, 7681])
def test_kept_count_on_tie_free_clouds(n):
    from regtr_amd.augment import crop_quantile
    rng = np.random.default_rng(n)
    pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    cr = M.crop(pts, M.sphere(rng.random(), rng.random()), 0.7)
    assert len(np.unique(cr['dist'])) == n
    q = float(M.crop_q(0.7))
    assert int(cr['mask'].sum()) == n - 1 - int(np.floor((n - 1) * q / 100))
    assert crop_quantile(n, 0.7) == M.quantile_pos(n, 0.7)
    lo, t = M.quantile_pos(n, 0.7)
    assert lo + t == pytest.approx((n - 1) * q / 100, rel=1e-12) and cr['thr'] == np.percentile(cr['dist'], M.crop_q(0.7))


def test_resample_rows_regimes():
    rng = np.random.default_rng(0)
    for n, k in ((2048, 717), (300, 717), (10, 10)):
        mask = rng.random(n) < 0.7
        m = int(mask.sum())
        rows = M.resample_rows(mask, rng.integers(0, 2 ** 31, n), rng.integers(0, 2 ** 32, k), k)
        assert mask[rows].all() and len(rows) == k
        assert len(np.unique(rows[:min(m, k)])) == min(m, k)


def test_host_side_refusals_and_build_listing():
    from regtr_amd import augment, build
    assert 'augment_modelnet.hip' in build.SOURCES and build.EXTRA['augment_modelnet.hip'] == ['-ffp-contract=off']
    cfg = load_cfg('modelnet')
    assert cfg.partial == [0.7, 0.7] and cfg.num_points == 1024 and cfg.noise_type == 'crop' and cfg.rot_mag == 45.0 and cfg.trans_mag == 0.5
    x = torch.rand(10, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        augment.modelnet_train_batch([x], cfg, 0, 0)
    with pytest.raises(RuntimeError, match='non-empty'):
        augment.modelnet_train_batch([], cfg, 0, 0)
    for key, val in (('noise_type', 'jitter'), ('noise_type', 'clean'), ('partial', [0.7]), ('partial', [0.5, 0.5])):
        bad = {k: cfg[k] for k in ('partial', 'num_points', 'rot_mag', 'trans_mag', 'noise_type')}
        bad[key] = val
        with pytest.raises(NotImplementedError, match=str(val if key == 'noise_type' else val[0])):
            augment.modelnet_train_batch([x], bad, 0, 0)
