"""CPU: the numpy restatements of csrc/metrics.hip (tests/metrics_ref.py) against independent references -- the REAL reference's recorded
ModelNet metrics (tests/golden/modelnet_metrics.npz), its se3_compare and _aggregate_metrics (tests/golden/validation_metrics.npz,
tools/make_golden_validation.py), scipy's KD-tree and scipy's Euler angles -- and the header / binding agreement of the new entry points.
The GPU tests (tests/test_gpu_metrics.py) then hold the kernels to these restatements."""
import os
import re

import numpy as np
import pytest

from tests import metrics_ref as ref
from tests.util import GOLD, ROOT

U = 2.0 ** -24


def test_modelnet_metrics_restatement_matches_reference_golden():
    """The restatement on the reference's recorded inputs: the bar of tests/test_evaluation.py for this fixture."""
    from regtr_amd import evaluation as ev
    g = np.load(os.path.join(GOLD, 'modelnet_metrics.npz'))
    B = len(g['pred'])
    m = ref.modelnet_metrics(g['pred'], g['gt'], list(g['src']), list(g['ref']), list(g['raw']))
    assert sorted(m) == sorted(k[2:] for k in g.files if k.startswith('m_'))
    for k, v in m.items():
        assert v.shape == (B,)
        print(k, np.abs(v - g['m_' + k]).max())
        assert np.allclose(v, g['m_' + k], rtol=2e-4, atol=2e-6), (k, v, g['m_' + k])
    for k, v in ev.summarize_metrics({k: np.asarray(v, np.float64) for k, v in m.items()}).items():
        assert np.allclose(v, g['s_' + k], rtol=2e-4, atol=2e-6), k


def test_nearest_restatement_vs_kdtree():
    """float32 `nearest` against scipy's cKDTree in float64.  d2 within 5 * 2^-24 relative: the roundings of one subtraction per
    component (it enters d2 twice: 2u), one square, two additions (3u) over non-negative terms, and the compared operand; the index
    equal wherever the float64 nearest beats the runner-up by more than that bound on both."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(5)
    q = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    s = rng.uniform(-1, 1, (2100, 3)).astype(np.float32)
    d2, idx = ref.nearest_cloud(q, s)
    dd, ii = cKDTree(s.astype(np.float64)).query(q.astype(np.float64), k=2)
    want = dd[:, 0] ** 2
    rel = np.abs(d2.astype(np.float64) - want) / want
    bound = 5 * U
    unique = dd[:, 1] ** 2 * (1 - bound) > want * (1 + bound)       # the float32 order of the two cannot differ from the float64 one
    print(f'nearest vs cKDTree: worst relative {rel.max():.2e} (bound {bound:.2e}), indices equal {np.mean(idx == ii[:, 0]):.4f}, '
          f'unique {unique.mean():.4f}')
    assert rel.max() <= bound
    assert unique.mean() > 0.99 and np.array_equal(idx[unique], ii[unique, 0])


def test_nearest_restatement_ties_nan_and_poses():
    g = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    s = np.concatenate([g, g])                                       # every point twice: the first copy must win
    q = np.array([[0.5, 0.5, 0.5], [1, 1, 1], [2, 0.5, 0]], np.float32)
    d2, idx = ref.nearest_cloud(q, s)
    assert idx.tolist() == [0, 13, 18] and d2.tolist() == [0.75, 0.0, 0.25]
    s2 = s.copy()
    s2[13] = np.nan
    d2, idx = ref.nearest_cloud(q, s2)
    assert idx.tolist() == [0, 13 + 27, 18]
    d2, idx = ref.nearest_cloud(q, np.full((2, 3), np.nan, np.float32))
    assert np.all(np.isinf(d2)) and idx.tolist() == [-1, -1, -1]
    T = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32)
    d2p, idxp = ref.nearest(q, [0, 3], s, [0, 54], q_pose=T[None], s_pose=T[None])
    d2, idx = ref.nearest_cloud(q, s)
    assert np.array_equal(idxp, idx) and np.array_equal(d2p, d2)     # an exact rigid motion of both sides changes nothing


def test_euler_closed_form_vs_scipy():
    """a = atan2(R21, R22), b = -asin(R20), c = atan2(R10, R00) against Rotation.as_euler('xyz') on float32-rounded matrices, |pitch| <= 60
    degrees.  Bar 1e-4 degrees: an entry is off by 2^-24, the angles' sensitivity to an entry is 1 / cos b <= 2, and scipy (which
    re-orthonormalises its input) is off by as much again: 4 * 2^-24 rad = 1.4e-5 degrees, with an order of magnitude to spare."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(9)
    n = 20000
    ang = np.stack([rng.uniform(-180, 180, n), rng.uniform(-60, 60, n), rng.uniform(-180, 180, n)], 1)
    R = Rotation.from_euler('xyz', ang, degrees=True).as_matrix().astype(np.float32).astype(np.float64)
    want = Rotation.from_matrix(R).as_euler('xyz', degrees=True)
    got = ref._euler_xyz_deg(R)
    err = np.abs((got - want + 180.0) % 360.0 - 180.0)
    print(f'euler closed form vs scipy: worst {err.max():.2e} degrees')
    assert err.max() <= 1e-4


def test_se3_compare_and_aggregate_vs_reference_golden():
    """tests/golden/validation_metrics.npz holds the outputs of the reference's se3_compare (float32 torch) and _aggregate_metrics on
    seeded (L = 2, B = 5) poses of two steps.  The float64 restatement meets them within float32's error: the rotation error comes from
    acos of a float32 trace (error 4 * 2^-24 through 1 / sin(angle), angle >= 0.1 degree here: 0.01 degrees), the translation from
    float32 sums of terms below 1 (1e-6); aggregate is exact given the same float32 inputs."""
    g = np.load(os.path.join(GOLD, 'validation_metrics.npz'))
    steps = []
    for s in range(int(g['n_steps'])):
        m = ref.compute_metrics(g[f'pred_{s}'], g[f'gt_{s}'])
        assert m['rot_err_deg'].shape == (2, 5) and m['rot_err_deg'].dtype == np.float32
        er, et = np.abs(m['rot_err_deg'] - g[f'rot_err_deg_{s}']).max(), np.abs(m['trans_err'] - g[f'trans_err_{s}']).max()
        print(f'step {s}: rot {er:.2e} deg, trans {et:.2e}')
        assert er <= 1e-2 and et <= 1e-6
        steps.append({'rot_err_deg': g[f'rot_err_deg_{s}'], 'trans_err': g[f'trans_err_{s}']})
    agg = ref.aggregate(steps, float(g['thresh_rot']), float(g['thresh_trans']))
    assert sorted(agg) == list(g['agg_keys'])
    for k, v in agg.items():
        want = g['agg_' + k]
        if k.endswith('hist') or k.startswith('reg_success'):
            assert np.array_equal(v, want), k
        else:
            assert np.allclose(v, want, rtol=4 * U, atol=0), k      # a float32 mean of ten values, any summation order
    # the fixture has pairs on either side of both thresholds
    rot, trans = g['agg_rot_err_final_hist'], g['agg_trans_err_final_hist']
    assert (rot < 10).any() and (rot >= 10).any() and (trans < 0.1).any() and (trans >= 0.1).any()
    assert 0 < float(g['agg_reg_success_final']) < 1


def test_device_aggregate_matches_restatement_on_cpu_tensors():
    """regtr_amd.metrics.aggregate is plain tensor code: on CPU tensors it equals the reference's recorded dict."""
    import torch
    from regtr_amd import metrics
    g = np.load(os.path.join(GOLD, 'validation_metrics.npz'))
    steps = [{'rot_err_deg': torch.from_numpy(g[f'rot_err_deg_{s}']), 'trans_err': torch.from_numpy(g[f'trans_err_{s}'])}
             for s in range(int(g['n_steps']))]
    agg = metrics.aggregate(steps, float(g['thresh_rot']), float(g['thresh_trans']))
    assert sorted(agg) == list(g['agg_keys'])
    for k, v in agg.items():
        assert torch.equal(v, torch.from_numpy(np.asarray(g['agg_' + k]))), k
    assert metrics.aggregate([], 10, 0.1) == {} and metrics.aggregate([{}], 10, 0.1) == {}


def test_header_and_bindings_declare_the_metrics_entry_points():
    from regtr_amd import _lib, ops
    header = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    for name in ('regtr_nearest', 'regtr_nearest_lds_points', 'regtr_segment_mean', 'regtr_pose_metrics'):
        assert re.search(r'^int %s\(' % name, header, re.M), name
        assert name in _lib.SIGNATURES
    assert re.search(r'#define\s+REGTR_ABI_VERSION\s+11\b', header) and _lib.ABI_VERSION == 11
    src = open(os.path.join(ROOT, 'regtr_amd', 'csrc', 'metrics.hip')).read()
    threads = int(re.search(r'constexpr int NR_THREADS = (\d+);', src).group(1))
    qpt = int(re.search(r'constexpr int NR_QPT = (\d+);', src).group(1))
    assert ops.NEAREST_QUERY_TILE == threads * qpt
    from regtr_amd import build
    assert 'metrics.hip' in build.SOURCES and '-ffp-contract=off' in build.EXTRA['metrics.hip']


def test_modelnet_metrics_names_the_missing_key():
    from regtr_amd import metrics
    with pytest.raises(KeyError, match='tgt_raw'):
        metrics.modelnet_metrics(None, {'src_xyz': [], 'tgt_xyz': [], 'pose': None})
