"""GPU: the metric kernels of csrc/metrics.hip against the numpy restatements of tests/metrics_ref.py (which tests/test_metrics_host.py
pins to the reference's recorded outputs, scipy's KD-tree and scipy's Euler angles), regtr_amd.metrics against the reference's recorded
ModelNet metrics and the host function regtr_amd.evaluation.modelnet_metrics, and RegTR.validation_step / validation_epoch_end /
test_step.  Shapes are the smallest that reach every path: one lane, a wave +- 1, a query tile +- 1, a support tile +- 1, two tiles + 1."""
import numpy as np
import pytest
import torch

from tests import metrics_ref as ref
from tests.util import gold, load_cfg, seeded_sd

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
CHAMFER_BAR = 5 * U + 1e-14      # relative, against the float64 host function: 5 * 2^-24 = 3.0e-7 (the float32 distance arithmetic) + its rounding
EULER_BAR = 1e-4        # degrees per angle against scipy at |pitch| <= 60 degrees (tests/test_metrics_host.py derives it)


def _dev(x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t if dt is None else t.to(dt)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def _pose(rng, max_deg=45.0, t=0.5):
    return np.concatenate([_rot(rng.standard_normal(3), rng.uniform(0, max_deg)), rng.uniform(-t, t, (3, 1))], 1).astype(F32)


def _offsets(lens):
    return [0] + np.cumsum(lens).tolist()


# ---------------------------------------------------------------------------------------------------- regtr_nearest
def _nearest_groups():
    from regtr_amd import ops
    T, Q = ops.nearest_lds_points(), ops.NEAREST_QUERY_TILE
    return [[(1, 1), (63, 2), (64, 63)], [(65, 65), (Q - 1, T - 1), (Q, T)], [(Q + 1, T + 1), (5, 2 * T + 1), (Q + 2, 2 * T + 1)]]


@pytest.mark.parametrize('group', [0, 1, 2])
@pytest.mark.parametrize('poses', ['none', 'q', 's', 'both'])
def test_nearest_bit_for_bit(group, poses):
    """d2 and idx equal the float32 restatement bit for bit on three ragged clouds; a second run gives the same bits."""
    from regtr_amd import ops
    lens = _nearest_groups()[group]
    rng = np.random.default_rng(100 + group)
    q = rng.uniform(-1, 1, (sum(a for a, _ in lens), 3)).astype(F32)
    s = rng.uniform(-1, 1, (sum(b for _, b in lens), 3)).astype(F32)
    q_off, s_off = _offsets([a for a, _ in lens]), _offsets([b for _, b in lens])
    qp = np.stack([_pose(rng) for _ in lens]) if poses in ('q', 'both') else None
    sp = np.stack([_pose(rng) for _ in lens]) if poses in ('s', 'both') else None
    want_d2, want_idx = ref.nearest(q, q_off, s, s_off, qp, sp)
    args = (_dev(q), q_off, _dev(s), s_off, None if qp is None else _dev(qp), None if sp is None else _dev(sp))
    d2, idx = ops.nearest(*args)
    d2b, idxb = ops.nearest(*args)
    assert torch.equal(d2, d2b) and torch.equal(idx, idxb)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), want_d2.view(np.uint32))
    d2_only, none = ops.nearest(*args, return_idx=False)
    assert none is None and torch.equal(d2_only, d2)


def test_nearest_ties_take_the_lowest_index_and_nan_never_wins():
    """An integer-grid support with every point present three times, spread over two support tiles: every query has exact ties and the
    lowest index must win; one support row set to NaN is never chosen."""
    from regtr_amd import ops
    T = ops.nearest_lds_points()
    g = np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing='ij'), -1).reshape(-1, 3).astype(F32)      # 729 points
    s = np.concatenate([g, g, g, g])[:T + 700]                                                          # copies straddle the tile
    rng = np.random.default_rng(3)
    q = np.concatenate([g[40:41], g[rng.permutation(len(g))[:300]], rng.integers(0, 17, (500, 3)).astype(F32) / 2])   # on points and between them
    for nan_row in (None, 40):
        s2 = s.copy()
        if nan_row is not None:
            s2[nan_row] = np.nan
        want_d2, want_idx = ref.nearest_cloud(q, s2)
        d2, idx = ops.nearest(_dev(q), [0, len(q)], _dev(s2), [0, len(s2)])
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(d2.cpu().numpy(), want_d2)
        if nan_row is None:
            assert want_idx.max() < len(g) and want_idx[0] == 40                     # always the first copy
        else:
            assert not np.any(want_idx == nan_row) and want_idx[0] == nan_row + len(g)      # the query on the NaN row went to its next copy
    d2, idx = ops.nearest(_dev(q[:5]), [0, 5], _dev(np.full((3, 3), np.nan, F32)), [0, 3])
    assert torch.isinf(d2).all() and (idx == -1).all()


def test_refusals():
    from regtr_amd import ops
    q, s = torch.zeros((4, 3), device='cuda'), torch.zeros((6, 3), device='cuda')
    with pytest.raises(RuntimeError):
        ops.nearest(q.cpu(), [0, 4], s, [0, 6])
    with pytest.raises(RuntimeError):
        ops.nearest(q, [0, 4], s.cpu(), [0, 6])
    with pytest.raises(RuntimeError):
        ops.nearest(q.double(), [0, 4], s, [0, 6])
    with pytest.raises(RuntimeError):
        ops.nearest(q, [0, 4], s.half(), [0, 6])
    with pytest.raises(RuntimeError):
        ops.nearest(torch.zeros((4, 4), device='cuda'), [0, 4], s, [0, 6])
    with pytest.raises(RuntimeError):
        ops.nearest(q, [0, 4], torch.zeros(18, device='cuda'), [0, 6])
    with pytest.raises(RuntimeError):
        ops.nearest(q, [0, 2, 4], s, [0, 6])                    # offset vectors of different lengths
    with pytest.raises(RuntimeError):
        ops.nearest(q, [0, 2, 4], s, [0, 6, 6])                 # an empty support cloud
    with pytest.raises(RuntimeError):
        ops.nearest(q, [0, 2, 4], s, [0, 0, 6])
    with pytest.raises(RuntimeError):
        ops.nearest(q, [0, 3], s, [0, 6])                       # offsets that do not cover the cloud
    with pytest.raises(RuntimeError):
        ops.segment_mean(torch.zeros(4), torch.tensor([0, 4], dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.pose_metrics(torch.zeros((2, 3, 4)), torch.zeros((2, 3, 4)))
    with pytest.raises(RuntimeError):
        ops.pose_metrics(torch.zeros((2, 3, 4), device='cuda'), torch.zeros((3, 3, 4), device='cuda'))
    d2, idx = ops.nearest(torch.zeros((0, 3), device='cuda'), [0, 0], s, [0, 6])        # no query: nothing to do
    assert d2.shape == (0,) and idx.shape == (0,)


# ---------------------------------------------------------------------------------------------------- regtr_segment_mean
def test_segment_mean_vs_float64():
    from regtr_amd import ops
    lens = [1, 255, 256, 257, 0, 5000]
    rng = np.random.default_rng(4)
    v = np.abs(rng.standard_normal(sum(lens)) * np.exp(rng.uniform(-6, 6, sum(lens)))).astype(F32)      # squared distances: non-negative
    off = _offsets(lens)
    want = ref.segment_mean(v, off)
    # float64 sums of non-negative float32 values in another order: n * 2^-53 relative at most (5000 * 1.1e-16 = 5.6e-13); bar 1e-12
    scale = np.where(want > 0, want, 1.0)
    dv, doff = _dev(v), _dev(np.asarray(off, np.int32))
    got = ops.segment_mean(dv, doff)
    assert got.dtype == torch.float64 and torch.equal(got, ops.segment_mean(dv, doff))
    err = np.abs(got.cpu().numpy() - want) / scale
    print('segment_mean relative error per length', dict(zip(lens, err)))
    assert err.max() <= 1e-12 and got[4].item() == 0.0


# ---------------------------------------------------------------------------------------------------- regtr_pose_metrics
def _pose_cases():
    """L = 2, B = 5: general poses, pred == gt exactly (a general pose: the float32 matrix is a rotation only to rounding, so the error
    is that of the matrix, the same on both sides; and an exact quarter turn, where the arithmetic is exact and every error must be 0)
    and a 179 degree error."""
    rng = np.random.default_rng(8)
    gt = np.stack([_pose(rng) for _ in range(5)])
    gt[1, :, :3] = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    gt[1, :, 3] = [0.25, -0.5, 0.125]
    pred = np.stack([np.stack([_pose(rng) for _ in range(5)]) for _ in range(2)])
    pred[0, 0] = gt[0]
    pred[:, 1] = gt[1]
    E = np.concatenate([_rot([1, 2, 3], 179.0), [[0.1], [0.2], [-0.1]]], 1)
    pred[1, 2] = np.concatenate([E[:, :3] @ gt[2][:, :3], E[:, :3] @ gt[2][:, 3:] + E[:, 3:]], 1).astype(F32)
    return pred.astype(F32), gt.astype(F32)


@pytest.mark.parametrize('gt_rows', [3, 4])
def test_pose_metrics_vs_restatement(gt_rows):
    """Rotation errors within 1e-5 degrees (a float64 trace error of 1e-15 through acos near 1 is sqrt(2e-15) rad = 2.6e-6 degrees),
    everything else within 1e-12 relative (the Euler terms included: in these cases the angle differences are exactly 0 or of the order
    of degrees, so a few ulp of an angle below 180 degrees stay far below 1e-12 of them)."""
    from regtr_amd import ops
    pred, gt = _pose_cases()
    want, want_comp = ref.pose_metrics(pred, gt)
    g = gt if gt_rows == 3 else np.concatenate([gt, np.tile(np.array([[[0, 0, 0, 1]]], F32), (5, 1, 1))], 1)
    out, comp = ops.pose_metrics(_dev(pred), _dev(g))
    out2, comp2 = ops.pose_metrics(_dev(pred), _dev(g))
    assert torch.equal(out, out2) and torch.equal(comp, comp2)
    out, comp = out.cpu().numpy(), comp.cpu().numpy()
    assert out.shape == (2, 5, 8) and comp.shape == (2, 5, 3, 4)
    for c in (0, 2):
        assert np.abs(out[..., c] - want[..., c]).max() <= 1e-5, c
    for c in (1, 3, 4, 5, 6, 7):
        rel = np.abs(out[..., c] - want[..., c]) / np.where(want[..., c] != 0, np.abs(want[..., c]), 1.0)
        print(f'pose_metrics column {c}: worst relative error {rel.max():.2e}')
        assert np.all(np.abs(out[..., c] - want[..., c]) <= 1e-12 * np.abs(want[..., c])), c
    assert np.allclose(comp, want_comp, rtol=0, atol=2 * U)
    assert np.all(out[:, 1] == 0.0) and np.array_equal(comp[:, 1], np.tile(np.eye(3, 4, dtype=F32), (2, 1, 1)))      # exact pose: all 0
    assert np.all(out[0, 0, 4:] == 0.0) and out[0, 0, 0] < 0.1 and out[0, 0, 1] < 1e-6                                # pred == gt
    assert abs(out[1, 2, 0] - 179.0) < 1e-3 and abs(out[1, 2, 2] - 179.0) < 1e-3
    single, comp1 = ops.pose_metrics(_dev(pred[1]), _dev(g))
    assert np.array_equal(single.cpu().numpy(), out[1]) and np.array_equal(comp1.cpu().numpy(), comp[1])


# ---------------------------------------------------------------------------------------------------- metrics.modelnet_metrics
def _modelnet_batch(src, refc, raw, gt):
    return {'src_xyz': [_dev(x) for x in src], 'tgt_xyz': [_dev(x) for x in refc], 'tgt_raw': [_dev(x) for x in raw], 'pose': _dev(gt)}


def test_modelnet_metrics_vs_reference_golden():
    """The reference's own recorded outputs (float32 torch), at the bar tests/test_evaluation.py holds the host function to."""
    from regtr_amd import metrics
    g = gold('modelnet_metrics')
    m = metrics.modelnet_metrics(_dev(g['pred']), _modelnet_batch(g['src'], g['ref'], g['raw'], g['gt']))
    assert tuple(m) == metrics.MODELNET_KEYS
    for k, v in m.items():
        assert v.shape == (4,) and v.is_cuda
        assert np.allclose(v.cpu().numpy(), g['m_' + k], rtol=2e-4, atol=2e-6), (k, v, g['m_' + k])
    for k, v in metrics.summarize(m).items():
        assert np.allclose(v.item(), g['s_' + k], rtol=2e-4, atol=2e-6), k
    want = ref.chamfer(list(g['src']), list(g['ref']), list(g['raw']), g['pred'], g['gt'])
    assert np.array_equal(m['chamfer_dist'].cpu().numpy(), want)                     # the restatement, bit for bit
    ch = metrics.chamfer([_dev(x) for x in g['src']], [_dev(x) for x in g['ref']], [_dev(x) for x in g['raw']], _dev(g['pred']), _dev(g['gt']))
    assert torch.equal(ch, m['chamfer_dist']) and ch.dtype == torch.float32


def _check_vs_host(m, pred, gt, src, refc, raw):
    """Device metrics against regtr_amd.evaluation.modelnet_metrics (float64 numpy, scipy) on the same float32 poses.
    err_r_deg: 1e-5 degrees; err_t, t_mse, t_mae: 1e-12 relative; r_mae: both sides' Euler angles within EULER_BAR of each other (scaled
    by 0.5 / cos(pitch) beyond 60 degrees of pitch) -> 2 bars; r_mse: 2 |de|max 2 bars + (2 bars)^2; chamfer: CHAMFER_BAR relative."""
    from regtr_amd import evaluation as ev
    B = len(src)
    host = [ev.modelnet_metrics(pred[b:b + 1], gt[b:b + 1], src[b][None], refc[b][None], raw[b][None]) for b in range(B)]
    host = {k: np.concatenate([h[k] for h in host]) for k in host[0]}
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in m.items()}
    rep = {k: float(np.abs(got[k] - host[k]).max()) for k in host}
    rep['chamfer_rel'] = float((np.abs(got['chamfer_dist'] - host['chamfer_dist']) / host['chamfer_dist']).max())
    print('device vs host metrics, worst absolute difference:', {k: f'{v:.2e}' for k, v in rep.items()})
    assert np.abs(got['err_r_deg'] - host['err_r_deg']).max() <= 1e-5
    for k in ('err_t', 't_mse', 't_mae'):
        assert np.all(np.abs(got[k] - host[k]) <= 1e-12 * np.abs(host[k])), k
    pitch = np.maximum(np.abs(np.arcsin(np.clip(pred[:, 2, 0], -1, 1))), np.abs(np.arcsin(np.clip(gt[:, 2, 0], -1, 1))))
    bar = EULER_BAR * np.maximum(1.0, 0.5 / np.cos(pitch))
    de = np.sqrt(3 * host['r_mse'])                                                   # >= the largest angle difference
    assert np.all(np.abs(got['r_mae'] - host['r_mae']) <= 2 * bar), (got['r_mae'], host['r_mae'])
    assert np.all(np.abs(got['r_mse'] - host['r_mse']) <= 2 * de * 2 * bar + (2 * bar) ** 2)
    assert np.all(np.abs(got['chamfer_dist'] - host['chamfer_dist']) <= CHAMFER_BAR * host['chamfer_dist']), rep


def _quarter_turn_pose(rng):
    """Rz(90 c) Rx(90 a) with a translation on the 2^-10 grid: exact in float32, pitch 0."""
    a, c = rng.choice([0, 1, 3], 2)                          # (no half turn: atan2 gives +180 where another convention gives -180)
    R = np.rint(_rot([0, 0, 1], 90.0 * c) @ _rot([1, 0, 0], 90.0 * a)) + 0.0      # (+ 0.0: no negative zero)
    return np.concatenate([R, rng.integers(-512, 513, (3, 1)) / 1024.0], 1).astype(F32)


def test_modelnet_metrics_vs_host_function_exact_transforms():
    """Three ragged pairs (200 - 2100 points) on the 2^-10 grid under quarter-turn poses: every transformed coordinate is exact in
    float32 and in float64, so the two sides differ by the float32 distance arithmetic alone: every min d2 within 5 * 2^-24 relative
    (tests/test_metrics_host.py), hence their means.  Measured: 2.5e-8."""
    from regtr_amd import metrics
    rng = np.random.default_rng(21)
    lens = [(200, 717, 2100), (717, 333, 2048), (1025, 900, 1300)]
    cloud = lambda n: (rng.integers(-1024, 1025, (n, 3)) / 1024.0).astype(F32)
    src, refc, raw = [cloud(a) for a, _, _ in lens], [cloud(b) for _, b, _ in lens], [cloud(c) for _, _, c in lens]
    pred, gt = np.stack([_quarter_turn_pose(rng) for _ in lens]), np.stack([_quarter_turn_pose(rng) for _ in lens])
    m = metrics.modelnet_metrics(_dev(pred), _modelnet_batch(src, refc, raw, gt))
    _check_vs_host(m, pred, gt, src, refc, raw)


def test_modelnet_metrics_vs_host_function_general_poses():
    """Three ragged pairs under general poses (pitch below 45 degrees), Chamfer within CHAMFER_BAR.  That bar covers the distance
    arithmetic alone, while the device also transforms the clouds in float32 (as the reference does) where the host function works in
    float64; the means over hundreds of points absorb that: measured 1.4e-7 relative."""
    from regtr_amd import metrics
    rng = np.random.default_rng(22)
    lens = [(200, 717, 2100), (717, 333, 2048), (1025, 900, 1300)]
    cloud = lambda n: rng.uniform(-1, 1, (n, 3)).astype(F32)
    src, refc, raw = [cloud(a) for a, _, _ in lens], [cloud(b) for _, b, _ in lens], [cloud(c) for _, _, c in lens]
    pred, gt = np.stack([_pose(rng) for _ in lens]), np.stack([_pose(rng) for _ in lens])
    m = metrics.modelnet_metrics(_dev(pred), _modelnet_batch(src, refc, raw, gt))
    _check_vs_host(m, pred, gt, src, refc, raw)


# ---------------------------------------------------------------------------------------------------- RegTR.validation_step
def _close_metrics(got, want):
    """(L, B) float32 device results against the restatement's float32: the float64 values agree to 1e-5 degrees / 1e-12 relative, and
    rounding each to float32 can then land on neighbouring numbers."""
    for k, bar in (('rot_err_deg', 1e-5), ('trans_err', 0.0)):
        g, w = got[k].cpu().numpy(), want[k]
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.all(np.abs(g.astype(np.float64) - w) <= bar + np.spacing(np.abs(w))), k


def test_validation_step_and_epoch_end():
    from tests.test_gpu_losses import _golden_batch, _model
    case = '3dmatch_crop_b2'
    g = gold(f'losses_{case}')
    cfg = load_cfg('3dmatch')
    model = _model(cfg, g)
    srcs, tgts, extra = _golden_batch(g, case)

    def batch_of(pairs):
        b = {'src_xyz': [_dev(srcs[i]) for i in pairs], 'tgt_xyz': [_dev(tgts[i]) for i in pairs], 'pose': extra['pose'][pairs],
             'src_overlap': [extra['src_overlap'][i] for i in pairs], 'tgt_overlap': [extra['tgt_overlap'][i] for i in pairs]}
        return b

    before = {k: v.clone() for k, v in model.state_dict().items()}
    for p in model.parameters():
        p.grad = None
    b0 = batch_of([0, 1])
    pred = model(b0)
    want_losses = model.compute_loss(pred, b0)
    losses, met = model.validation_step(batch_of([0, 1]), 0)
    assert sorted(losses) == sorted(want_losses) and all(torch.equal(losses[k], want_losses[k]) for k in losses)
    assert sorted(met) == ['rot_err_deg', 'trans_err']
    L = pred['pose'].shape[0]
    assert met['rot_err_deg'].shape == (L, 2) and met['rot_err_deg'].dtype == torch.float32 and met['rot_err_deg'].is_cuda
    _close_metrics(met, ref.compute_metrics(pred['pose'].cpu().numpy(), extra['pose'].cpu().numpy()))
    assert all(p.grad is None for p in model.parameters())
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    # compute_metrics reads nothing but the poses
    again = model.compute_metrics({'pose': pred['pose']}, {'pose': extra['pose']})
    assert all(torch.equal(again[k], met[k]) for k in met)

    out1 = model.validation_step(batch_of([1]), 1)
    score, summary = model.validation_epoch_end([(losses, met), out1])
    assert type(score) is float
    for k in losses:
        assert torch.equal(summary['losses'][k], torch.stack([losses[k], out1[0][k]]).mean()), k
    steps = [{k: v.cpu().numpy() for k, v in m.items()} for m in (met, out1[1])]
    want = ref.aggregate(steps, 10, 0.1)
    assert sorted(summary['metrics']) == sorted(want)
    for k, v in want.items():
        got = summary['metrics'][k].cpu().numpy()
        if k.endswith('hist') or k.startswith('reg_success'):
            assert np.array_equal(got, v), k
        else:
            assert np.allclose(got, v, rtol=4 * U, atol=0), k
    assert score == float(want['reg_success_final']) and summary['metrics']['rot_err_final_hist'].shape == (3,)
    assert all(p.grad is None for p in model.parameters())


# ---------------------------------------------------------------------------------------------------- ModelNet end to end
def test_modelnet_test_step_end_to_end():
    from regtr_amd import RegTR, metrics
    from regtr_amd.augment import modelnet_train_batch
    from tests.test_gpu_modelnet_training import SEED, _cloud
    cfg = load_cfg('modelnet')
    model = RegTR(cfg)
    model.load_state_dict(seeded_sd(cfg), strict=True)
    model = model.cuda().eval()
    rng = np.random.default_rng(12)
    points = [_dev(_cloud(rng)) for _ in range(4)]
    batch = modelnet_train_batch(points, cfg, SEED, 0)
    assert 'tgt_raw' not in batch
    losses0, met0 = model.test_step(dict(batch), 0)
    assert 'modelnet' not in met0 and sorted(met0) == ['rot_err_deg', 'trans_err']
    with pytest.raises(KeyError, match='tgt_raw'):
        metrics.modelnet_metrics(torch.zeros((4, 3, 4), device='cuda'), batch)
    batch['tgt_raw'] = points
    losses, met = model.test_step(batch, 0)
    assert all(torch.equal(losses[k], losses0[k]) for k in losses) and torch.equal(met['rot_err_deg'], met0['rot_err_deg'])
    mm = met['modelnet']
    assert tuple(mm) == metrics.MODELNET_KEYS and all(v.shape == (4,) for v in mm.values())
    pred = model(batch)['pose'][-1].cpu().numpy()
    gt = batch['pose'].cpu().numpy()
    assert np.isfinite(pred).all()
    src, refc, raw = ([x.cpu().numpy() for x in batch[k]] for k in ('src_xyz', 'tgt_xyz', 'tgt_raw'))
    want = ref.modelnet_metrics(pred, gt, src, refc, raw)
    assert np.array_equal(mm['chamfer_dist'].cpu().numpy(), want['chamfer_dist'])      # the float32 restatement, bit for bit
    _check_vs_host(mm, pred, gt, src, refc, raw)                                      # the host function (measured: Chamfer 5.8e-8 relative)
