"""GPU: regtr_weighted_procrustes_bwd (csrc/procrustes.hip: k_procrustes_bwd) and everything built on it -- ops.weighted_procrustes_bwd,
head_grad.procrustes_forward_grad, se3.compute_rigid_transform's gradients, RegTR.forward_grad's differentiable pose and the opt-in
pose term -- against the float64 restatement with its derived float32 bound (tests/procrustes_grads_ref.py) and the reference's own
float64 autograd (tests/golden/procrustes_grads.npz).

Measured on an MI355X (the golden launch, L = 2, pairs (5, 9), (300, 257), (64, 0), (130, 1)): worst err / bound 0.025 (d_corr), 0.054
(d_logit), 0.027 (d_kp), 0.054 (d_weight), the bound 4.0e-6 .. 6.6e-6 of each tensor's maximum; 1.3e-7 of the maximum from the
reference's float64 autograd; rotation- / translation-only d_pose 0.094 / 0.044; docs/KERNELS.md keeps the table."""
import numpy as np
import pytest
import torch

from tests import procrustes_grads_ref as R
from tests.util import gold, load_cfg, to_dev

pytestmark = pytest.mark.gpu

OUTS = ('d_corr', 'd_logit', 'd_kp', 'd_weight')
_shared = {}


def _golden():
    if 'g' not in _shared:
        g = gold('procrustes_grads')
        ref, infos = R.model_backward(g['kp'], g['corr'], g['logit'], g['seg_off'], g['d_pose'])
        _shared.update(g=g, ref=ref, infos=infos, bound=R.pair_bounds(ref, infos),
                       dev={k: to_dev(g[k]) for k in ('kp', 'corr', 'logit', 'seg_off', 'd_pose')})
    return _shared['g'], _shared['ref'], _shared['infos'], _shared['bound'], _shared['dev']


def _run(d, d_pose=None, **want):
    from regtr_amd import ops
    B = (d['seg_off'].numel() - 1) // 2
    out = ops.weighted_procrustes_bwd(d['kp'], d['corr'], d['logit'], d['seg_off'], B, d['d_pose'] if d_pose is None else d_pose, **want)
    return dict(zip(OUTS, out))


def _np(out):
    return {k: v.double().cpu().numpy() for k, v in out.items() if v is not None}


def _worst(got, ref, bound):
    worst = {}
    for k in OUTS:
        m = bound[k] > 0
        assert np.array_equal(got[k][~m], ref[k][~m]), k              # (entries with a zero bound: rows of zeroed pairs)
        worst[k] = float((np.abs(got[k] - ref[k])[m] / bound[k][m]).max())
    return worst


def test_operator_vs_restatement_and_golden():
    g, ref, infos, bound, d = _golden()
    out = _run(d, want_logit=True, want_kp=True, want_weight=True)
    got = _np(out)
    assert all(np.isfinite(got[k]).all() for k in OUTS)
    worst = _worst(got, ref, bound)
    rel = {k: float(bound[k].max() / np.abs(ref[k]).max()) for k in OUTS}
    vs_gold = {k: float(np.abs(got[k] - g[k]).max() / np.abs(g[k]).max()) for k in OUTS}
    print('procrustes_bwd vs restatement, worst err / bound:', {k: f'{v:.3f}' for k, v in worst.items()})
    print('procrustes_bwd bound / tensor maximum:', {k: f'{v:.2e}' for k, v in rel.items()})
    print('procrustes_bwd vs reference autograd, err / tensor maximum:', {k: f'{v:.2e}' for k, v in vs_gold.items()})
    assert max(rel.values()) <= 1e-5, rel
    assert max(worst.values()) <= 1.0, worst
    assert max(vs_gold.values()) <= 1e-4, vs_gold
    # two runs are bit-equal; the optional outputs change nothing
    again = _run(d, want_logit=True, want_kp=True, want_weight=True)
    assert all(torch.equal(out[k], again[k]) for k in OUTS)
    for want in (dict(want_logit=False), dict(want_logit=True), dict(want_logit=False, want_kp=True), dict(want_logit=False, want_weight=True)):
        o = _run(d, **want)
        assert torch.equal(o['d_corr'], out['d_corr']), want
        for k, flag in (('d_logit', 'want_logit'), ('d_kp', 'want_kp'), ('d_weight', 'want_weight')):
            assert (o[k] is None) == (not want.get(flag, False)) and (o[k] is None or torch.equal(o[k], out[k])), (want, k)


@pytest.mark.parametrize('part', ['rotation', 'translation'])
def test_rotation_only_and_translation_only_gradients(part):
    g, _, _, _, d = _golden()
    dp = g['d_pose'].copy()
    if part == 'rotation':
        dp[..., 3] = 0
    else:
        dp[..., :3] = 0
    ref, infos = R.model_backward(g['kp'], g['corr'], g['logit'], g['seg_off'], dp)
    got = _np(_run(d, d_pose=to_dev(dp), want_logit=True, want_kp=True, want_weight=True))
    worst = _worst(got, ref, R.pair_bounds(ref, infos))
    print(f'procrustes_bwd, {part} gradient only, worst err / bound:', {k: f'{v:.3f}' for k, v in worst.items()})
    assert max(worst.values()) <= 1.0 and all(np.abs(got[k]).max() > 0 for k in OUTS)


def test_function_forward_is_the_operator_and_carries_a_gradient():
    from regtr_amd import head_grad, ops
    g, ref, _, bound, d = _golden()
    B = (d['seg_off'].numel() - 1) // 2
    corr, logit = d['corr'].clone().requires_grad_(), d['logit'].clone().requires_grad_()
    pose = head_grad.procrustes_forward_grad(d['kp'], corr, logit, d['seg_off'], B)
    want = ops.weighted_procrustes(d['kp'], d['corr'], d['logit'], d['seg_off'], B)
    assert torch.equal(pose.detach(), want) and pose.grad_fn is not None
    assert float(np.abs(pose.detach().cpu().numpy() - g['pose']).max()) <= 1e-5
    (pose * d['d_pose']).sum().backward()
    out = _run(d)
    assert torch.equal(corr.grad, out['d_corr']) and torch.equal(logit.grad, out['d_logit'])
    with pytest.raises(NotImplementedError):
        head_grad.procrustes_forward_grad(d['kp'].clone().requires_grad_(), corr, logit, d['seg_off'], B)
    pose2 = head_grad.procrustes_forward_grad(d['kp'], corr, logit, d['seg_off'], B)
    gr, = torch.autograd.grad((pose2 * d['d_pose']).sum(), corr, create_graph=True)
    with pytest.raises(RuntimeError):                                                              # double backward is refused
        gr.sum().backward()


def test_degenerate_pairs_get_zero_rows_beside_a_healthy_pair():
    """Pairs: 0 healthy (40, 30); 1 one point; 2 collinear source key points (on the x axis: a' has exactly zero y and z); 3 an exactly
    zero covariance (every a_i the origin); 4 logits of -40 throughout (the weight sum clamps); 5 healthy again.  L = 2."""
    rng = np.random.default_rng(17)
    lens = [40, 1, 12, 9, 10, 33] + [30, 0, 0, 0, 6, 20]
    B = 6
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N, L = int(seg[-1]), 2
    kp = rng.standard_normal((N, 3)).astype(np.float32)
    corr = (kp @ np.diag([1.0, 0.8, 0.6]) + 0.1 * rng.standard_normal((L, N, 3))).astype(np.float32)
    logit = rng.uniform(-2, 2, (L, N)).astype(np.float32)
    s = lambda p: slice(seg[p], seg[p + 1])
    kp[s(2), 1:] = 0
    kp[s(3)] = 0
    logit[:, s(4)] = -40
    logit[:, s(B + 4)] = -40
    d_pose = rng.standard_normal((L, B, 3, 4)).astype(np.float32)
    d = dict(kp=to_dev(kp), corr=to_dev(corr), logit=to_dev(logit), seg_off=to_dev(seg), d_pose=to_dev(d_pose))
    out = _run(d, want_logit=True, want_kp=True, want_weight=True)
    ref, infos = R.model_backward(kp, corr, logit, seg, d_pose)
    assert [i['zeroed'] for i in infos[0]] == [i['zeroed'] for i in infos[1]] == [False, True, True, True, True, False]
    for k in OUTS:
        assert torch.isfinite(out[k]).all(), k
        for p in (1, 2, 3, 4):
            assert not out[k][:, s(p)].any() and not out[k][:, s(B + p)].any(), (k, p)
        for p in (0, 5):
            assert out[k][:, s(p)].abs().max() > 0
    worst = _worst(_np(out), ref, R.pair_bounds(ref, infos))
    print('procrustes_bwd, healthy pairs beside degenerate ones, worst err / bound:', {k: f'{v:.3f}' for k, v in worst.items()})
    assert max(worst.values()) <= 1.0
    # the healthy pairs alone, in a launch of their own: the same bits
    for p in (0, 5):
        rows = np.r_[seg[p]:seg[p + 1], seg[B + p]:seg[B + p + 1]]
        seg1 = np.array([0, lens[p], lens[p] + lens[B + p]], np.int32)
        d1 = dict(kp=to_dev(kp[rows]), corr=to_dev(corr[:, rows]), logit=to_dev(logit[:, rows]), seg_off=to_dev(seg1),
                  d_pose=to_dev(d_pose[:, p:p + 1]))
        alone = _run(d1, want_logit=True, want_kp=True, want_weight=True)
        idx = torch.from_numpy(rows).cuda()
        for k in OUTS:
            assert torch.equal(alone[k], out[k][:, idx]), (k, p)


def test_equal_singular_values():
    """A cube's corners under a rigid motion (tests/test_procrustes_grads_host.py checks the restatement there against finite
    differences): S0 = S1 = S2 up to float32 rounding, kappa = 1 / 2 -- finite, and within the bound of the restatement."""
    from tests.test_procrustes_grads_host import _cube
    a, b, lg, dp = _cube()
    kp, corr, logit = a.astype(np.float32), b.astype(np.float32)[None], lg.astype(np.float32)[None]
    seg, d_pose = np.array([0, 8, 8], np.int32), dp.astype(np.float32)[None, None]
    ref, infos = R.model_backward(kp, corr, logit, seg, d_pose)
    assert not infos[0][0]['zeroed'] and abs(infos[0][0]['kappa'] - 0.5) <= 1e-6
    d = dict(kp=to_dev(kp), corr=to_dev(corr), logit=to_dev(logit), seg_off=to_dev(seg), d_pose=to_dev(d_pose))
    got = _np(_run(d, want_logit=True, want_kp=True, want_weight=True))
    worst = _worst(got, ref, R.pair_bounds(ref, infos))
    print('procrustes_bwd, equal singular values, worst err / bound:', {k: f'{v:.3f}' for k, v in worst.items()})
    assert all(np.isfinite(got[k]).all() for k in OUTS) and max(worst.values()) <= 1.0


@pytest.mark.parametrize('with_weights', [True, False])
def test_compute_rigid_transform_gradients(with_weights):
    from regtr_amd import se3
    g = gold('procrustes_grads')
    tag = '' if with_weights else '_none'
    a, b = to_dev(g['se3_a']).requires_grad_(), to_dev(g['se3_b']).requires_grad_()
    w = to_dev(g['se3_w']).requires_grad_() if with_weights else None
    assert tuple(a.shape) == (2, 3, 40, 3) and (g['se3_w'] == 0).any() and (g['se3_w'] == 1).any()
    T = se3.compute_rigid_transform(a, b, w)
    with torch.no_grad():
        T0 = se3.compute_rigid_transform(a.detach(), b.detach(), None if w is None else w.detach())
    assert tuple(T.shape) == (2, 3, 3, 4) and torch.equal(T.detach(), T0) and T.grad_fn is not None
    assert float(np.abs(T.detach().cpu().numpy() - g[f'se3{tag}_T']).max()) <= 1e-5
    (T * to_dev(g['se3_dT'])).sum().backward()
    pairs = [('da', a), ('db', b)] + ([('dw', w)] if with_weights else [])
    for name, t in pairs:
        want = g[f'se3{tag}_{name}']
        got = t.grad.double().cpu().numpy()
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print(f'compute_rigid_transform (weights {with_weights}) {name}: err / tensor maximum {err:.2e}')
        assert np.isfinite(got).all() and err <= 1e-4, name


# ------------------------------------------------------------------------------------------------ the model
CASE = '3dmatch_crop_b2'


def _model_setup(wt_pose=None):
    key = ('model', wt_pose)
    if key not in _shared:
        from tests.test_gpu_losses import _golden_batch, _model
        g = gold(f'losses_{CASE}')
        cfg = load_cfg('3dmatch')
        if wt_pose is not None:
            cfg.wt_pose = wt_pose
        model = _model(cfg, g)
        srcs, tgts, extra = _golden_batch(g, CASE)

        def batch():
            b = {'src_xyz': [torch.from_numpy(s).cuda() for s in srcs], 'tgt_xyz': [torch.from_numpy(t).cuda() for t in tgts]}
            b.update(extra)
            return b
        _shared[key] = (model, batch)
    return _shared[key]


def _packed(pred, key, layer=None):
    views = list(pred['src_' + key]) + list(pred['tgt_' + key])
    return torch.cat([v if layer is None else v[layer] for v in views], dim=0)


def test_forward_grad_pose_is_the_detached_pose_with_a_grad_fn_and_its_gradient_reaches_the_head():
    from regtr_amd import context, ops
    model, batch = _model_setup()
    for p in model.parameters():
        p.grad = None
    b = batch()
    pred = model.forward_grad(b)
    B = len(pred['src_kp'])
    last = model.cfg.num_encoder_layers - 1
    xyz = _packed(pred, 'kp').contiguous()
    corr = _packed(pred, 'kp_warped', last).detach().contiguous()[None]
    logit = _packed(pred, 'overlap', last).detach().reshape(1, -1).contiguous()
    seg = b['kpconv_meta']['_seg_off'][-1]
    with context.forward(xyz.device, f16_pair=False, status=None):
        want = ops.weighted_procrustes(xyz, corr, logit, seg, B)
    assert tuple(pred['pose'].shape) == (1, B, 3, 4) and torch.equal(pred['pose'].detach(), want)
    assert pred['pose'].grad_fn is not None and pred['pose'].requires_grad
    assert np.array_equal(pred['pose'][0].cpu().numpy(), want[0].cpu().numpy())          # (head_grad.PoseTensor: numpy() detaches)
    # a pose-only loss: the two output biases of the head receive the row sums of the operator's d_corr and d_logit
    gen = torch.Generator().manual_seed(3)
    d_pose = torch.randn((1, B, 3, 4), generator=gen).cuda()
    (pred['pose'] * d_pose).sum().backward()
    d_corr, d_logit, _, _ = ops.weighted_procrustes_bwd(xyz, corr, logit, seg, B, d_pose)
    head = model.correspondence_decoder
    n = xyz.shape[0]
    for name, got, terms in (('coor_mlp[4].bias', head.coor_mlp[4].bias.grad, d_corr[0].double()),
                             ('conf_logits_decoder.bias', head.conf_logits_decoder.bias.grad, d_logit[0].double().unsqueeze(1))):
        want_sum, bar = terms.sum(0), n * 2.0 ** -23 * terms.abs().sum(0)
        err = (got.double() - want_sum).abs()
        print(f'pose-only loss, {name}.grad vs the row sums: err {err.max().item():.2e} (bar {bar.min().item():.2e})')
        assert torch.isfinite(got).all() and (err <= bar).all() and got.abs().max() > 0, name
    assert model.feat_proj.weight.grad is not None and model.feat_proj.weight.grad.abs().max() > 0


def test_without_wt_pose_training_step_is_the_parent_code_path():
    """wt_pose absent: the parent's keys, and losses and every parameter gradient bit-equal to the parent's code path -- the pose
    computed from detached inputs without gradient -- and to a repeat."""
    from regtr_amd import head_grad, ops
    model, batch = _model_setup()
    params = model.trainable_parameters()

    def step():
        for p in model.parameters():
            p.grad = None
        pred, losses = model.training_step(batch())
        losses['total'].backward()
        return pred, {k: v.detach().clone() for k, v in losses.items()}, [p.grad.clone() for p in params]

    pred, losses, grads = step()
    assert list(losses) == model.loss_keys() == ['overlap_5', 'feature_5', 'feature_un', 'corr_5', 'total']
    _, losses2, grads2 = step()
    saved = head_grad.procrustes_forward_grad

    def parent_path(kp, corr, logit, seg_off, n_pairs):
        with torch.no_grad():
            return ops.weighted_procrustes(kp, corr.detach(), logit.detach(), seg_off, n_pairs)
    head_grad.procrustes_forward_grad = parent_path
    try:
        pred3, losses3, grads3 = step()
    finally:
        head_grad.procrustes_forward_grad = saved
    assert pred3['pose'].grad_fn is None and torch.equal(pred3['pose'], pred['pose'].detach())
    for other_l, other_g in ((losses2, grads2), (losses3, grads3)):
        assert all(torch.equal(losses[k], other_l[k]) for k in losses)
        assert all(torch.equal(x, y) for x, y in zip(grads, other_g))


def test_five_fused_steps_with_the_pose_term():
    model, batch = _model_setup(wt_pose=1.0)
    last = model.cfg.num_encoder_layers - 1
    model.configure_optimizers()
    assert model.head_layers() == [last] and f'pose_{last}' in model.loss_keys()
    hist = []
    for step in range(5):
        model.optimizer.zero_grad()
        b = batch()
        pred, losses = model.training_step(b, train_backbone=True)
        if step == 0:
            ref = model.compute_loss(pred, b)
            assert list(ref) == list(losses) == model.loss_keys()
            assert torch.equal(ref[f'pose_{last}'], losses[f'pose_{last}'].detach())
        losses['total'].backward()
        model.optimizer.step()
        model.scheduler.step()
        hist.append({k: float(v.detach()) for k, v in losses.items()})
    print('pose term, five fused steps: first', {k: f'{v:.4f}' for k, v in hist[0].items()})
    print('pose term, five fused steps: last ', {k: f'{v:.4f}' for k, v in hist[-1].items()})
    assert all(np.isfinite(v) for h in hist for v in h.values())
    assert hist[-1]['total'] < hist[0]['total']
    assert all(torch.isfinite(p).all() for p in model.parameters())
