"""GPU: RegTR.training_step(train_backbone=True) under the ModelNet configuration (two-level backbone, first_feats_dim 512, rows up to
1024 wide, one strided block) on batches built by regtr_amd.augment.modelnet_train_batch: the prediction against the inference forward,
a gradient for every trainable parameter, bitwise repeatability, the encoder's weight gradients against the float64 restatement
(tests/backbone_grads_ref.py, given the forward's own sides, at the FLAT = 1e-4 bar of tests/test_gpu_backbone_grads.py), and five AdamW
steps.  The shipped configuration has wt_feature_un = 0.0, which makes feature_criterion_un.W's gradient vanish by construction: the
training step runs under the shipped configuration with that one parameter exempt from the non-zero check, and again with
wt_feature_un = 0.05 (as tests/test_gpu_head_grads.py sets it) with no parameter exempt.

Inputs: seeded weights, B = 2 raw clouds of 2048 seeded points on a box and a sphere inside the unit ball (ModelNet40's normalisation;
regtr_amd/synthetic.py and workload.py sample room-like 3DMatch pairs only)."""
import numpy as np
import pytest
import torch

from tests.util import load_cfg, seeded_sd

pytestmark = pytest.mark.gpu

SEED = 20240611
_shared = {}


def _cloud(rng, n=2048):
    a = n // 2
    dims = np.array([1.0, 0.6, 0.3])
    box = rng.uniform(-0.5, 0.5, (a, 3)) * dims
    face = rng.integers(0, 3, a)
    box[np.arange(a), face] = np.sign(box[np.arange(a), face]) * 0.5 * dims[face]
    v = rng.standard_normal((n - a, 3))
    ball = 0.35 * v / np.linalg.norm(v, axis=1, keepdims=True) + np.array([0.2, 0.1, 0.25])
    return np.concatenate([box, ball]).astype(np.float32)[rng.permutation(n)]


def _setup(wt_feature_un=None):
    """Seeded model and two raw clouds; wt_feature_un None: the shipped configuration."""
    if wt_feature_un not in _shared:
        from regtr_amd import RegTR
        cfg = load_cfg('modelnet')
        if wt_feature_un is not None:
            cfg.wt_feature_un = wt_feature_un
        model = RegTR(cfg)
        model.load_state_dict(seeded_sd(cfg), strict=True)
        model = model.cuda().eval()
        rng = np.random.default_rng(11)
        points = [torch.from_numpy(_cloud(rng)).cuda() for _ in range(2)]
        _shared[wt_feature_un] = dict(cfg=cfg, model=model, points=points, sd={k: v.clone() for k, v in model.state_dict().items()})
    s = _shared[wt_feature_un]
    s['model'].load_state_dict(s['sd'], strict=True)
    return s['cfg'], s['model'], s['points']


def _step(model, batch, params):
    for p in model.parameters():
        p.grad = None
    pred, losses = model.training_step(batch, train_backbone=True)
    losses['total'].backward()
    return pred, losses, [None if p.grad is None else p.grad.clone() for p in params]


@pytest.mark.parametrize('wt_feature_un', [None, 0.05])
def test_training_step_on_a_modelnet_batch(wt_feature_un):
    from regtr_amd import context
    from regtr_amd.augment import modelnet_train_batch
    cfg, model, points = _setup(wt_feature_un)
    assert cfg.wt_feature_un == (0.0 if wt_feature_un is None else wt_feature_un)
    params = model.trainable_parameters(backbone=True)
    assert any(n.startswith('kpf_encoder.') for n, p in model.named_parameters() if id(p) in set(map(id, params)))
    pred, losses, grads = _step(model, modelnet_train_batch(points, cfg, SEED, 0), params)
    assert all(bool(torch.isfinite(v)) for v in losses.values()), {k: float(v) for k, v in losses.items()}
    name_of = {id(p): n for n, p in model.named_parameters()}
    for p, g in zip(params, grads):
        if wt_feature_un is None and name_of[id(p)] == 'feature_criterion_un.W':      # weight 0.0: no gradient by construction
            assert g is None or (torch.isfinite(g).all() and not g.any())
            continue
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, name_of[id(p)]
    # the inference forward on the same batch: the forward's existing 1e-4 bars
    b2 = modelnet_train_batch(points, cfg, SEED, 0)
    dev = points[0].device
    with torch.no_grad(), context.forward(dev, f16_pair=False, force_x3=True, status=None):
        want = model._forward(b2, dev)
    layer = model.head_layers()[-1]
    ep = (pred['pose'][-1].detach() - want['pose'][-1]).abs().max().item()
    ec = max((pred['src_kp_warped'][b][layer].detach() - want['src_kp_warped'][b][layer]).abs().max().item() for b in range(2))
    print(f'training_step vs inference forward: pose {ep:.2e}, correspondences {ec:.2e}')
    assert ep < 1e-4 and ec < 1e-4
    # the same batch again: the same bits
    _, losses2, grads2 = _step(model, modelnet_train_batch(points, cfg, SEED, 0), params)
    assert torch.equal(losses['total'].detach(), losses2['total'].detach())
    assert all(torch.equal(x, y) for x, y in zip(grads, grads2))


def test_encoder_weight_gradients_against_float64():
    """KPFEncoder.forward_grad on the built batch's pyramid (two levels, 512 -> 1024 channels, one strided block) and the backward of
    sum(out * d_out) against tests/backbone_grads_ref.run in float64, which is handed the forward's own LeakyReLU sides, pool winners
    and row flags (tests/test_gpu_backbone_grads.py: _sides).  Every encoder weight gradient and the output at FLAT = 1e-4 of the
    tensor's maximum."""
    from regtr_amd import context
    from regtr_amd.augment import modelnet_train_batch
    from tests import backbone_grads_ref as BR
    from tests.test_gpu_backbone_grads import FLAT, _dev, _flat, _sides
    cfg, model, points = _setup()
    batch = modelnet_train_batch(points, cfg, SEED, 0)
    dev = points[0].device
    enc = model.kpf_encoder
    model.zero_grad()
    taps = []
    with context.forward(dev, f16_pair=False, force_x3=True, status=None):
        with torch.no_grad():
            meta = model.preprocessor(batch['src_xyz'] + batch['tgt_xyz'])
        assert len(meta['points']) == 2 and [sum(l) for l in meta['_lens_host']] == [int(p.shape[0]) for p in meta['points']]
        ones = torch.ones((meta['points'][0].shape[0], 1), device='cuda')
        out = enc.forward_grad(ones, meta, taps)
        d_out = np.random.default_rng(17).normal(0, 1, tuple(out.shape)).astype(np.float32)
        (out * _dev(d_out)).sum().backward()
    assert len(enc.encoder_blocks) == 6 == len(taps) and out.shape[1] == 1024
    grads = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    sides, cur = [], ones
    for m, tap in zip(enc.encoder_blocks, taps):
        sides.append(_sides(m, tap, cur, meta))
        cur = tap['norms'][-1]
    blocks = BR.encoder_blocks(cfg, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
    ref = BR.run(blocks, ones.cpu().numpy(), BR.meta_of(meta), d_out, sides=sides, device='cuda')
    weights = {k for k, p in enc.named_parameters() if p.requires_grad}
    assert set(grads) == weights == {f'encoder_blocks.{i}.{k}' for (i, k) in ref['grads']}, 'every encoder weight is checked'
    assert max(g.shape[-1] for g in grads.values()) == 1024 and any(512 in g.shape for g in grads.values())
    worst = ('', 0.0)
    for (i, k), want in ref['grads'].items():
        e = _flat(grads[f'encoder_blocks.{i}.{k}'], want)
        print(f'modelnet encoder block {i} {k} {tuple(want.shape)}: {e:.2e}')
        worst = max(worst, (f'{i}.{k}', e), key=lambda t: t[1])
    e_out = _flat(out, ref['out'])
    print(f'modelnet encoder: worst gradient {worst[0]} {worst[1]:.2e}; output {e_out:.2e} of the float64 restatement')
    assert worst[1] <= FLAT and e_out <= FLAT


def test_five_adamw_steps_lower_the_total():
    from regtr_amd.augment import modelnet_train_batch
    cfg, model, points = _setup()
    params = model.trainable_parameters(backbone=True)
    opt = torch.optim.AdamW(params, lr=1e-4)
    totals = []
    for step in range(5):
        batch = modelnet_train_batch(points, cfg, SEED, step)
        opt.zero_grad(set_to_none=True)
        pred, losses = model.training_step(batch, train_backbone=True)
        losses['total'].backward()
        opt.step()
        totals.append(float(losses['total'].detach()))
        assert [int(x.shape[0]) for x in batch['src_xyz'] + batch['tgt_xyz']] == [717] * 4
    print('totals over five AdamW steps:', [f'{t:.4f}' for t in totals])
    assert all(np.isfinite(totals)) and totals[-1] < totals[0]
    assert all(torch.isfinite(p).all() for p in params)
