"""GPU: one RegTR.training_step and losses['total'].backward() against the composed float64 restatement tests/training_step_ref.py --
every loss, and the .grad of EVERY trainable parameter, in four configurations that between them walk every branch regtr.py adds to the
gradients (tests/training_step_ref.py: CONFIGS).  The kernels are held to float64 stage by stage elsewhere; this file is about the wiring.

The model: the shipped 3DMatch backbone at full size on the two-pair golden crop (tests/golden/losses_3dmatch_crop_b2.npz: 452 tokens),
cut down above the backbone to d_embed 64 / nhead 2 / d_feedforward 128 / 2 layers (training_step_ref.CUT says why).  Backbone weights:
oracle.seeded_weights, seed 0, the same in every configuration, so ONE tapped encoder run hands its LeakyReLU sides, pool winners and
row flags to every float64 run (tests/test_gpu_backbone_grads.py shows that the tapped run is the untapped one).  Above the backbone:
training_step_ref.draw_above at the seeds below -- the first at or after the nominal 51 (71 for the learned embedding's MLP) at which every
ReLU pre-activation and every weighted L1 residual of the float64 run keeps head_grads_ref.RELU_MARGIN from 0; asserted on every run.
A and D both train the backbone (a float64 encoder forward + backward on the device each: A 2.5 s with everything's first use, D 0.6 s, so
D did not have to fall back to a frozen backbone); B and C read the frozen backbone's output, for which the float64 encoder forward is
run once and shared (0.1 s each).  C's last regressor Linear is fitted (training_step_ref.fit_pose_head): a drawn one makes the pose
solve too ill-conditioned for the requirement below.

Bars.  Losses: 1e-5 relative (test_stack_against_the_real_reference_modules').  Gradients: max err <= 1e-4 max |ref| per tensor, the
project's flat bar; a tensor beyond it is held to 4x the error of the SAME composed restatement evaluated in float32 stock torch ops
against its float64 run (that test's relaxation and factor), never to anything taken from the code under test.  The set of checked names
is asserted equal to the set of trainable names.  C: the float64 solve's Procrustes conditioning (no zeroed pair, pair_bounds <= 1e-5
of the tensor maximum: tests/test_gpu_procrustes_grads.py's requirement).  B: two steps' backward passes without clearing .grad give
twice the single step's gradients to 2 ulp per element.

Worst figures measured on an MI355X: docs/PARITY.md, "The composed training step".
"""
import numpy as np
import pytest
import torch

from tests import backbone_grads_ref as BR
from tests import head_grads_ref as HR
from tests import training_step_ref as TS
from tests.util import gold, load_cfg, seeded_sd

pytestmark = pytest.mark.gpu

FLAT = 1e-4
LOSS_REL = 1e-5
CASE = '3dmatch_crop_b2'
BACKBONE_SEED = 0
# draw_above's seed per embedding (nominal 51): A, B and C share one set of weights (C with its last regressor Linear fitted).  At 51 the sine model has
# a pre-activation at 4.2e-7; 52 keeps 5.2e-6, the learned model at 51 keeps 1.0e-5 (RELU_MARGIN is 1.9e-6).
SEED = {'sine': 52, 'learned': 51}
MLP_SEED = 71                               # posemb_mlp_ref.STACK_SEED: the learned embedding's MLP
_shared = {}


def _flat(got, ref):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def _batch():
    from tests.test_gpu_losses import _golden_batch
    srcs, tgts, extra = _golden_batch(gold(f'losses_{CASE}'), CASE)
    b = {'src_xyz': [torch.from_numpy(s).cuda() for s in srcs], 'tgt_xyz': [torch.from_numpy(t).cuda() for t in tgts]}
    b.update(extra)
    return b


def _model(name):
    """-> (cfg, model, the parameters above the backbone as drawn)."""
    from regtr_amd import RegTR
    cfg = TS.config(load_cfg('3dmatch'), name)
    learned = cfg.pos_emb_type == 'learned'
    sd = {k: v for k, v in seeded_sd(cfg, BACKBONE_SEED).items() if k.startswith('kpf_encoder.')}
    K = sd['kpf_encoder.encoder_blocks.10.unary2.mlp.weight'].shape[0]
    above = TS.draw_above(cfg, K, SEED['learned' if learned else 'sine'], MLP_SEED)
    sd.update(above)
    model = RegTR(cfg)
    model.load_state_dict(sd, strict=True)
    return cfg, model.cuda().eval(), above


def _step(model, run):
    b = _batch()
    if run.get('backbone_grad'):
        pred = model.forward_grad(b, backbone_grad=True)
        losses = model.compute_loss_grad(pred, b)
    elif run.get('train_backbone'):
        pred, losses = model.training_step(b, train_backbone=True)
    else:
        pred, losses = model.training_step(b)
    losses['total'].backward()
    return b, pred, losses


def _encoder(model, cfg, kpconv_meta):
    """The backbone's share of the reference, once for all configurations: the block dicts, the host meta, the tapped device run's sides."""
    from regtr_amd import context
    from tests.test_gpu_backbone_grads import _sides
    enc_sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.startswith('kpf_encoder.')}
    if 'sides' in _shared:
        assert all(torch.equal(v, _shared['enc_sd'][k]) for k, v in enc_sd.items()), 'the shared sides are those of other backbone weights'
        return _shared
    enc = model.kpf_encoder
    ones = torch.ones((kpconv_meta['points'][0].shape[0], 1), device='cuda')
    taps = []
    dev = ones.device
    with context.forward(dev, f16_pair=False, force_x3=True, status=None):
        enc.forward_grad(ones, kpconv_meta, taps)
    assert len(taps) == len(enc.encoder_blocks) == 11
    sides, cur = [], ones
    for m, tap in zip(enc.encoder_blocks, taps):
        sides.append(_sides(m, tap, cur, kpconv_meta))
        cur = tap['norms'][-1]
    _shared.update(enc_sd=enc_sd, sides=sides, meta=BR.meta_of(kpconv_meta), ones=ones.cpu().numpy(),
                   blocks=BR.encoder_blocks(cfg, {k: v.numpy() for k, v in enc_sd.items()}))
    return _shared


def _pyramid(model):
    from regtr_amd import context
    b = _batch()
    dev = b['src_xyz'][0].device
    with torch.no_grad(), context.forward(dev, f16_pair=False, force_x3=True, status=None):
        return model.preprocessor(b['src_xyz'] + b['tgt_xyz'])


def _feats_un(s, dtype=torch.float64):
    """The restatement's encoder output under the shared sides, once per dtype."""
    key = 'feats_un' if dtype is torch.float64 else 'feats_un32'
    if key not in s:
        s[key] = BR.run(s['blocks'], s['ones'], s['meta'], None, sides=s['sides'], backward=False, device='cuda', dtype=dtype)['out']
    return s[key]


def _reference(cfg, above, s, b, train_backbone, dtype=torch.float64):
    n_lvl = len(s['meta']['points'])
    gt = b['overlap_pyr'][f'pyr_{n_lvl - 1}'].cpu().numpy()
    pose = b['pose'].cpu().numpy()
    kw = dict(sides=s['sides'], device='cuda', dtype=dtype)
    if train_backbone:
        ref = TS.run(cfg, s['blocks'], above, s['meta'], s['ones'], gt, pose, train_backbone=True, **kw)
        if dtype is torch.float64:
            s.setdefault('feats_un', ref['feats_un'])
        return ref
    return TS.run(cfg, s['blocks'], above, s['meta'], s['ones'], gt, pose, train_backbone=False, feats_un=_feats_un(s, dtype), **kw)


@pytest.mark.parametrize('name', list(TS.CONFIGS))
def test_training_step_against_the_composed_float64_reference(name):
    run = TS.CONFIGS[name]
    tb = bool(run.get('train_backbone'))
    cfg, model, above = _model(name)
    params = model.trainable_parameters(backbone=tb)
    named = {k: p for k, p in model.named_parameters() if p.requires_grad and (tb or not k.startswith('kpf_encoder.'))}
    assert {id(p) for p in named.values()} == {id(p) for p in params} and len(params) == len(named)
    s = _encoder(model, cfg, _pyramid(model))
    if name == 'C':
        # (a drawn regressor's pose solve is ill-conditioned: training_step_ref.fit_pose_head fits its last Linear on the float64 run)
        above = TS.fit_pose_head(cfg, above, s['meta'], _batch()['pose'].cpu().numpy(), _feats_un(s))
        fitted = {k: above[k] for k in ('correspondence_decoder.coor_mlp.4.weight', 'correspondence_decoder.coor_mlp.4.bias')}
        assert not model.load_state_dict(fitted, strict=False).unexpected_keys
    b, pred, losses = _step(model, run)
    assert list(losses) == model.loss_keys() == TS.loss_keys(cfg) and model.head_layers() == TS.head_layers(cfg)
    assert all(np.array_equal(p, q) for p, q in zip(BR.meta_of(b['kpconv_meta'])['points'], s['meta']['points'])), 'the step built another pyramid'
    ref = _reference(cfg, above, s, b, tb)

    # the case: every ReLU and every L1 residual of the float64 run away from its kink; C: a well-conditioned solve
    print(f'{name}: relu margin {ref["relu_margin"]:.3e}, L1 margin {ref["l1_margin"]:.3e} (required {HR.RELU_MARGIN:.3e})')
    assert min(ref['relu_margin'], ref['l1_margin']) >= HR.RELU_MARGIN, 'the seeded case sits on a kink: take the next seed'
    if name == 'C':
        assert TS.pose_on(cfg) and 1 not in set(cfg.overlap_loss_on) | set(cfg.corr_loss_on) and model.head_layers() == [0, 1]
        print(f'{name}: Procrustes kappa {[round(float(i["kappa"]), 3) for i in ref["pose_infos"]]}, bound / maximum {ref["pose_bound"]:.2e}')
        assert not any(i['zeroed'] for i in ref['pose_infos']) and ref['pose_bound'] <= 1e-5
        assert np.abs(pred['pose'][0].detach().double().cpu().numpy() - ref['pose']).max() <= FLAT
    else:
        assert not TS.pose_on(cfg)

    # losses
    for k in TS.loss_keys(cfg):
        got, want = float(losses[k]), ref['losses'][k]
        print(f'{name} loss {k}: {got:.7f} vs {want:.7f} ({abs(got - want) / abs(want):.2e})')
    for k in TS.loss_keys(cfg):
        assert abs(float(losses[k]) - ref['losses'][k]) <= LOSS_REL * abs(ref['losses'][k]), k

    # gradients: every trainable tensor, none other
    assert set(named) == set(ref['grads']), 'the checked names are the trainable names'
    items = [(k, named[k].grad, ref['grads'][k]) for k in sorted(named)]
    if run.get('backbone_grad'):
        fu = pred['_feats_un']
        assert fu.is_leaf and fu.grad is not None
        items.append(('d_feats_un', fu.grad, ref['d_feats_un']))
    if not tb:
        assert all(p.grad is None for p in model.kpf_encoder.parameters())
    assert all(p.grad is None for k, p in model.named_parameters() if k.endswith('kernel_points'))
    f32, beyond, worst = None, [], ('', 0.0)
    for k, got, want in items:
        assert got is not None and torch.isfinite(got).all() and np.abs(want).max() > 0, k
        e, bar = _flat(got, want), FLAT
        if e > FLAT:
            if f32 is None:
                f32 = _reference(cfg, above, s, b, tb, dtype=torch.float32)
            bar = 4 * _flat(f32['d_feats_un'] if k == 'd_feats_un' else f32['grads'][k], want)
        print(f'{name} {k}: {e:.2e} (bar {bar:.2e})')
        worst = max(worst, (k, e), key=lambda x: x[1])
        if e > bar:
            beyond.append((k, e, bar))
    print(f'{name}: worst gradient {worst[0]} {worst[1]:.2e} of {len(items)} tensors')
    assert not beyond, beyond

    if name == 'B':
        # two steps, two backward passes, .grad never cleared: twice the single step's gradients
        once = {k: p.grad.clone() for k, p in named.items()}
        for p in model.parameters():
            p.grad = None
        _step(model, run)
        _step(model, run)
        for k, p in named.items():
            want = 2.0 * once[k].double().cpu().numpy()
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert (np.abs(p.grad.double().cpu().numpy() - want) <= 2 * ulp).all(), k
