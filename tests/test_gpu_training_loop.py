"""GPU: the optimiser wired into the model -- RegTR.configure_optimizers, the weight caches after a fused step, five fused steps on
device-built ModelNet batches, and train.py's checkpoint / resume.

Inputs as tests/test_gpu_modelnet_training.py builds them: seeded weights, B = 2 raw clouds of 2048 seeded points on a box and a sphere
inside the unit ball."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import ROOT, load_cfg, seeded_sd

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


def _points():
    if 'points' not in _shared:
        rng = np.random.default_rng(11)
        _shared['points'] = [torch.from_numpy(_cloud(rng)).cuda() for _ in range(2)]
    return _shared['points']


def _fresh_model(cfg, sd=None):
    from regtr_amd import RegTR
    model = RegTR(cfg)
    model.load_state_dict(seeded_sd(cfg) if sd is None else sd, strict=True)
    return model.cuda().eval()


def _inference(model, batch):
    with torch.no_grad():
        out = model({'src_xyz': list(batch['src_xyz']), 'tgt_xyz': list(batch['tgt_xyz'])})
    return out['pose'].clone(), [w.clone() for w in out['src_kp_warped'][0]]


def _stale_cache_case(cfg, batch):
    """An inference forward (fills the weight caches), one training_step + backward + optimizer.step(), the forward again: bit for bit
    the forward of a fresh model loaded from the stepped state_dict, and different from the first forward."""
    model = _fresh_model(cfg)
    model.configure_optimizers()
    pose0, warped0 = _inference(model, batch)
    model.optimizer.zero_grad()
    _, losses = model.training_step(batch, train_backbone=True)
    losses['total'].backward()
    model.optimizer.step()
    pose1, warped1 = _inference(model, batch)
    fresh = _fresh_model(cfg, {k: v.clone() for k, v in model.state_dict().items()})
    pose2, warped2 = _inference(fresh, batch)
    assert torch.equal(pose1, pose2) and all(torch.equal(a, b) for a, b in zip(warped1, warped2)), 'a cache kept the weights of before the step'
    assert not torch.equal(pose0, pose1) and not torch.equal(warped0[-1], warped1[-1])
    return model


def test_forward_after_a_fused_step_uses_the_stepped_weights_modelnet():
    from regtr_amd.augment import modelnet_train_batch
    cfg = load_cfg('modelnet')
    model = _stale_cache_case(cfg, modelnet_train_batch(_points(), cfg, SEED, 0))
    # state only for the parameters that got a gradient: not the frozen kernel_points, not feature_criterion_un.W under wt_feature_un = 0
    # unless autograd handed it zeros
    opt = model.optimizer
    names = {id(p): n for n, p in model.named_parameters()}
    with_state = {names[id(p)] for p in opt.state}
    assert not any(n.endswith('kernel_points') for n in with_state)
    assert with_state == {n for n, p in model.named_parameters() if p.grad is not None}
    assert any(n.startswith('kpf_encoder.') for n in with_state) and len(with_state) >= 139


def test_forward_after_a_fused_step_uses_the_stepped_weights_3dmatch():
    from tests.test_gpu_losses import _golden_batch
    from tests.util import gold
    cfg = load_cfg('3dmatch')
    case = '3dmatch_crop_b2'
    srcs, tgts, extra = _golden_batch(gold(f'losses_{case}'), case)
    batch = dict({'src_xyz': [torch.from_numpy(x).cuda() for x in srcs], 'tgt_xyz': [torch.from_numpy(x).cuda() for x in tgts]}, **extra)
    _stale_cache_case(cfg, batch)


@pytest.mark.parametrize('name,n_params', [('modelnet', 146), ('3dmatch', 168)])
def test_configure_optimizers(name, n_params):
    from regtr_amd import RegTR
    from regtr_amd.optim import FusedAdamW
    cfg = load_cfg(name)
    model = RegTR(cfg).cuda()
    opt, sched = model.configure_optimizers()
    assert type(opt) is FusedAdamW and opt is model.optimizer and sched is model.scheduler and opt.decoupled
    g = opt.param_groups[0]
    assert g['lr'] == 1e-4 and g['weight_decay'] == 1e-4 and opt.max_grad_norm == 0.1      # (torch's default decay would be 1e-2)
    assert len(g['params']) == n_params and all(a is b for a, b in zip(g['params'], model.parameters()))
    assert isinstance(sched, torch.optim.lr_scheduler.StepLR) and sched.gamma == 0.5 and len(opt.state) == 0
    cfg.optimizer = 'Adam'
    cfg.scheduler = 'none'
    m2 = RegTR(cfg).cuda()
    opt2, sched2 = m2.configure_optimizers()
    assert not opt2.decoupled and (sched2.step_size, sched2.gamma) == (50, 1.0)
    w = m2.feat_proj.weight
    w.grad = torch.ones_like(w)
    before = w.detach().clone()
    opt2.step()                                                                              # Adam works: one step moves the weight
    assert len(opt2.state) == 1 and w in opt2.state and not torch.equal(w.detach(), before) and torch.isfinite(w).all()
    for key, val in (('scheduler', 'warmup'), ('optimizer', 'SGD')):
        bad = load_cfg(name)
        bad[key] = val
        with pytest.raises(NotImplementedError):
            RegTR(bad).configure_optimizers()


def _five_steps(cfg):
    from regtr_amd.augment import modelnet_train_batch
    model = _fresh_model(cfg)
    model.configure_optimizers()
    totals = []
    for step in range(5):
        batch = modelnet_train_batch(_points(), cfg, SEED, step)
        model.optimizer.zero_grad()
        _, losses = model.training_step(batch, train_backbone=True)
        losses['total'].backward()
        model.optimizer.step()
        model.scheduler.step()
        totals.append(losses['total'].detach())
    return model, [float(t) for t in totals]


def test_five_fused_steps_lower_the_total_and_repeat_bit_for_bit():
    cfg = load_cfg('modelnet')
    m1, totals = _five_steps(cfg)
    print('totals over five fused steps:', [f'{t:.4f}' for t in totals], 'last gradient norm', float(m1.optimizer.last_grad_norm))
    assert all(np.isfinite(totals)) and totals[-1] < totals[0]
    assert all(torch.isfinite(p).all() for p in m1.parameters())
    m2, totals2 = _five_steps(cfg)
    assert totals2 == totals
    assert all(torch.equal(a, b) for a, b in zip(m1.parameters(), m2.parameters()))


def _train(tmp, name, *args):
    """train.py as a fresh child process under its own time limit; --dev logs to ../logdev relative to the working directory."""
    cwd = os.path.join(tmp, name, 'work')
    os.makedirs(cwd, exist_ok=True)
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--config', os.path.join(ROOT, 'regtr_amd', 'conf', 'modelnet.yaml'),
           '--synthetic', '4', '--batch', '2', '--num_workers', '0', '--dev', '--validate_every', '2', *args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(tmp, name, 'logdev', 'ckpt')


def test_train_py_resume_equals_the_unbroken_run(tmp_path):
    tmp = str(tmp_path)
    full = _train(tmp, 'full', '--steps', '4')
    part = _train(tmp, 'part', '--steps', '2')
    assert open(os.path.join(part, 'checkpoints.txt')).readline().strip() == 'Best step: 2'
    assert sorted(f for f in os.listdir(part) if f.endswith('.pth')) == ['model-2.pth']
    resumed = _train(tmp, 'part', '--steps', '2', '--resume', part)
    assert resumed == part
    first = open(os.path.join(full, 'checkpoints.txt')).readline()
    assert first.startswith('Best step: ') and int(first.split(':')[1]) in (2, 4)
    a = torch.load(os.path.join(full, 'model-4.pth'), map_location='cpu', weights_only=False)
    b = torch.load(os.path.join(part, 'model-4.pth'), map_location='cpu', weights_only=False)
    assert sorted(a) == sorted(b) == ['optimizer', 'scheduler', 'state_dict', 'step'] and a['step'] == b['step'] == 4
    assert list(a['state_dict']) == list(b['state_dict'])
    assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])
    sa, sb = a['optimizer']['state'], b['optimizer']['state']
    assert sorted(sa) == sorted(sb) and len(sa) >= 139
    for k in sa:
        assert float(sa[k]['step']) == float(sb[k]['step']) == 4.0
        assert torch.equal(sa[k]['exp_avg'], sb[k]['exp_avg']) and torch.equal(sa[k]['exp_avg_sq'], sb[k]['exp_avg_sq'])
    assert a['optimizer']['param_groups'] == b['optimizer']['param_groups'] and a['scheduler'] == b['scheduler']
    assert a['scheduler']['last_epoch'] == 4
    from regtr_amd import RegTR
    RegTR(load_cfg('modelnet')).load_state_dict(a['state_dict'], strict=True)
    # the two-step checkpoint differs: the resumed steps did something
    c = torch.load(os.path.join(full, 'model-2.pth'), map_location='cpu', weights_only=False)
    assert not torch.equal(c['state_dict']['feat_proj.weight'], a['state_dict']['feat_proj.weight'])
