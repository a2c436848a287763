"""GPU: skip_nonfinite in harness.train_loop and train.py -- a stand-in module whose gradient the batch's data makes infinite, the plain
and the bucket path, the finite-only loss statistics, three guarded steps of the real ModelNet model, and train.py's resume."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import ROOT, load_cfg

pytestmark = pytest.mark.gpu


class Toy(torch.nn.Module):
    """Two parameters (4097 and 5 elements), the duck type train_loop needs.  total = scale * (w . x + sum(b) - y)^2, so its gradient is
    scale * 2 r x: a batch with scale = inf makes it +-inf / NaN through the DATA alone.  'aux' is a second loss key outside the total:
    NaN when the batch says so, with the gradients untouched."""

    def __init__(self, guarded=True, seed=3, lr_every=50):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(4097, generator=g))
        self.b = torch.nn.Parameter(torch.randn(5, generator=g))
        self.guarded, self.lr_every = guarded, lr_every
        self.optimizer = self.scheduler = None

    def configure_optimizers(self, train_backbone=True):
        from regtr_amd.optim import FusedAdamW
        self.optimizer = FusedAdamW(list(self.parameters()), lr=1e-2, weight_decay=1e-2, max_grad_norm=0.1,
                                    **({'skip_nonfinite': True} if self.guarded else {}))
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, self.lr_every, 0.5)
        return self.optimizer, self.scheduler

    def training_step(self, batch, step=None, train_backbone=True):
        r = (self.w * batch['x']).sum() + self.b.sum() - batch['y']
        total = batch['scale'] * r * r
        aux = r.detach().abs() + (float('nan') if batch.get('nan_aux', False) else 0.0)
        return None, {'aux': aux, 'total': total}


def _batch(i, scale=1.0, nan_aux=False):
    g = torch.Generator().manual_seed(100 + i)
    return {'x': torch.randn(4097, generator=g).cuda(), 'y': torch.tensor(float(i), device='cuda'),
            'scale': torch.tensor(scale, device='cuda'), 'nan_aux': nan_aux}


def _state(model):
    opt = model.optimizer
    return [t.detach().clone() for p in model.parameters() for t in (p, opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'], opt.state[p]['step'])]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _grad_of(model, batch):
    model.optimizer.zero_grad()
    _, losses = model.training_step(batch)
    losses['total'].backward()
    return [p.grad.clone() for p in model.parameters()], losses


def test_flag_needs_a_guarded_optimiser_and_flag_off_keeps_its_keys():
    from regtr_amd import harness
    with pytest.raises(RuntimeError, match='skip_nonfinite'):
        harness.train_loop(Toy(guarded=False).cuda(), [_batch(1)], 1, skip_nonfinite=True)
    out = harness.train_loop(Toy(guarded=False).cuda(), [_batch(1), _batch(2)], 2)
    assert sorted(out) == ['loss_avg', 'loss_smooth', 'scores', 'step', 'validation']


def _logged(fn):
    records = []
    logger = logging.getLogger('tests.nonfinite_guard_loop')
    logger.setLevel(logging.INFO)
    handler = logging.Handler()
    handler.emit = lambda rec: records.append(rec.getMessage())
    logger.addHandler(handler)
    try:
        return fn(logger), records
    finally:
        logger.removeHandler(handler)


def test_plain_path_skips_the_bad_batch_and_leaves_no_trace():
    from regtr_amd import harness
    b1, b2, bad = _batch(1), _batch(2), _batch(9, scale=float('inf'))
    a, b = Toy().cuda(), Toy().cuda()
    out_a, records = _logged(lambda lg: harness.train_loop(a, [b1, bad, b2], 3, skip_nonfinite=True, logger=lg, log_every=1))
    out_b = harness.train_loop(b, [b1, b2], 2, skip_nonfinite=True)
    assert _same(_state(a), _state(b))                                         # weights, moments and the Adam step counts
    assert int(out_a['skipped_steps']) == 1 and int(out_a['skipped_micro_batches']) == 1 and out_a['step'] == 3
    assert int(out_b['skipped_steps']) == 0 and out_b['step'] == 2
    assert out_a['skipped_steps'].is_cuda and out_a['skipped_micro_batches'].is_cuda
    assert [float(a.optimizer.state[p]['step']) for p in a.parameters()] == [2.0, 2.0]
    assert a.scheduler.last_epoch == 3 and b.scheduler.last_epoch == 2         # the scheduler went on over the skipped step
    assert all(torch.isfinite(p).all() for p in a.parameters())
    assert sorted(out_a) == ['loss_avg', 'loss_smooth', 'scores', 'skipped_micro_batches', 'skipped_steps', 'step', 'validation']
    assert len(records) == 3 and 'skipped steps 0, skipped micro-batches 0' in records[0] and 'skipped steps 1, skipped micro-batches 1' in records[2]
    assert torch.isfinite(out_a['loss_smooth'])
    assert torch.equal(out_a['loss_avg']['total'], out_b['loss_avg']['total']) # the skipped step's losses are left out of the mean
    # a scheduler that decays INSIDE the run: the skipped step advanced it (GradScaler's semantics), so b2 is stepped with the learning
    # rate of global step 3 -- the reference is built by hand with that schedule
    c, d = Toy(lr_every=2).cuda(), Toy(lr_every=2).cuda()
    out_c = harness.train_loop(c, [b1, bad, b2], 3, skip_nonfinite=True)
    d.configure_optimizers()
    for i, batch in enumerate([b1, None, b2]):
        if batch is not None:
            d.optimizer.zero_grad()
            _, losses = d.training_step(batch, i + 1)
            losses['total'].backward()
            d.optimizer.step()
        d.scheduler.step()
    assert _same(_state(c), _state(d)) and int(out_c['skipped_steps']) == 1
    assert c.optimizer.param_groups[0]['lr'] == 5e-3 and not _same(_state(c), _state(a))
    # BAD first: the guard word does not exist before the first step
    e, f = Toy().cuda(), Toy().cuda()
    out_e = harness.train_loop(e, [bad, b1], 2, skip_nonfinite=True)
    out_f = harness.train_loop(f, [b1], 1, skip_nonfinite=True)
    assert _same(_state(e), _state(f)) and int(out_e['skipped_steps']) == 1 and int(out_f['skipped_steps']) == 0
    assert torch.equal(out_e['loss_avg']['total'], out_f['loss_avg']['total'])


def test_a_nan_loss_with_finite_gradients_is_applied_and_left_out_of_the_mean():
    from regtr_amd import harness
    batches = [_batch(1), _batch(2, nan_aux=True), _batch(3)]
    a, b = Toy().cuda(), Toy().cuda()
    out = harness.train_loop(a, batches, 3, skip_nonfinite=True)
    ref = harness.train_loop(b, [_batch(1), _batch(2), _batch(3)], 3, skip_nonfinite=True)
    assert int(out['skipped_steps']) == 0 and _same(_state(a), _state(b))      # applied, not skipped
    assert [float(a.optimizer.state[p]['step']) for p in a.parameters()] == [3.0, 3.0]
    # the mean over the finite values: steps 1 and 3 of the reference run's 'aux'
    c = Toy().cuda()
    c.configure_optimizers()
    auxes = []
    for i, batch in enumerate([_batch(1), _batch(2), _batch(3)]):
        c.optimizer.zero_grad()
        _, losses = c.training_step(batch, i + 1)
        losses['total'].backward()
        c.optimizer.step(); c.scheduler.step()
        auxes.append(losses['aux'])
    assert torch.isfinite(out['loss_avg']['aux']) and torch.equal(out['loss_avg']['aux'], (auxes[0] + auxes[2]) / 2.0)
    assert torch.equal(out['loss_avg']['total'], ref['loss_avg']['total'])
    # flag off, the same batches: the NaN reaches the average (what the flag is for)
    off = harness.train_loop(Toy(guarded=False).cuda(), batches, 3)
    assert torch.isnan(off['loss_avg']['aux'])


def test_bucket_path_k2_equals_the_hand_built_steps():
    """K = 2 over [b1, BAD, b2, b3]: step 1 holds g1 / 2 alone and grad_scale = 2 / 1, step 2 holds fma(1/2, g3, g2 / 2) and
    grad_scale = 1 -- built by hand with a guarded optimiser, as the bucket tests do."""
    from regtr_amd import harness
    b1, bad, b2, b3 = _batch(1), _batch(9, scale=float('inf')), _batch(2), _batch(3, nan_aux=True)
    a, b = Toy().cuda(), Toy().cuda()
    out = harness.train_loop(a, [b1, bad, b2, b3], 2, accumulate=2, skip_nonfinite=True)
    assert out['step'] == 2 and int(out['skipped_steps']) == 0 and float(out['skipped_micro_batches']) == 1.0
    b.configure_optimizers()
    opt = b.optimizer
    g1, l1 = _grad_of(b, b1)
    for p, g in zip(b.parameters(), g1):
        p.grad = 0.5 * g
    opt.grad_scale = torch.tensor([2.0], device='cuda')
    opt.step(); b.scheduler.step()
    g2, l2 = _grad_of(b, b2)
    g3, l3 = _grad_of(b, b3)
    for p, x, y in zip(b.parameters(), g2, g3):
        p.grad = 0.5 * x + 0.5 * y                                             # (halving is exact: one rounding, as the bucket's fma)
    opt.grad_scale = torch.tensor([1.0], device='cuda')
    opt.step(); b.scheduler.step()
    assert _same(_state(a), _state(b))
    # loss statistics: 'total' over the three good micro-batches as ratios per step, 'aux' without b3's NaN
    assert torch.isfinite(out['loss_avg']['total']) and torch.isfinite(out['loss_avg']['aux'])
    want_total = (0.5 * l1['total'].detach() + (0.5 * l2['total'].detach() + 0.5 * l3['total'].detach())) / (0.5 + 1.0)
    assert abs(float(out['loss_avg']['total']) - float(want_total)) <= 4 * 2.0 ** -24 * abs(float(want_total))
    want_aux = (0.5 * l1['aux'] + 0.5 * l2['aux']) / (0.5 + 0.5)
    assert abs(float(out['loss_avg']['aux']) - float(want_aux)) <= 4 * 2.0 ** -24 * abs(float(want_aux))


def test_three_guarded_steps_of_the_real_model():
    from regtr_amd import RegTR, harness
    from regtr_amd.augment import modelnet_train_batch
    from tests.test_gpu_training_loop import SEED, _points
    from tests.util import seeded_sd
    runs = {}
    for guarded in (True, False):
        cfg = load_cfg('modelnet')
        if guarded:
            cfg['skip_nonfinite'] = True
        model = RegTR(cfg)
        model.load_state_dict(seeded_sd(cfg), strict=True)
        model = model.cuda().eval()
        model.configure_optimizers()
        assert model.optimizer.skip_nonfinite is guarded
        totals = []
        batches = (modelnet_train_batch(_points(), cfg, SEED, step) for step in range(3))

        def tapped(batch, step, train_backbone=True, _f=model.training_step):  # records every step's total (no host read in the loop)
            pred, losses = _f(batch, step, train_backbone=train_backbone)
            totals.append(losses['total'].detach())
            return pred, losses
        model.training_step = tapped
        out = harness.train_loop(model, batches, 3, **({'skip_nonfinite': True} if guarded else {}))
        runs[guarded] = (model, out, [float(t) for t in totals])
    (on, out_on, tot_on), (off, out_off, tot_off) = runs[True], runs[False]
    print('totals, flag on:', tot_on, 'flag off:', tot_off)
    assert int(out_on['skipped_steps']) == 0 and int(out_on['skipped_micro_batches']) == 0 and 'skipped_steps' not in out_off
    assert all(torch.isfinite(p).all() for p in on.parameters())
    assert all(np.isfinite(tot_on)) and tot_on[0] == tot_off[0]                # the first forward: the same weights
    assert tot_on[-1] < tot_on[0] and tot_off[-1] < tot_off[0]                 # the total falls, as in the flag-off run
    assert all(int(on.optimizer.state[p]['step']) == 3 and on.optimizer.state[p]['step'].is_cuda for p in on.optimizer.state)


# ---------------------------------------------------------------------------------------------------------------- train.py
def _train(tmp, name, *args):
    """train.py as a fresh child process under its own time limit, with the arguments of tests/test_gpu_training_loop.py's resume test."""
    cwd = os.path.join(tmp, name, 'work')
    os.makedirs(cwd, exist_ok=True)
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--config', os.path.join(ROOT, 'regtr_amd', 'conf', 'modelnet.yaml'),
           '--synthetic', '4', '--batch', '2', '--num_workers', '0', '--dev', '--validate_every', '2', '--skip_nonfinite', *args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    return os.path.join(tmp, name, 'logdev', 'ckpt'), r.stderr


def test_train_py_skip_nonfinite_resume_equals_the_unbroken_run(tmp_path):
    tmp = str(tmp_path)
    full, log = _train(tmp, 'full', '--steps', '4')
    assert 'skipped steps 0, skipped micro-batches 0' in log
    part, _ = _train(tmp, 'part', '--steps', '2')
    resumed, _ = _train(tmp, 'part', '--steps', '2', '--resume', part)
    assert resumed == part
    a = torch.load(os.path.join(full, 'model-4.pth'), map_location='cpu', weights_only=False)
    b = torch.load(os.path.join(part, 'model-4.pth'), map_location='cpu', weights_only=False)
    assert sorted(a) == sorted(b) == ['nonfinite_guard', 'optimizer', 'scheduler', 'state_dict', 'step'] and a['step'] == b['step'] == 4
    assert a['nonfinite_guard'] == b['nonfinite_guard'] == {'skipped_steps': 0, 'skipped_micro_batches': 0}
    assert list(a['state_dict']) == list(b['state_dict'])
    assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])
    sa, sb = a['optimizer']['state'], b['optimizer']['state']
    assert sorted(sa) == sorted(sb) and len(sa) >= 139
    for k in sa:
        assert float(sa[k]['step']) == float(sb[k]['step']) == 4.0
        assert torch.equal(sa[k]['exp_avg'], sb[k]['exp_avg']) and torch.equal(sa[k]['exp_avg_sq'], sb[k]['exp_avg_sq'])
    assert a['optimizer']['param_groups'] == b['optimizer']['param_groups'] and a['scheduler'] == b['scheduler']
    c = torch.load(os.path.join(full, 'model-2.pth'), map_location='cpu', weights_only=False)
    assert not torch.equal(c['state_dict']['feat_proj.weight'], a['state_dict']['feat_proj.weight'])
    # the checkpoint loads into torch.optim.AdamW over the model's parameters (device step counts and all)
    from regtr_amd import RegTR
    model = RegTR(load_cfg('modelnet'))
    model.load_state_dict(a['state_dict'], strict=True)
    torch.optim.AdamW(list(model.parameters())).load_state_dict(a['optimizer'])
