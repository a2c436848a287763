"""CPU: tests/optim_ref.py pinned to the calls the reference makes -- torch.nn.utils.clip_grad_norm_, torch.optim.AdamW / Adam and
StepLR on CPU float64 tensors -- and its one-step float32 error bound checked against a numpy float32 replay of the kernel's operation
order and against torch's own float32 step; the host-side contracts of the optimiser wrappers, FusedAdamW, configure_optimizers and
train.py that need no GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.util import ROOT, load_cfg

SHAPES = [(5,), (3, 4), (1,), (7, 2)]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize('decoupled', [True, False])
@pytest.mark.parametrize('clip', ['on', 'off', 'inactive'])
def test_restatement_equals_torch_float64(decoupled, clip):
    """Six steps; tensor 1 has no gradient on step 3 only; StepLR(2, 0.5) drops the lr twice inside the run; clipping active
    (max_norm far below the norms), off (no clip call), inactive (coef = 1).  1e-12 of every tensor's largest entry."""
    rng = np.random.default_rng(3)
    p0 = [rng.standard_normal(s) for s in SHAPES]
    max_norm = {'on': 0.05, 'off': 0.0, 'inactive': 1e6}[clip]
    lr, wd, betas, eps = 3e-2, 1e-1, (0.9, 0.999), 1e-8
    tp = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in p0]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(tp, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    ref = R.AdamRef(p0, lr=lr, betas=betas, eps=eps, weight_decay=wd, max_grad_norm=max_norm, decoupled=decoupled)
    for step in range(1, 7):
        grads = [rng.standard_normal(s) * 10.0 ** rng.integers(-3, 2) for s in SHAPES]
        if step == 3:
            grads[1] = None
        for t, g in zip(tp, grads):
            t.grad = None if g is None else torch.tensor(g, dtype=torch.float64)
        want_norm = None
        if clip != 'off':
            want_norm = float(torch.nn.utils.clip_grad_norm_(tp, max_norm=max_norm))
        opt.step()
        cur_lr = R.step_lr(lr, 2, 0.5, step - 1)
        assert abs(cur_lr - opt.param_groups[0]['lr']) <= 1e-15 * lr
        norm, coef = ref.step(grads, lr=cur_lr)
        sched.step()
        if want_norm is not None:
            assert abs(norm - want_norm) <= 1e-12 * want_norm
            assert (coef < 1.0) == (clip == 'on')
        for i, t in enumerate(tp):
            assert _rel(ref.p[i], t.detach().numpy()) <= 1e-12, (step, i)
            st = opt.state[t]
            assert int(st['step']) == ref.t[i]
            assert _rel(ref.m[i], st['exp_avg'].numpy()) <= 1e-12 and _rel(ref.v[i], st['exp_avg_sq'].numpy()) <= 1e-12
    assert ref.t == [6, 5, 6, 6] and abs(opt.param_groups[0]['lr'] - lr * 0.125) <= 1e-15


def test_clip_coef_edge_cases_equal_torch():
    """max_norm / (norm + 1e-6) clamped from above: an infinite norm gives 0 (and inf * 0 = NaN in the update, as with torch), a NaN
    norm a NaN."""
    for norm in (0.0, 0.05, 0.1, 3.0, float('inf'), float('nan')):
        want = float(torch.clamp(0.1 / (torch.tensor(norm, dtype=torch.float64) + 1e-6), max=1.0))
        got = R.clip_coef(norm, 0.1)
        assert (got != got and want != want) or abs(got - want) <= 1e-15 * want, (norm, got, want)
    assert R.clip_coef(5.0, 0.0) == 1.0 and R.clip_coef(float('nan'), -1.0) == 1.0


def _f32_replay(p, g, m, v, coef, lr, wd, b1, b2, eps, t, decoupled):
    """The kernel's operation order in numpy float32, one rounding per operation (csrc/optim.hip: opt_update)."""
    f = np.float32
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    decay, wdf, b1f, o1, b2f, o2 = f(1.0 - lr * wd), f(wd), f(b1), f(1.0 - b1), f(b2), f(1.0 - b2)
    ss, sb, ef = f(lr / (1.0 - b1 ** t)), f(np.sqrt(1.0 - b2 ** t)), f(eps)
    g = g * f(coef)
    if decoupled:
        p = p * decay
    else:
        g = g + wdf * p
    m = b1f * m + o1 * g
    v = b2f * v + (o2 * g) * g
    p = p - ss * (m / (np.sqrt(v) / sb + ef))
    return p, m, v


def wide_gradients(rng, n):
    """Magnitudes from 1e-12 to 1e3, both signs, exact zeros among them."""
    g = (10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.1] = 0.0
    return g


@pytest.mark.parametrize('decoupled', [True, False])
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_float32_replay_and_torch_float32_stay_inside_the_bound(decoupled, t):
    rng = np.random.default_rng(100 + t)
    n = 20000
    g = wide_gradients(rng, n)
    p = rng.standard_normal(n).astype(np.float32)
    first = t == 1
    m = np.zeros(n, np.float32) if first else (wide_gradients(rng, n) * np.float32(0.3))
    v = np.zeros(n, np.float32) if first else (wide_gradients(rng, n) ** 2 * np.float32(0.5)).astype(np.float32)
    v[:50] = 0.0                                          # the v -> 0 end: the denominator is eps
    hp = dict(lr=1e-3, wd=1e-2, b1=0.9, b2=0.999, eps=1e-8)
    for coef in (1.0, float(np.float32(0.0123))):
        want = R.adam_update(p, g, m, v, coef, t=t, decoupled=decoupled, **hp)
        bound = R.step_bound(p, g, m, v, coef, t=t, decoupled=decoupled, **hp)
        got = _f32_replay(p, g, m, v, coef, t=t, decoupled=decoupled, **hp)
        worst = [float(np.max(np.abs(a.astype(np.float64) - w) / b)) for a, w, b in zip(got, want, bound)]
        print(f'float32 replay, t = {t}, decoupled = {decoupled}, coef = {coef}: worst err / bound (p, m, v) = {worst}')
        assert max(worst) <= 1.0
        # the bound is not vacuous: within a small factor of one float32 spacing of the result where the update is benign
        assert float(np.median(bound[0] / np.maximum(np.abs(want[0]), 1e-30))) < 16 * R.U
    # torch's own float32 step (its lerp form of the first moment): inside the same bound
    tp = torch.tensor(p, requires_grad=True)
    tp.grad = torch.tensor(g)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([tp], lr=hp['lr'], betas=(hp['b1'], hp['b2']), eps=hp['eps'], weight_decay=hp['wd'])
    opt.state[tp] = {'step': torch.tensor(float(t - 1)), 'exp_avg': torch.tensor(m), 'exp_avg_sq': torch.tensor(v)}
    opt.step()
    want = R.adam_update(p, g, m, v, 1.0, t=t, decoupled=decoupled, **hp)
    bound = R.step_bound(p, g, m, v, 1.0, t=t, decoupled=decoupled, **hp)
    got = (tp.detach().numpy(), opt.state[tp]['exp_avg'].numpy(), opt.state[tp]['exp_avg_sq'].numpy())
    worst = [float(np.max(np.abs(a.astype(np.float64) - w) / b)) for a, w, b in zip(got, want, bound)]
    print(f'torch float32, t = {t}, decoupled = {decoupled}: worst err / bound (p, m, v) = {worst}')
    assert max(worst) <= 1.0


def test_wrappers_refuse_cpu_tensors_with_a_python_exception():
    from regtr_amd import ops
    p, g, m, v = (torch.zeros(8) for _ in range(4))
    sc = [(1e-3, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.03)]
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.grad_sumsq([g])
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.adam_step([p], [g], [m], [v], sc)


def test_entry_points_refuse_bad_arguments_with_a_status():
    """No launch happens: NULL tables with work to do, negative counts, a partial count that does not follow from the lengths."""
    import ctypes
    from regtr_amd import _lib
    lib = _lib.lib()
    sl, st, ch = lib.regtr_optim_norm_slice(), lib.regtr_optim_step_slice(), lib.regtr_optim_chunk_tensors()
    assert sl > 0 and st > 0 and sl % 1024 == 0 and st % 1024 == 0 and ch * 80 + 16 <= 4096 - 64       # the 4 KiB argument segment
    assert lib.regtr_grad_sumsq(None, 1, None, 0, None) == -2 and lib.regtr_grad_sumsq(None, -1, None, 0, None) == -2
    assert lib.regtr_adam_step(None, 1, None, 1, None) == -2
    assert lib.regtr_grad_norm_finish(None, 0, 0.1, None, None) == -2
    tab = np.zeros(1, dtype=np.dtype([('p', np.uint64), ('g', np.uint64), ('m', np.uint64), ('v', np.uint64), ('n', np.int64),
                                      ('scalars', np.float64, (7,))], align=True))
    tab['n'] = 100
    buf = ctypes.c_double()
    assert lib.regtr_grad_sumsq(tab.ctypes.data, 1, ctypes.addressof(buf), 2, None) == -2             # 100 elements are ONE slice
    assert lib.regtr_grad_sumsq(tab.ctypes.data, 1, ctypes.addressof(buf), 1, None) == -2             # ... and g is NULL
    assert lib.regtr_adam_step(tab.ctypes.data, 1, None, 1, None) == -2                                # bias corrections of 0


def test_fused_adamw_is_a_torch_optimizer_with_torchs_state_layout():
    from regtr_amd.optim import FusedAdamW
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    opt = FusedAdamW(ps, lr=1e-4, weight_decay=1e-4, max_grad_norm=0.1)
    assert isinstance(opt, torch.optim.Optimizer) and opt.max_grad_norm == 0.1 and opt.decoupled
    g = opt.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (1e-4, (0.9, 0.999), 1e-8, 1e-4)
    assert FusedAdamW(ps).defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    assert opt.step() is None and len(opt.state) == 0                      # no gradient anywhere: torch's rule, nothing happens
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    lrs = []
    for _ in range(5):
        lrs.append(opt.param_groups[0]['lr'])
        opt.step(); sched.step()
    assert np.allclose(lrs, [1e-4, 1e-4, 5e-5, 5e-5, 2.5e-5], rtol=1e-12)
    # a torch.optim.AdamW state_dict over the same parameter list loads, and the reverse
    ta = torch.optim.AdamW(ps, lr=1e-4)
    for p in ps:
        p.grad = torch.ones_like(p)
    ta.step()
    opt.load_state_dict(ta.state_dict())
    assert set(opt.state[ps[0]]) == {'step', 'exp_avg', 'exp_avg_sq'} and float(opt.state[ps[0]]['step']) == 1.0
    tb = torch.optim.AdamW(ps, lr=1e-4)
    tb.load_state_dict(opt.state_dict())
    tb.step()
    assert float(tb.state[ps[1]]['step']) == 2.0
    ps[0].grad = torch.ones_like(ps[0])
    with pytest.raises(RuntimeError, match='GPU tensor'):                  # a CPU parameter WITH a gradient: refused, not computed elsewhere
        opt.step()


@pytest.mark.parametrize('name,n_params', [('modelnet', 146), ('3dmatch', 168)])
def test_configure_optimizers(name, n_params):
    from regtr_amd import RegTR
    from regtr_amd.optim import FusedAdamW
    cfg = load_cfg(name)
    model = RegTR(cfg)
    opt, sched = model.configure_optimizers()
    assert opt is model.optimizer and sched is model.scheduler and type(opt) is FusedAdamW and opt.decoupled
    g = opt.param_groups[0]
    assert g['lr'] == 1e-4 and g['weight_decay'] == 1e-4 and opt.max_grad_norm == 0.1
    assert len(g['params']) == n_params and all(a is b for a, b in zip(g['params'], model.parameters()))
    assert isinstance(sched, torch.optim.lr_scheduler.StepLR) and sched.step_size == cfg.scheduler_param[0] and sched.gamma == 0.5
    if hasattr(model.feature_criterion, 'W'):
        assert model.feature_criterion.W.requires_grad and model.feature_criterion_un.W.requires_grad
    cfg.optimizer = 'Adam'
    cfg.scheduler = 'none'
    opt, sched = RegTR(cfg).configure_optimizers(train_backbone=False)
    assert not opt.decoupled and (sched.step_size, sched.gamma) == (50, 1.0)
    for key, val in (('scheduler', 'warmup'), ('optimizer', 'SGD'), ('scheduler', 'cosine')):
        bad = load_cfg(name)
        bad[key] = val
        with pytest.raises(NotImplementedError):
            RegTR(bad).configure_optimizers()


def test_train_py_exits_with_a_message_without_a_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES='')      # (the child sees no device on any box)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), '--config', os.path.join(ROOT, 'regtr_amd', 'conf', 'modelnet.yaml'),
                        '--synthetic', '4', '--dev'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and 'no CPU path' in (r.stderr + r.stdout)
