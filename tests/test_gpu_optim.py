"""GPU: the optimiser step's kernels (csrc/optim.hip) and regtr_amd.optim.FusedAdamW against the float64 restatement of
clip_grad_norm_ + AdamW / Adam (tests/optim_ref.py, pinned to the torch calls by tests/test_optim_host.py) and its derived one-step
float32 bound.

Tensor lengths: 1, 3, 255, 256, 257, 1023, 4097, the largest real tensor (983040), and one on each side of both slice sizes (the norm's
and the step's).  Tensor counts per call: one, exactly one chunk of the by-value descriptor, one chunk plus one.

BOUNDS of the norm half.  A partial is a float64 sum of at most S products of float32 numbers (each exact in float64): relative error
below (S + 8) 2^-53.  total_norm is the float64 sum of the partials (relative error again ~ P 2^-53, P partials), its float64 square root
and ONE rounding to float32: |total_norm - exact| <= 2^-24 exact (1 + 2^-20) -- half a float32 spacing, the float64 part hides in the
2^-20.  clip_coef = fl(fl(max_norm) / fl(total_norm + fl(1e-6))): five roundings, |coef - exact| <= 5 * 2^-24 exact (1 + 2^-20)."""
import copy

import numpy as np
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu

U = R.U
BIG = 983040
HP = dict(lr=1e-3, wd=1e-2, b1=0.9, b2=0.999, eps=1e-8)
COEF_REL = 6 * U            # a float32 coefficient from the kernels against the float64 one (5u, see above) with room for its own rounding


def _slices():
    from regtr_amd import ops
    return ops.optim_slices()


def _lengths():
    ns, ss, _ = _slices()
    return sorted({1, 3, 255, 256, 257, 1023, 4097, BIG, ns - 1, ns + 1, ss - 1, ss + 1})


def _call_configs():
    """Lists of tensor lengths, one list per call: every length alone, one full chunk, one chunk plus one (the big tensor in it)."""
    _, _, ch = _slices()
    small = [n for n in _lengths() if n != BIG]
    cyc = [small[i % len(small)] for i in range(ch + 1)]
    return [[n] for n in _lengths()] + [cyc[:ch], [BIG] + cyc[:ch]]


def _wide(rng, n):
    """Gradients spanning 1e-12 to 1e3, both signs, exact zeros among them."""
    g = (10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g[rng.random(n) < 0.1] = 0.0
    return g


def _dev(a, offset=0, guard=0):
    """a on the device inside a longer buffer: `offset` float32 in front (offset 1: the view starts 4 bytes off a 16-byte boundary),
    `guard` elements of 12345 behind.  -> (view, buffer)"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1)
    buf = torch.full((offset + a.size + guard,), 12345.0, dtype=torch.float32, device='cuda')
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view, buf


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- the norm
def test_grad_norm_against_float64():
    from regtr_amd import ops
    ns, _, _ = _slices()
    rng = np.random.default_rng(5)
    for lens in _call_configs():
        host = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32) for n in lens]
        grads = [_dev(h)[0] for h in host]
        partials = ops.grad_sumsq(grads)
        want_p = np.concatenate([[np.sum(h[i:i + ns].astype(np.float64) ** 2) for i in range(0, len(h), ns)] for h in host])
        assert partials.shape == want_p.shape                                              # one partial per slice: a function of the lengths
        assert np.all(np.abs(_f64(partials) - want_p) <= (ns + 8) * 2.0 ** -53 * want_p)
        want = R.total_norm(host)
        for max_norm in (0.1, 0.0, 1e9):
            out = ops.grad_norm_finish(partials, max_norm)
            norm, coef = (float(x) for x in out.cpu())
            wc = R.clip_coef(want, max_norm)
            assert abs(norm - want) <= U * want * (1 + 2.0 ** -20), (lens[:3], norm, want)
            if max_norm == 0.1:
                assert abs(coef - wc) <= 5 * U * wc * (1 + 2.0 ** -20), (coef, wc)
                if want + 1e-6 < 0.1 * (1 - 8 * U):
                    assert coef == 1.0                                                     # the norm below max_norm: exactly 1
            else:
                assert coef == 1.0                                                         # no clipping / the norm below max_norm: exactly 1
        # the same call again: the same bits
        assert torch.equal(ops.grad_sumsq(grads), partials)
        assert torch.equal(ops.grad_norm_finish(partials, 0.1), ops.grad_norm_finish(partials, 0.1))


def test_grad_norm_edge_cases():
    from regtr_amd import ops
    ns, _, _ = _slices()
    n = ns + 257
    zeros = torch.zeros(n, device='cuda')
    out = ops.grad_norm_finish(ops.grad_sumsq([zeros, zeros[:3]]), 0.1).cpu()
    assert float(out[0]) == 0.0 and float(out[1]) == 1.0                                   # all zero: norm 0, coef exactly 1
    g = torch.ones(n, device='cuda')
    g[ns + 5] = float('inf')
    out = ops.grad_norm_finish(ops.grad_sumsq([g]), 0.1).cpu()
    want = torch.clamp(0.1 / (torch.tensor(float('inf')) + 1e-6), max=1.0)                 # clip_grad_norm_'s lines: 0.1 / inf = 0
    assert torch.isinf(out[0]) and float(out[1]) == float(want) == 0.0
    g[3] = float('nan')
    out = ops.grad_norm_finish(ops.grad_sumsq([g]), 0.1).cpu()
    assert torch.isnan(out[0]) and torch.isnan(out[1])                                     # a NaN norm: a NaN coefficient, as torch.clamp keeps it
    assert float(ops.grad_norm_finish(ops.grad_sumsq([g]), 0.0)[1]) == 1.0
    assert ops.grad_sumsq([]).numel() == 0 and ops.grad_norm_finish(ops.grad_sumsq([]), 0.1).cpu().tolist() == [0.0, 1.0]


def test_grad_norm_of_a_misaligned_view_equals_its_aligned_copy():
    from regtr_amd import ops
    rng = np.random.default_rng(6)
    for n in _lengths():
        h = rng.standard_normal(n).astype(np.float32)
        aligned, _ = _dev(h)
        view, _ = _dev(h, offset=1)
        assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
        a, b = ops.grad_sumsq([aligned]), ops.grad_sumsq([view])
        assert torch.equal(a, b), n
        strided = torch.stack([view, view], dim=1)[:, 0]                                   # a non-contiguous gradient is made contiguous
        assert (n == 1 or not strided.is_contiguous()) and torch.equal(ops.grad_sumsq([strided]), a)


# ---------------------------------------------------------------------------------------------------------------- the update
def _state(rng, n, t):
    p = rng.standard_normal(n).astype(np.float32)
    g = _wide(rng, n)
    if t == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    m = (_wide(rng, n) * np.float32(0.3)).astype(np.float32)
    v = (_wide(rng, n).astype(np.float64) ** 2 * 0.5).astype(np.float32)
    v[: max(1, n // 50)] = 0.0                                                             # the v -> 0 end
    return p, g, m, v


def _worst(got, want, bound):
    return max(float(np.max(np.abs(_f64(a) - w) / b)) for a, w, b in zip(got, want, bound))


@pytest.mark.parametrize('clip', [False, True])
@pytest.mark.parametrize('decoupled', [True, False])
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_adam_step_against_float64(t, decoupled, clip):
    from regtr_amd import ops
    rng = np.random.default_rng(1000 * t + 10 * decoupled + clip)
    coef32 = torch.tensor([0.0123], dtype=torch.float32, device='cuda') if clip else None
    coef = float(np.float32(0.0123)) if clip else 1.0
    worst = 0.0
    for ci, lens in enumerate(_call_configs()):
        host = [_state(rng, n, t) for n in lens]
        # every third tensor sits 4 bytes off a 16-byte boundary (the scalar path); guards behind every p, m, v
        dev = [[_dev(x, offset=int(i % 3 == 1), guard=8) for x in st] for i, st in enumerate(host)]
        outside_host = _state(rng, 777, 2)
        outside = [_dev(x)[0] for x in outside_host]
        # per-tensor scalars: tensor i carries its own step count (t, t + 1, ...) and lr
        ts = [t + (i % 2) for i in range(len(lens))]
        lrs = [HP['lr'] * (1 + i % 3) for i in range(len(lens))]
        scalars = [(lrs[i], HP['wd'], HP['b1'], HP['b2'], HP['eps'], 1.0 - HP['b1'] ** ts[i], np.sqrt(1.0 - HP['b2'] ** ts[i]))
                   for i in range(len(lens))]
        g_before = [d[1][0].clone() for d in dev]
        ops.adam_step([d[0][0] for d in dev], [d[1][0] for d in dev], [d[2][0] for d in dev], [d[3][0] for d in dev], scalars,
                      clip_coef=coef32, decoupled=decoupled)
        for i, (st, d) in enumerate(zip(host, dev)):
            hp = dict(HP, lr=lrs[i])
            want = R.adam_update(*st, coef, t=ts[i], decoupled=decoupled, **hp)
            bound = R.step_bound(*st, coef, t=ts[i], decoupled=decoupled, **hp)
            w = _worst((d[0][0], d[2][0], d[3][0]), want, bound)
            worst = max(worst, w)
            assert w <= 1.0, (lens[i], i, w)
            for k in (0, 2, 3):                                                            # the guards behind p, m, v; the slot in front
                off = int(i % 3 == 1)
                assert bool((d[k][1][off + lens[i]:] == 12345.0).all()) and (off == 0 or float(d[k][1][0]) == 12345.0)
            assert torch.equal(d[1][0], g_before[i])                                       # the gradient is read only
        assert all(torch.equal(o, torch.from_numpy(h).cuda()) for o, h in zip(outside, outside_host))
    print(f'regtr_adam_step t = {t} decoupled = {decoupled} clip = {clip}: worst err / bound = {worst:.3f}')


def test_adam_step_refusals():
    from regtr_amd import ops
    z = lambda *s: torch.zeros(*s, device='cuda')
    sc = [(1e-3, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0.03)]
    with pytest.raises(RuntimeError, match='float32'):
        ops.adam_step([z(8).double()], [z(8).double()], [z(8).double()], [z(8).double()], sc)
    with pytest.raises(RuntimeError, match='float32'):
        ops.grad_sumsq([z(8).half()])
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.adam_step([z(4, 4).t()], [z(4, 4)], [z(4, 4)], [z(4, 4)], sc)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.adam_step([z(4, 4)], [z(4, 4)], [z(4, 4)], [z(4, 4).t()], sc)
    with pytest.raises(RuntimeError, match='shape'):
        ops.adam_step([z(4, 4)], [z(16)], [z(4, 4)], [z(4, 4)], sc)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        ops.adam_step([z(8)], [torch.zeros(8)], [z(8)], [z(8)], sc)


# ---------------------------------------------------------------------------------------------------------------- FusedAdamW
SHAPES = [(1,), (3,), (257,), (64, 65), (4097,), (300, 301)]
OPT = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def _params(rng):
    return [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()) for s in SHAPES]


def _grads(rng, skip=()):
    return [None if i in skip else torch.from_numpy((rng.standard_normal(s) * 10.0 ** rng.integers(-4, 1)).astype(np.float32)).cuda()
            for i, s in enumerate(SHAPES)]


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        z = np.zeros(tuple(p.shape))
        out.append((_f64(p), _f64(st['exp_avg']) if st else z, _f64(st['exp_avg_sq']) if st else z, int(st['step']) if st else 0))
    return out


def _check_one_step(before, opt, params, grads, max_norm, decoupled=True, lr=None):
    """Every stepped tensor of `opt` against one float64 step from ITS OWN float32 state `before`, within the bound (the coefficient a
    float32 one: COEF_REL); tensors without a gradient unchanged.  -> worst err / bound."""
    lr = OPT['lr'] if lr is None else lr
    hp = dict(lr=lr, wd=OPT['weight_decay'], b1=OPT['betas'][0], b2=OPT['betas'][1], eps=OPT['eps'])
    coef = R.clip_coef(R.total_norm([None if g is None else _f64(g) for g in grads]), max_norm)
    after = _snapshot(opt, params)
    worst = 0.0
    for (p0, m0, v0, t0), (p1, m1, v1, t1), g in zip(before, after, grads):
        if g is None:
            assert t1 == t0 and np.array_equal(p0, p1) and np.array_equal(m0, m1) and np.array_equal(v0, v1)
            continue
        assert t1 == t0 + 1
        want = R.adam_update(p0, _f64(g), m0, v0, coef, t=t1, decoupled=decoupled, **hp)
        bound = R.step_bound(p0, _f64(g), m0, v0, coef, t=t1, decoupled=decoupled, coef_rel=COEF_REL, **hp)
        worst = max(worst, max(float(np.max(np.abs(a - w) / b)) for a, w, b in zip((p1, m1, v1), want, bound)))
    return worst


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()


@pytest.mark.parametrize('decoupled', [True, False])
def test_fused_adamw_against_the_torch_calls(decoupled):
    """Four steps with the gradient clip active, tensor 1 without a gradient on step 2: FusedAdamW and clip_grad_norm_ + torch.optim.AdamW /
    Adam, each within the bound of the restatement from its own state at every step; step counts and state presence equal."""
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(21)
    mine = _params(rng)
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    max_norm = 0.1
    fused = FusedAdamW(mine, max_grad_norm=max_norm, decoupled=decoupled, **OPT)
    ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(theirs, **OPT)
    worst_f = worst_t = 0.0
    for step in range(1, 5):
        grads = _grads(rng, skip=(1,) if step == 2 else ())
        _set_grads(mine, grads); _set_grads(theirs, grads)
        bf, bt = _snapshot(fused, mine), _snapshot(ref, theirs)
        fused.step()
        torch.nn.utils.clip_grad_norm_(theirs, max_norm=max_norm)
        ref.step()
        worst_f = max(worst_f, _check_one_step(bf, fused, mine, grads, max_norm, decoupled))
        worst_t = max(worst_t, _check_one_step(bt, ref, theirs, grads, max_norm, decoupled))
        want_norm = R.total_norm([None if g is None else _f64(g) for g in grads])
        assert abs(float(fused.last_grad_norm) - want_norm) <= U * want_norm * (1 + 2.0 ** -20)
        assert all(torch.equal(p.grad, g) for p, g in zip(mine, grads) if g is not None)          # p.grad is NOT scaled in place
    dist = max(float((a.detach() - b.detach()).abs().max() / b.detach().abs().max()) for a, b in zip(mine, theirs))
    print(f'FusedAdamW (decoupled = {decoupled}) worst err / bound {worst_f:.3f}; torch {worst_t:.3f}; distance between the two after '
          f'four steps {dist:.2e} of the largest entry')
    assert worst_f <= 1.0 and worst_t <= 1.0
    for a, b in zip(mine, theirs):
        assert float(fused.state[a]['step']) == float(ref.state[b]['step'])
    assert [int(fused.state[p]['step']) for p in mine] == [4, 3, 4, 4, 4, 4]


def test_step_counts_and_state_of_a_parameter_without_a_gradient():
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(22)
    params = _params(rng)
    opt = FusedAdamW(params, max_grad_norm=0.0, **OPT)
    _set_grads(params, _grads(rng, skip=(2, 5)))
    p2 = params[2].detach().clone()
    opt.step()
    assert params[2] not in opt.state and params[5] not in opt.state and torch.equal(params[2].detach(), p2)      # no decay, no state
    assert set(opt.state[params[0]]) == {'step', 'exp_avg', 'exp_avg_sq'} and float(opt.state[params[0]]['step']) == 1.0
    assert float(opt.last_clip_coef) == 1.0
    _set_grads(params, _grads(rng))
    opt.step()
    assert [int(opt.state[p]['step']) for p in params] == [2, 2, 1, 2, 2, 1]


def test_steplr_around_fused_adamw_gives_torchs_lr_sequence():
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(23)
    params = _params(rng)
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in params]
    a, b = FusedAdamW(params, **OPT), torch.optim.AdamW(theirs, **OPT)
    sa, sb = torch.optim.lr_scheduler.StepLR(a, 2, 0.5), torch.optim.lr_scheduler.StepLR(b, 2, 0.5)
    seq = []
    for step in range(6):
        grads = _grads(rng)
        _set_grads(params, grads); _set_grads(theirs, grads)
        before = _snapshot(a, params)
        lr = a.param_groups[0]['lr']
        assert lr == b.param_groups[0]['lr']
        a.step(); b.step(); sa.step(); sb.step()
        assert _check_one_step(before, a, params, grads, 0.0, lr=lr) <= 1.0                       # the kernel steps with the scheduler's lr
        seq.append(lr)
    assert sa.get_last_lr() == sb.get_last_lr() and np.allclose(seq, [1e-3, 1e-3, 5e-4, 5e-4, 2.5e-4, 2.5e-4], rtol=1e-12)


def test_state_dict_interop_with_torch_adamw():
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(24)
    mine = _params(rng)
    fused = FusedAdamW(mine, max_grad_norm=0.1, **OPT)
    for _ in range(2):
        _set_grads(mine, _grads(rng))
        fused.step()
    # FusedAdamW -> torch.optim.AdamW over the same parameter list (clones)
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    ta = torch.optim.AdamW(theirs, **OPT)
    ta.load_state_dict(copy.deepcopy(fused.state_dict()))          # (as a checkpoint's save / load copies: load_state_dict itself aliases the tensors)
    assert all(torch.equal(ta.state[b]['exp_avg'], fused.state[a]['exp_avg']) and float(ta.state[b]['step']) == 2.0 for a, b in zip(mine, theirs))
    # torch.optim.AdamW -> a fresh FusedAdamW
    again = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    fb = FusedAdamW(again, max_grad_norm=0.1, **OPT)
    fb.load_state_dict(copy.deepcopy(ta.state_dict()))
    assert all(set(fb.state[p]) == {'step', 'exp_avg', 'exp_avg_sq'} and fb.state[p]['exp_avg_sq'].is_cuda for p in again)
    grads = _grads(rng)
    for ps in (theirs, again):
        _set_grads(ps, grads)
    bt, bf = _snapshot(ta, theirs), _snapshot(fb, again)
    torch.nn.utils.clip_grad_norm_(theirs, max_norm=0.1)
    ta.step(); fb.step()
    wt, wf = _check_one_step(bt, ta, theirs, grads, 0.1), _check_one_step(bf, fb, again, grads, 0.1)
    print(f'one more step after the state_dict round trip: torch {wt:.3f}, FusedAdamW {wf:.3f} of the bound')
    assert wt <= 1.0 and wf <= 1.0 and [int(fb.state[p]['step']) for p in again] == [3] * len(again)


def test_step_advances_the_version_counters():
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(25)
    params = _params(rng)
    opt = FusedAdamW(params, max_grad_norm=0.1, **OPT)
    _set_grads(params, _grads(rng))
    opt.step()
    _set_grads(params, _grads(rng, skip=(3,)))
    pv = [p._version for p in params]
    sv = [(opt.state[p]['exp_avg']._version, opt.state[p]['exp_avg_sq']._version) for p in params]
    opt.step()
    for i, p in enumerate(params):
        st = opt.state[p]
        if i == 3:
            assert p._version == pv[i] and (st['exp_avg']._version, st['exp_avg_sq']._version) == sv[i]
        else:
            assert p._version > pv[i] and st['exp_avg']._version > sv[i][0] and st['exp_avg_sq']._version > sv[i][1]


def test_fresh_gradient_allocations_after_zero_grad():
    """zero_grad() (set_to_none), a fresh backward whose gradients live at OTHER addresses (the first ones are kept alive), a second step:
    right against the restatement -- nothing of the first step's pointers is reused."""
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(26)
    params = _params(rng)
    xs = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in SHAPES]
    opt = FusedAdamW(params, max_grad_norm=0.1, **OPT)
    held = []
    for step in range(2):
        opt.zero_grad()
        assert all(p.grad is None for p in params)
        sum(((p * x) ** 2).sum() * (step + 1.0) for p, x in zip(params, xs)).backward()
        grads = [p.grad for p in params]
        if held:
            assert not {g.data_ptr() for g in grads} & {g.data_ptr() for g in held}
        held += grads                                                                      # keeps the old allocations alive
        before = _snapshot(opt, params)
        opt.step()
        w = _check_one_step(before, opt, params, [g.clone() for g in grads], 0.1)
        assert w <= 1.0, (step, w)
