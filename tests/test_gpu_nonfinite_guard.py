"""GPU: skip_nonfinite below the training loop -- the guarded finish, the guarded AdamW / Adam step and the guarded gradient bucket
(csrc/optim.hip, csrc/grad_bucket.hip; regtr_amd.optim.FusedAdamW, regtr_amd.grad_bucket.GradBucket) against the numpy restatement of
tests/nonfinite_guard_ref.py and the float32 one-step bound of tests/optim_ref.py.

TENSOR SETS, the smallest at which these kernels can go wrong.  MIXED: lengths 1, 3, 4, 5, 4095, 4096, 4097, an EMPTY tensor, a
6-element view that starts one float off a 16-byte boundary, and 8193 last (its n % 4 tail is element 8192) -- they straddle a 16-byte
group, the step kernel's slice (4096) and the norm kernel's (8192).  MANY(n): n tensors of 1 .. 5 elements for n = chunk, chunk + 1 and
2 chunk + 1, chunk = regtr_optim_guarded_chunk_tensors().  BAD values NaN, +inf, -inf at: the first element of the first tensor, the
n % 4 tail of the last one, inside the misaligned view, the first tensor of the second chunk; and one all-finite gradient of 3e38 whose
float32 norm overflows."""
import copy

import numpy as np
import pytest
import torch

from tests import nonfinite_guard_ref as G
from tests.test_gpu_optim import COEF_REL, OPT, _check_one_step, _dev, _f64, _grads, _params, _set_grads, _snapshot

pytestmark = pytest.mark.gpu

U = G.U
SENT = 12345.0
MIXED = [1, 3, 4, 5, 4095, 4096, 4097, 0, 6, 8193]
MISALIGNED = 8
BADS = [float('nan'), float('inf'), float('-inf')]


def _chunk():
    from regtr_amd import ops
    return ops.optim_guarded_chunk()


def _many(n):
    return [1 + i % 5 for i in range(n)]


def _placements():
    """(set name, lengths, misaligned index or None, (tensor, element) of the bad value or 'huge')."""
    ch = _chunk()
    out = [('mixed/first', MIXED, MISALIGNED, (0, 0)), ('mixed/tail', MIXED, MISALIGNED, (len(MIXED) - 1, 8192)),
           ('mixed/misaligned', MIXED, MISALIGNED, (MISALIGNED, 3)), ('mixed/huge', MIXED, MISALIGNED, 'huge')]
    for n in (ch + 1, 2 * ch + 1):
        out.append((f'many{n}/second-chunk', _many(n), None, (ch, 0)))
    return out


def _cases():
    for name, lens, mis, where in _placements():
        for bad in ([None] if where == 'huge' else BADS):
            yield name, lens, mis, where, bad


def _good_grads(rng, lens):
    return [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 1)).astype(np.float32) for n in lens]


def _spoil(grads, where, bad):
    out = [g.copy() for g in grads]
    if where == 'huge':
        return [np.full_like(g, 3e38) for g in out]                            # every element finite; the float32 norm is not
    out[where[0]][where[1]] = bad
    return out


class _Set:
    """Parameters (views inside sentinel-filled buffers, one of them misaligned) under a guarded FusedAdamW whose moments and step counts
    start from a given state, also inside sentinel-filled buffers."""

    def __init__(self, rng, lens, mis, decoupled=True, max_norm=0.1, state=True, t0=3, guarded=True):
        from regtr_amd.optim import FusedAdamW
        self.lens, self.mis = lens, mis
        self.bufs = []
        self.params = []
        for i, n in enumerate(lens):
            view, buf = self._buf(rng.standard_normal(n), i)
            self.params.append(torch.nn.Parameter(view))
            assert self.params[-1].data_ptr() == view.data_ptr()
        self.opt = FusedAdamW(self.params, max_grad_norm=max_norm, decoupled=decoupled, **OPT, **({'skip_nonfinite': True} if guarded else {}))
        if state:
            for i, (p, n) in enumerate(zip(self.params, lens)):
                m, _ = self._buf(rng.standard_normal(n) * 0.01, i)
                v, _ = self._buf(rng.standard_normal(n) ** 2 * 1e-4, i)
                self.opt.state[p] = {'step': torch.tensor(float(t0 + i % 2)), 'exp_avg': m, 'exp_avg_sq': v}

    def _buf(self, a, i):
        off = 4 + int(i == self.mis)                                           # four sentinels in front (16 bytes), one more: misaligned
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        buf = torch.full((off + a.size + 8,), SENT, dtype=torch.float32, device='cuda')
        view = buf[off:off + a.size]
        view.copy_(torch.from_numpy(a))
        assert a.size == 0 or view.data_ptr() % 16 == (4 if i == self.mis else 0)
        self.bufs.append((buf, off, a.size))
        return view, buf

    def set_grads(self, host):
        for i, (p, g) in enumerate(zip(self.params, host)):
            if g is None:
                p.grad = None
                continue
            t = torch.from_numpy(np.ascontiguousarray(g, np.float32)).cuda()
            if i == self.mis:                                                  # the gradient too starts 4 bytes off
                buf = torch.empty(t.numel() + 1, device='cuda')
                buf[1:].copy_(t)
                t = buf[1:]
            p.grad = t

    def bits(self):
        """int32 views of every buffer (margins included) and of the step counts -- cloned."""
        out = [b.view(torch.int32).clone() for b, _, _ in self.bufs]
        if self.opt._steps is not None:
            out.append(self.opt._steps.view(torch.int32).clone())
            out.append(self.opt._step_scalars.view(torch.int32).clone())       # (the kernels' workspace: not written either)
        return out

    def margins_intact(self):
        return all(bool((b[:o] == SENT).all()) and bool((b[o + n:] == SENT).all()) for b, o, n in self.bufs)

    def state(self):
        return [(p.detach().clone(), self.opt.state[p]['exp_avg'].clone(), self.opt.state[p]['exp_avg_sq'].clone(),
                 self.opt.state[p]['step'].clone()) for p in self.params if p in self.opt.state]


# ---------------------------------------------------------------------------------------------------------------- 1: the guarded finish
def test_guarded_finish_against_numpy():
    from regtr_amd import ops
    rng = np.random.default_rng(41)
    dev = 'cuda'
    cases = {'finite': rng.random(700) * 3.0, 'nan': np.array([1.0, np.nan, 2.0]), '+inf': np.array([np.inf, 1.0]),
             'overflow': np.full(8, 9e76), 'zero-partials': np.zeros(0), 'zeros': np.zeros(5), 'one': np.array([4.0])}
    guard = ops.new_guard(dev)
    applied = skipped = 0
    for name, parts in cases.items():
        partials = torch.from_numpy(parts.astype(np.float64)).to(dev)
        # the kernel's own summation order differs from numpy's by float64 rounding only: compare through the float32 norm it rounds to
        for max_norm in (0.1, 0.0, 1e9):
            for gs in (None, 1.0, 0.5, float('inf'), float('nan')):
                scale = None if gs is None else torch.tensor([gs], dtype=torch.float32, device=dev)
                out = ops.grad_norm_finish_guarded(partials, max_norm, guard, scale).cpu().numpy()
                plain = ops.grad_norm_finish(partials, max_norm).cpu().numpy()
                norm, coef, ok = G.finish(float(np.sum(parts)) if name != 'finite' else float(plain[0].astype(np.float64) ** 2), max_norm, gs)
                if name == 'finite':                                           # (the unscaled float32 norm: the unguarded kernel's, bit for bit)
                    assert abs(float(plain[0]) - np.sqrt(parts.sum())) <= U * np.sqrt(parts.sum()) * (1 + 2.0 ** -20)
                    norm = plain[0] * np.float32(1.0 if gs is None else gs)
                    with np.errstate(invalid='ignore', over='ignore'):
                        c = np.float32(max_norm) / (norm + np.float32(1e-6)) if max_norm > 0 else np.float32(1.0)
                        coef = np.float32(1.0) if c > 1.0 else c
                    ok = bool(np.isfinite(norm) and np.isfinite(np.float32(1.0 if gs is None else gs)))
                applied, skipped = applied + ok, skipped + (not ok)
                assert guard.cpu().tolist() == [int(ok), applied, skipped, 0], (name, max_norm, gs)
                assert np.array_equal(out, np.array([norm, coef], np.float32), equal_nan=True), (name, max_norm, gs, out, norm, coef)
                if gs in (None, 1.0):                                          # regtr_grad_norm_finish's bits (a NaN: a NaN)
                    assert all(a == b or (x != x and y != y) for a, b, x, y in zip(out.view(np.int32), plain.view(np.int32), out, plain))
                if gs == 0.5 and np.isfinite(plain[0]):
                    assert out[0] == plain[0] * np.float32(0.5)                # exactly halved
                expect_ok = name in ('finite', 'zero-partials', 'zeros', 'one') and gs in (None, 1.0, 0.5)
                assert ok == expect_ok, (name, gs)
    assert applied > 0 and skipped > 0


# ---------------------------------------------------------------------------------------------------------------- 2: a skipped step writes nothing
@pytest.mark.parametrize('decoupled', [True, False])
def test_a_skipped_step_writes_nothing(decoupled):
    rng = np.random.default_rng(42)
    n_cases = 0
    for name, lens, mis, where, bad in _cases():
        s = _Set(rng, lens, mis, decoupled=decoupled)
        s.set_grads(_good_grads(rng, lens))
        s.opt.step()                                                           # binds the counts to the device vector; applied
        assert int(s.opt.last_step_applied) == 1 and int(s.opt.skipped_steps) == 0
        before = s.bits()
        versions = [p._version for p in s.params]
        s.set_grads(_spoil(_good_grads(rng, lens), where, bad))
        s.opt.step()
        after = s.bits()
        assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), (name, bad)
        assert s.margins_intact(), (name, bad)
        assert int(s.opt.skipped_steps) == 1 and int(s.opt.last_step_applied) == 0, (name, bad)
        assert not torch.isfinite(s.opt.last_grad_norm), (name, bad)
        assert all(p._version > v for p, v in zip(s.params, versions))         # the versions advance without a host decision
        n_cases += 1
    assert n_cases == 3 * 5 + 1


def test_a_skipped_step_leaves_the_step_vector_and_its_margins_alone():
    """The same through ops.clip_adam_step_guarded, where the test owns the step-count vector and the guard word."""
    from regtr_amd import ops
    rng = np.random.default_rng(43)
    ch = _chunk()
    lens = _many(ch + 1)
    host = [[rng.standard_normal(n).astype(np.float32) for _ in range(4)] for n in lens]
    for h in host:
        h[3] = np.abs(h[3])
    dev = [[_dev(x, guard=8) for x in st] for st in host]
    steps, sbuf = _dev(np.arange(1, len(lens) + 3, dtype=np.float32), offset=4, guard=8)      # two more entries than tensors
    scal, cbuf = _dev(np.full(2 * (len(lens) + 2), -7.0, np.float32), offset=4, guard=8)       # the per-tensor scalars' workspace
    index = list(range(1, len(lens) + 1))
    hyp = [(1e-3, 1e-2, 0.9, 0.999, 1e-8)] * len(lens)
    guard = ops.new_guard('cuda')
    args = lambda: ([d[0][0] for d in dev], [d[1][0] for d in dev], [d[2][0] for d in dev], [d[3][0] for d in dev], hyp, index, steps, guard)
    dev[ch][1][0][0] = float('inf')                                            # the first tensor of the second chunk
    before = [d[k][1].view(torch.int32).clone() for d in dev for k in range(4)] + [sbuf.view(torch.int32).clone(), cbuf.view(torch.int32).clone()]
    ops.clip_adam_step_guarded(*args(), 0.1, step_scalars=scal)
    after = [d[k][1].view(torch.int32) for d in dev for k in range(4)] + [sbuf.view(torch.int32), cbuf.view(torch.int32)]
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and guard.cpu().tolist() == [0, 0, 1, 0]
    dev[ch][1][0][0] = 0.25                                                    # finite again: applied, every participating count + 1, no other
    ops.clip_adam_step_guarded(*args(), 0.1, step_scalars=scal)
    assert guard.cpu().tolist() == [1, 1, 1, 0]
    want = np.arange(1, len(lens) + 3, dtype=np.float32)
    want[1:len(lens) + 1] += 1
    assert steps.cpu().numpy().tolist() == want.tolist()
    assert bool((sbuf[:4] == SENT).all()) and bool((sbuf[4 + steps.numel():] == SENT).all())
    assert bool((cbuf[:4] == SENT).all()) and bool((cbuf[4 + scal.numel():] == SENT).all())
    want_scal = np.full((len(lens) + 2, 2), -7.0, np.float32)                  # the participating tensors' two scalars, bit for bit
    want_scal[1:len(lens) + 1] = [G.bias_scalars(1e-3, 0.9, 0.999, int(t)) for t in want[1:len(lens) + 1]]
    assert scal.cpu().numpy().view(np.int32).tolist() == want_scal.reshape(-1).view(np.int32).tolist()
    assert all(bool((d[k][1][lens[i]:] == SENT).all()) for i, d in enumerate(dev) for k in range(4))
    assert not torch.equal(dev[0][0][1].view(torch.int32), before[0])          # ... and it did step


# ---------------------------------------------------------------------------------------------------------------- 3: an applied step is right
def _check_set_step(s, before, host_grads, max_norm, decoupled, grad_scale=None):
    """Every tensor of the set against one float64 step of the restatement from its own float32 state; -> worst err / bound."""
    hp = dict(lr=OPT['lr'], wd=OPT['weight_decay'], b1=OPT['betas'][0], b2=OPT['betas'][1], eps=OPT['eps'])
    gs = 1.0 if grad_scale is None else float(np.float32(grad_scale))
    scaled = [None if g is None else np.asarray(g, np.float64) * gs for g in host_grads]
    coef = G.clip_coef(G.total_norm(scaled), max_norm)
    worst = 0.0
    for (p0, m0, v0, t0), p, g in zip(before, s.params, scaled):
        st = s.opt.state[p]
        t1 = int(st['step'])
        if g is None:
            assert t1 == t0 and np.array_equal(_f64(p), p0)
            continue
        assert t1 == t0 + 1 and st['step'].is_cuda and st['step'].dtype is torch.float32 and st['step'].dim() == 0
        if p.numel() == 0:
            continue
        want = G.adam_update(p0, g, m0, v0, coef, t=t1, decoupled=decoupled, **hp)
        bound = G.step_bound(p0, g, m0, v0, coef, t=t1, decoupled=decoupled, coef_rel=COEF_REL + (U if grad_scale is not None else 0.0), **hp)
        got = (_f64(p), _f64(st['exp_avg']), _f64(st['exp_avg_sq']))
        worst = max(worst, max(float(np.max(np.abs(a - w) / b)) for a, w, b in zip(got, want, bound)))
    return worst


def _before(s):
    return [(_f64(p), _f64(s.opt.state[p]['exp_avg']), _f64(s.opt.state[p]['exp_avg_sq']), int(s.opt.state[p]['step'])) for p in s.params]


@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('decoupled', [True, False])
def test_an_applied_step_is_within_the_bound(decoupled, clip):
    rng = np.random.default_rng(44 + 2 * decoupled + clip)
    max_norm = 0.1 if clip else 0.0
    ch = _chunk()
    worst = 0.0
    for lens, mis in ((MIXED, MISALIGNED), (_many(ch), None), (_many(2 * ch + 1), None)):
        s = _Set(rng, lens, mis, decoupled=decoupled, max_norm=max_norm)       # per-tensor counts that differ: 3, 4, 3, ...
        for step in range(2):
            host = _good_grads(rng, lens)
            if step == 1:
                host[1] = None                                                 # one tensor without a gradient in step 2
            before = _before(s)
            s.set_grads(host)
            s.opt.step()
            assert int(s.opt.last_step_applied) == 1 and int(s.opt.skipped_steps) == 0
            w = _check_set_step(s, before, host, max_norm, decoupled)
            assert w <= 1.0, (len(lens), step, w)
            worst = max(worst, w)
            assert s.margins_intact()
            if clip:
                assert float(s.opt.last_clip_coef) < 1.0
        counts = [int(s.opt.state[p]['step']) for p in s.params]
        assert counts == [3 + i % 2 + (2 if i != 1 else 1) for i in range(len(lens))]
    print(f'guarded step decoupled = {decoupled} clip = {clip}: worst err / bound = {worst:.3f}')


def test_fresh_state_and_the_step_2_gap_as_test_gpu_optim_arranges():
    """Four steps from no state, tensor 1 without a gradient on step 2 (tests/test_gpu_optim.py's arrangement), AdamW and Adam."""
    from regtr_amd.optim import FusedAdamW
    for decoupled in (True, False):
        rng = np.random.default_rng(21)
        mine = _params(rng)
        fused = FusedAdamW(mine, max_grad_norm=0.1, decoupled=decoupled, skip_nonfinite=True, **OPT)
        for step in range(1, 5):
            grads = _grads(rng, skip=(1,) if step == 2 else ())
            _set_grads(mine, grads)
            before = _snapshot(fused, mine)
            fused.step()
            assert _check_one_step(before, fused, mine, grads, 0.1, decoupled) <= 1.0
        assert [int(fused.state[p]['step']) for p in mine] == [4, 3, 4, 4, 4, 4]
        assert all(fused.state[p]['step'].is_cuda for p in mine) and int(fused.skipped_steps) == 0


def test_bias_correction_scalars_equal_the_restatement_bit_for_bit():
    from regtr_amd import ops
    ts = [1, 2, 3, 4, 5, 7, 8, 100, 1000, 4095, 65537, 2 ** 20, 2 ** 24 - 1]
    steps = torch.tensor(ts, dtype=torch.float32, device='cuda')
    for lr, b1, b2 in ((1e-3, 0.9, 0.999), (1e-4, 0.9, 0.999), (3e-4, 0.8, 0.99), (1e-3, 0.0, 0.5)):
        got = ops.adam_bias_scalars(lr, b1, b2, steps).cpu().numpy()
        want = np.array([G.bias_scalars(lr, b1, b2, t) for t in ts], dtype=np.float32)
        assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), (lr, b1, b2)


# ---------------------------------------------------------------------------------------------------------------- 4: no trace
def test_a_skipped_step_leaves_no_trace():
    rng = np.random.default_rng(45)
    for name, lens, mis, where, bad in _cases():
        seed = int(rng.integers(1 << 30))
        g1, g2 = _good_grads(np.random.default_rng(seed), lens), _good_grads(np.random.default_rng(seed + 1), lens)
        spoiled = _spoil(_good_grads(np.random.default_rng(seed + 2), lens), where, bad)
        runs = []
        for seq in ([g1, spoiled, g2], [g1, g2]):
            s = _Set(np.random.default_rng(seed + 3), lens, mis, state=False)
            for g in seq:
                s.set_grads(g)
                s.opt.step()
            runs.append((s.state(), int(s.opt.skipped_steps), s))
        (a, skipped_a, _), (b, skipped_b, _) = runs
        assert (skipped_a, skipped_b) == (1, 0), (name, bad)
        assert len(a) == len(b) == len(lens)
        for x, y in zip(a, b):
            assert all(torch.equal(u, v) for u, v in zip(x, y)), (name, bad)
        assert all(float(x[3]) == 2.0 for x in a)


# ---------------------------------------------------------------------------------------------------------------- 5: guard on against off
def test_guard_on_against_off_three_finite_steps():
    """Both inside the bound at every step.  Whether they are bit-equal is a MEASUREMENT (printed; tools/nonfinite_guard_bench.py
    records it): the device forms beta^t where the host calls pow."""
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(46)
    a = _params(rng)
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    on, off = FusedAdamW(a, max_grad_norm=0.1, skip_nonfinite=True, **OPT), FusedAdamW(b, max_grad_norm=0.1, **OPT)
    for _ in range(3):
        grads = _grads(rng)
        _set_grads(a, grads); _set_grads(b, grads)
        ba, bb = _snapshot(on, a), _snapshot(off, b)
        on.step(); off.step()
        assert _check_one_step(ba, on, a, grads, 0.1) <= 1.0 and _check_one_step(bb, off, b, grads, 0.1) <= 1.0
        assert torch.equal(on.last_grad_norm, off.last_grad_norm) and torch.equal(on.last_clip_coef, off.last_clip_coef)
    ulps = [float(((x.detach().view(torch.int32) - y.detach().view(torch.int32)).abs()).max()) for x, y in zip(a, b)]
    print(f'guard on against off after three steps: bit-equal = {max(ulps) == 0}, largest difference {max(ulps):.0f} ulp')


# ---------------------------------------------------------------------------------------------------------------- 6: state round trips
def test_state_round_trips():
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(47)
    mine = _params(rng)
    plain_p = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    guarded = FusedAdamW(mine, max_grad_norm=0.1, skip_nonfinite=True, **OPT)
    plain = FusedAdamW(plain_p, max_grad_norm=0.1, **OPT)                      # the unguarded optimiser over the same two steps
    for step in range(2):
        grads = _grads(rng, skip=(1,) if step == 1 else ())
        _set_grads(mine, grads); _set_grads(plain_p, grads)
        guarded.step(); plain.step()
    sd = guarded.state_dict()
    assert all(v['step'].is_cuda and v['step'].dim() == 0 and v['step'].dtype is torch.float32 for v in sd['state'].values())
    assert all(not plain.state[p]['step'].is_cuda for p in plain_p)
    # guarded -> torch.optim.AdamW -> guarded
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    ta = torch.optim.AdamW(theirs, **OPT)
    ta.load_state_dict(copy.deepcopy(sd))
    assert [float(ta.state[p]['step']) for p in theirs] == [2.0, 1.0, 2.0, 2.0, 2.0, 2.0]
    assert all(torch.equal(ta.state[b]['exp_avg'], guarded.state[a]['exp_avg']) for a, b in zip(mine, theirs))
    again = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    back = FusedAdamW(again, max_grad_norm=0.1, skip_nonfinite=True, **OPT)
    back.load_state_dict(copy.deepcopy(ta.state_dict()))
    # an unguarded FusedAdamW's state (CPU counts) -> guarded; and the same with integer counts, as an old checkpoint holds them
    from_plain_p = [torch.nn.Parameter(p.detach().clone()) for p in plain_p]
    from_plain = FusedAdamW(from_plain_p, max_grad_norm=0.1, skip_nonfinite=True, **OPT)
    from_plain.load_state_dict(copy.deepcopy(plain.state_dict()))
    ints_p = [torch.nn.Parameter(p.detach().clone()) for p in plain_p]
    ints = FusedAdamW(ints_p, max_grad_norm=0.1, skip_nonfinite=True, **OPT)
    sd_int = copy.deepcopy(plain.state_dict())
    for v in sd_int['state'].values():
        v['step'] = int(v['step'])
    ints.load_state_dict(sd_int)
    grads = _grads(rng)
    for opt, ps in ((ta, theirs), (back, again), (from_plain, from_plain_p), (ints, ints_p), (guarded, mine)):
        _set_grads(ps, grads)
        before = _snapshot(opt, ps)
        assert [b[3] for b in before] == [2, 1, 2, 2, 2, 2]
        if opt is ta:
            torch.nn.utils.clip_grad_norm_(ps, max_norm=0.1)
        opt.step()
        w = _check_one_step(before, opt, ps, grads, 0.1)
        assert w <= 1.0, (type(opt).__name__, w)
        assert [int(opt.state[p]['step']) for p in ps] == [3, 2, 3, 3, 3, 3]
    for opt, ps in ((back, again), (from_plain, from_plain_p), (ints, ints_p)):
        assert all(opt.state[p]['step'].is_cuda and opt.state[p]['step'].dtype is torch.float32 for p in ps) and int(opt.skipped_steps) == 0
    assert all(torch.equal(x, y) for x, y in zip(again, mine))                 # the same kernels from the same state: the same bits
    assert all(torch.equal(x, y) for x, y in zip(ints_p, from_plain_p))


# ---------------------------------------------------------------------------------------------------------------- 7: the guarded bucket
BUCKET_SHAPES = [(5,), (4097,), (3, 4), (1,), (8193,)]


def _bucket_params(rng):
    return [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()) for s in BUCKET_SHAPES]


def _micro(rng, bad=None):
    gs = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda() for s in BUCKET_SHAPES]
    if bad is not None:
        gs[4].view(-1)[8192] = bad                                             # the n % 4 tail of the last tensor
    return gs


def _feed(bucket, params, micros, scale, extras):
    for gs, ex in zip(micros, extras):
        for p, g in zip(params, gs):
            p.grad = g
        bucket.add(scale, ex)


def _padding(bucket):
    mask = torch.ones_like(bucket.flat, dtype=torch.bool)
    for o, n in zip(bucket.offsets, bucket.sizes):
        mask[o:o + n] = False
    mask[bucket.offsets[-1]:] = False
    return bucket.flat[mask]


@pytest.mark.parametrize('bad', BADS + ['huge'])
@pytest.mark.parametrize('pos', [0, 1, 2])
def test_guarded_bucket_excludes_a_bad_micro_batch(pos, bad):
    from regtr_amd.grad_bucket import GradBucket
    rng = np.random.default_rng(48)
    params = _bucket_params(rng)
    micros = [_micro(rng) for _ in range(3)]
    if bad == 'huge':
        micros[pos] = [torch.full_like(g, 3e38) for g in micros[pos]]
    else:
        micros[pos][4].view(-1)[8192] = bad
    extras = [torch.tensor([1.0 + i, 10.0 * (i + 1)], device='cuda') for i in range(3)]
    scale = 1.0 / 3.0
    guarded = GradBucket(params, n_extra=2, skip_nonfinite=True)
    _feed(guarded, params, micros, scale, extras)
    plain = GradBucket(params, n_extra=2)
    good = [i for i in range(3) if i != pos]
    _feed(plain, params, [micros[i] for i in good], scale, [extras[i] for i in good])
    for a, b in zip(guarded.views(), plain.views()):
        assert torch.equal(a, b)
    assert torch.equal(guarded.extra(), plain.extra())                         # the excluded micro-batch's row is absent from the tail
    assert float(guarded.n_good()) == 2.0
    assert guarded.flat.numel() == plain.flat.numel() + 1
    assert bool((_padding(guarded) == 0).all()) and _padding(guarded).numel() > 0
    scale_t = guarded.attach(3)
    assert float(scale_t) == 1.5 and float(guarded.skipped_micro_batches) == 1.0


def test_guarded_bucket_with_every_micro_batch_bad_skips_the_step():
    from regtr_amd.grad_bucket import GradBucket
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(49)
    params = _bucket_params(rng)
    opt = FusedAdamW(params, max_grad_norm=0.1, skip_nonfinite=True, **OPT)
    bucket = GradBucket(params, n_extra=2, skip_nonfinite=True)
    # a first, good step so that there is state to leave alone
    _feed(bucket, params, [_micro(rng) for _ in range(3)], 1.0 / 3.0, [torch.ones(2, device='cuda')] * 3)
    assert float(bucket.n_good()) == 3.0
    assert float(bucket.attach(3, opt)) == 1.0 and opt.grad_scale is not None
    opt.step()
    assert int(opt.last_step_applied) == 1
    before = [t.view(torch.int32).clone() for p in params for t in (p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'], opt._steps)]
    _feed(bucket, params, [_micro(rng, b) for b in BADS], 1.0 / 3.0, [torch.ones(2, device='cuda')] * 3)
    assert float(bucket.n_good()) == 0.0 and bool((bucket.flat == 0).all())    # segments, tail and padding: all zero
    bucket.attach(3, opt)
    assert torch.isinf(opt.grad_scale).all()
    opt.step()
    after = [t.view(torch.int32) for p in params for t in (p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'], opt._steps)]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert int(opt.skipped_steps) == 1 and int(opt.last_step_applied) == 0 and float(bucket.skipped_micro_batches) == 3.0


def test_a_nan_extra_with_finite_gradients_does_not_exclude_the_micro_batch():
    from regtr_amd.grad_bucket import GradBucket
    rng = np.random.default_rng(50)
    params = _bucket_params(rng)
    bucket = GradBucket(params, n_extra=2, skip_nonfinite=True)
    micros = [_micro(rng) for _ in range(2)]
    _feed(bucket, params, micros, 0.5, [torch.tensor([float('nan'), 1.0], device='cuda'), torch.tensor([2.0, 3.0], device='cuda')])
    assert float(bucket.n_good()) == 2.0 and torch.isnan(bucket.extra()[0]) and float(bucket.extra()[1]) == 2.0
    assert torch.equal(bucket.views()[1], torch.addcmul(0.5 * micros[0][1], micros[1][1], torch.tensor(0.5, device='cuda')))


# ---------------------------------------------------------------------------------------------------------------- 8: emulated ranks
def test_two_emulated_ranks_with_one_bad_micro_batch():
    """Two guarded buckets (two ranks, K = 2 each), their sum the all-reduce's result; one of the four micro-batches is bad.  The step
    after attach(4) against the float64 step on the float64 MEAN of the three good ones, within tests/optim_ref.py's bound with the
    error of the gradient the kernel sees entered ELEMENT BY ELEMENT through coef_rel.  Element i of the summed bucket is
    fl(g0 / 4 + fl(g2 / 4 + g3 / 4)) (the quarters are exact): two roundings, each at most u A_i with A_i = (|g0| + |g2| + |g3|) / 4,
    so it is 2 u A_i / |S_i| off the exact sum S_i in relative terms -- 2 u without cancellation between the micro-batches, more
    where they cancel.  grad_scale = fl(4 / 3) and the product g grad_scale add 2 u.  The norm of the bucket is within 2 u ||A|| <= 3 u
    ||S|| of the exact one for these gradients, times grad_scale (2 u more), and the float32 coefficient formed from it adds the 6 u
    of tests/test_gpu_optim.py's COEF_REL: 12 u for the coefficient with room.  coef_rel_i = 2 u A_i / |S_i| + 14 u."""
    from regtr_amd.grad_bucket import GradBucket
    from regtr_amd.optim import FusedAdamW
    rng = np.random.default_rng(51)
    params = _bucket_params(rng)
    opt = FusedAdamW(params, max_grad_norm=0.1, skip_nonfinite=True, **OPT)
    micros = [_micro(rng), _micro(rng, float('nan')), _micro(rng), _micro(rng)]
    ranks = [GradBucket(params, n_extra=1, skip_nonfinite=True) for _ in range(2)]
    for r, b in enumerate(ranks):
        _feed(b, params, micros[2 * r:2 * r + 2], 0.25, [torch.ones(1, device='cuda')] * 2)
    assert [float(b.n_good()) for b in ranks] == [1.0, 2.0]
    ranks[0].flat += ranks[1].flat                                             # the all-reduce (SUM) as arithmetic
    assert float(ranks[0].n_good()) == 3.0 and float(ranks[0].extra()) == 0.75
    p0 = [_f64(p) for p in params]
    ranks[0].attach(4, opt)
    assert float(opt.grad_scale) == float(np.float32(4.0) / np.float32(3.0))
    opt.step()
    assert int(opt.last_step_applied) == 1
    mean = [sum(_f64(micros[i][k]) for i in (0, 2, 3)) / 3.0 for k in range(len(params))]
    norm = G.total_norm(mean)
    coef = G.clip_coef(norm, 0.1)
    assert abs(float(opt.last_grad_norm) - norm) <= 8 * U * norm
    hp = dict(lr=OPT['lr'], wd=OPT['weight_decay'], b1=OPT['betas'][0], b2=OPT['betas'][1], eps=OPT['eps'])
    worst = 0.0
    for k, (p, q0, g) in enumerate(zip(params, p0, mean)):
        z = np.zeros(g.shape)
        want = G.adam_update(q0, g, z, z, coef, t=1, **hp)
        A = sum(np.abs(_f64(micros[i][k])) for i in (0, 2, 3)) / 4.0
        S = np.abs(g) * 0.75
        rel = 2 * U * A / np.where(S > 0, S, 1.0) + 14 * U
        bound = G.step_bound(q0, g, z, z, coef, t=1, coef_rel=rel, **hp)
        got = (_f64(p), _f64(opt.state[p]['exp_avg']), _f64(opt.state[p]['exp_avg_sq']))
        worst = max(worst, max(float(np.max(np.abs(a - w) / b)) for a, w, b in zip(got, want, bound)))
    print('worst error / bound of the step on the mean of the good micro-batches:', worst)
    assert worst <= 1.0


def test_nothing_bad_gives_scale_one_and_the_unguarded_bucket():
    from regtr_amd.grad_bucket import GradBucket
    rng = np.random.default_rng(52)
    params = _bucket_params(rng)
    micros = [_micro(rng) for _ in range(3)]
    extras = [torch.tensor([float(i)], device='cuda') for i in range(3)]
    on, off = GradBucket(params, n_extra=1, skip_nonfinite=True), GradBucket(params, n_extra=1)
    _feed(on, params, micros, 1.0 / 3.0, extras)
    _feed(off, params, micros, 1.0 / 3.0, extras)
    n = off.flat.numel()
    assert torch.equal(on.flat[:n], off.flat) and float(on.n_good()) == 3.0
    assert float(on.attach(3)) == 1.0 and float(on.skipped_micro_batches) == 0.0
