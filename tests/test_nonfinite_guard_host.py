"""CPU: the host side of skip_nonfinite -- the new entry points' refusals through the C ABI (nothing launched), the invariants of the
restatement (tests/nonfinite_guard_ref.py), the config key and train.py's switch, and FusedAdamW(skip_nonfinite=True) off the GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import nonfinite_guard_ref as G
from tests.util import load_cfg

ERR_ARG = -2


def _guarded_tensor(n=8, addr=256, **kw):
    """One regtr_optim_guarded_tensor_t as bytes the library reads on the host (it dereferences no device pointer before a launch)."""
    dt = np.dtype([('p', np.uint64), ('g', np.uint64), ('m', np.uint64), ('v', np.uint64), ('n', np.int64), ('hyper', np.float64, (5,)),
                   ('step_index', np.int32)], align=True)
    assert dt.itemsize == 88
    t = np.zeros(1, dtype=dt)
    for k in 'pgmv':
        t[k] = kw.get(k, addr)
    t['n'] = n
    t['hyper'] = kw.get('hyper', (1e-3, 1e-2, 0.9, 0.999, 1e-8))
    t['step_index'] = kw.get('step_index', 0)
    return t


def test_guarded_entry_points_refuse_bad_arguments():
    from regtr_amd import _lib
    lib = _lib.lib()
    A = 4096                                  # a plausible, aligned, never dereferenced address
    assert lib.regtr_optim_guarded_chunk_tensors() == 40 < lib.regtr_optim_chunk_tensors()
    fin = lib.regtr_grad_norm_finish_guarded
    assert fin(None, 0, 0.1, None, None, A, None) == ERR_ARG                  # no norm_coef
    assert fin(None, 0, 0.1, None, A, None, None) == ERR_ARG                  # no guard
    assert fin(None, 3, 0.1, None, A, A, None) == ERR_ARG                     # partials NULL with work to do
    assert fin(None, -1, 0.1, None, A, A, None) == ERR_ARG
    assert fin(None, 0, float('nan'), None, A, A, None) == ERR_ARG
    assert fin(None, 0, 0.1, A + 2, A, A, None) == ERR_ARG                    # misaligned grad_scale
    assert fin(None, 0, 0.1, None, A, A + 1, None) == ERR_ARG                 # misaligned guard
    step = lib.regtr_adam_step_guarded
    ok = _guarded_tensor()
    assert step(None, -1, A, A, 1, None, None, A, 1, None) == ERR_ARG
    assert step(None, 1, A, A, 1, None, None, A, 1, None) == ERR_ARG             # no tensors
    assert step(ok.ctypes.data, 1, None, A, 1, None, None, A, 1, None) == ERR_ARG   # no steps
    assert step(ok.ctypes.data, 1, A, None, 1, None, None, A, 1, None) == ERR_ARG   # no step_scalars
    assert step(ok.ctypes.data, 1, A, A + 2, 1, None, None, A, 1, None) == ERR_ARG  # misaligned step_scalars
    assert step(ok.ctypes.data, 1, A, A, 1, None, None, None, 1, None) == ERR_ARG      # no guard
    assert step(ok.ctypes.data, 1, A, A, -1, None, None, A, 1, None) == ERR_ARG
    assert step(ok.ctypes.data, 1, A, A, 1, A + 2, None, A, 1, None) == ERR_ARG        # misaligned clip_coef
    for bad in (_guarded_tensor(step_index=1), _guarded_tensor(step_index=-1), _guarded_tensor(n=-1), _guarded_tensor(p=0),
                _guarded_tensor(g=0), _guarded_tensor(m=A + 2), _guarded_tensor(hyper=(1e-3, 1e-2, 0.9, 0.999, -1.0)),
                _guarded_tensor(hyper=(float('nan'), 1e-2, 0.9, 0.999, 1e-8)), _guarded_tensor(hyper=(1e-3, float('nan'), 0.9, 0.999, 1e-8)),
                _guarded_tensor(hyper=(1e-3, 1e-2, 1.0, 0.999, 1e-8)), _guarded_tensor(hyper=(1e-3, 1e-2, 0.9, -0.1, 1e-8)),
                _guarded_tensor(hyper=(1e-3, 1e-2, 0.9, 0.999, float('nan')))):
        assert step(bad.ctypes.data, 1, A, A, 1, None, None, A, 1, None) == ERR_ARG
    assert step(None, 0, None, None, 0, None, None, None, 1, None) == 0             # nothing to do: nothing launched, no pointer looked at
    bias = lib.regtr_adam_bias_scalars
    assert bias(1e-3, 0.9, 0.999, None, 1, A, None) == ERR_ARG and bias(1e-3, 0.9, 0.999, A, -1, A, None) == ERR_ARG
    assert bias(1e-3, 0.9, 0.999, A, 1, A + 2, None) == ERR_ARG and bias(1e-3, 0.9, 0.999, None, 0, None, None) == 0
    pack = lib.regtr_grad_pack_guarded
    bt = np.zeros(1, dtype=np.dtype([('g', np.uint64), ('n', np.int64), ('offset', np.int64)], align=True))
    bt['g'], bt['n'], bt['offset'] = A, 8, 0
    assert pack(bt.ctypes.data, 1, A, 8, 1.0, 0, None, None, None) == ERR_ARG       # no flag
    assert pack(bt.ctypes.data, 1, A, 8, 1.0, 0, A + 2, None, None) == ERR_ARG      # misaligned flag
    assert pack(bt.ctypes.data, 1, A, 8, 1.0, 0, A, A + 1, None) == ERR_ARG         # misaligned n_good
    assert pack(bt.ctypes.data, 1, None, 8, 1.0, 0, A, None, None) == ERR_ARG       # what regtr_grad_pack refuses: no bucket,
    assert pack(bt.ctypes.data, 1, A, 4, 1.0, 0, A, None, None) == ERR_ARG          # a segment outside it,
    assert pack(bt.ctypes.data, 1, A, 8, float('nan'), 0, A, None, None) == ERR_ARG # a NaN scale,
    assert pack(None, -1, A, 8, 1.0, 0, A, None, None) == ERR_ARG and pack(None, 1, A, 8, 1.0, 0, A, None, None) == ERR_ARG
    bt['offset'] = 2
    assert pack(bt.ctypes.data, 1, A, 16, 1.0, 0, A, None, None) == ERR_ARG         # an offset that is no multiple of 4
    assert ctypes.sizeof(ctypes.c_int) == 4


def test_binary_exponentiation_is_within_4_ulp_of_pow():
    rng = np.random.default_rng(3)
    ts = sorted(set([0, 1, 2, 3, 4, 5, 7, 8, 1000, 2 ** 20, 2 ** 20 - 1] + rng.integers(1, 2 ** 20, 400).tolist()))
    worst = 0.0
    for b in (0.9, 0.999, 0.5, 0.99, 0.0, 0.8):
        for t in ts:
            got, want = G.ipow(b, t), float(np.float64(b) ** t)
            if want == 0.0 or got == 0.0:
                assert abs(got - want) <= 4 * 2.0 ** -1074 or (b == 0.0 and got == want), (b, t, got, want)
                continue
            if want < 2.0 ** -1022:           # subnormal results: absolute spacing
                assert abs(got - want) <= 4 * 2.0 ** -1074, (b, t)
                continue
            ulp = abs(got - want) / np.spacing(want)
            worst = max(worst, ulp)
            assert ulp <= 4, (b, t, got, want, ulp)
    assert G.ipow(0.9, 0) == 1.0 and G.ipow(0.9, 1) == 0.9 and G.ipow(0.9, 2) == 0.9 * 0.9
    print(f'ipow against pow, t <= 2^20: worst {worst:.2f} ulp')


def test_bias_scalars_agree_with_the_host_formula_to_float32_rounding():
    for t in (1, 2, 3, 10, 1000, 123456):
        ss, sb = G.bias_scalars(1e-3, 0.9, 0.999, t)
        want_ss, want_sb = 1e-3 / (1.0 - 0.9 ** t), np.sqrt(1.0 - 0.999 ** t)
        assert abs(float(ss) - want_ss) <= 2.0 ** -24 * want_ss * 1.001 and abs(float(sb) - want_sb) <= 2.0 ** -24 * want_sb * 1.001


def test_a_skipped_step_is_the_identity_in_the_restatement():
    rng = np.random.default_rng(4)
    shapes = [(5,), (3, 4), (1,)]
    params = [rng.standard_normal(s) for s in shapes]
    ref = G.GuardedAdamRef(params, max_grad_norm=0.1)
    good = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    assert ref.step(good) is True and ref.t == [1, 1, 1] and (ref.applied_steps, ref.skipped_steps) == (1, 0)
    before = ([p.copy() for p in ref.p], [m.copy() for m in ref.m], [v.copy() for v in ref.v], list(ref.t))
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = [g.copy() for g in good]
        bad[1][2, 3] = bad_value
        assert ref.step(bad) is False
    huge = [np.full(s, 3e38, np.float32) for s in shapes]                      # finite elements, a float32 norm that overflows
    assert all(np.isfinite(h).all() for h in huge) and ref.step(huge) is False
    assert ref.step(good, grad_scale=np.inf) is False and ref.step(good, grad_scale=np.nan) is False
    assert (ref.applied_steps, ref.skipped_steps) == (1, 6)
    after = (ref.p, ref.m, ref.v, ref.t)
    assert after[3] == before[3] and all(np.array_equal(a, b) for k in range(3) for a, b in zip(after[k], before[k]))
    # ... and an applied step with grad_scale = 1 is AdamRef's own
    plain = G.AdamRef(params, max_grad_norm=0.1)
    plain.step(good)
    assert all(np.array_equal(a, b) for a, b in zip(plain.p, ref.p))
    n32, c32, ok = G.finish(4.0, 0.1, 0.5)
    assert (float(n32), ok) == (1.0, True) and abs(float(c32) - 0.1 / (1.0 + 1e-6)) < 1e-8
    assert G.finish(0.0, 0.1)[:3] == (0.0, 1.0, True) and G.finish(np.nan, 0.1)[2] is False and G.finish(np.inf, 0.0)[2] is False


def test_skip_nonfinite_from_a_config_and_from_train_py(tmp_path):
    from regtr_amd import RegTR
    from regtr_amd.config import load_config
    from regtr_amd.optim import FusedAdamW
    import train
    assert train.parser.parse_args(['--config', 'x']).skip_nonfinite is False
    assert train.parser.parse_args(['--config', 'x', '--skip_nonfinite']).skip_nonfinite is True
    cfg = load_cfg('modelnet')
    assert cfg.get('skip_nonfinite', False) is False                           # the shipped configs leave it off
    off = RegTR(cfg)
    off.configure_optimizers()
    assert type(off.optimizer) is FusedAdamW and off.optimizer.skip_nonfinite is False
    src = open(train.ROOT + '/regtr_amd/conf/modelnet.yaml').read()
    p = tmp_path / 'guarded.yaml'
    p.write_text(src + '\nguard:\n  skip_nonfinite: true\n')
    cfg2 = load_config(str(p))
    assert cfg2.get('skip_nonfinite', False) is True
    on = RegTR(cfg2)
    on.configure_optimizers()
    assert on.optimizer.skip_nonfinite is True and on.optimizer.max_grad_norm == off.optimizer.max_grad_norm


def test_guarded_fused_adamw_constructs_on_the_cpu_and_refuses_cpu_parameters():
    from regtr_amd.grad_bucket import GradBucket
    from regtr_amd.optim import FusedAdamW
    w = torch.nn.Parameter(torch.ones(8))
    opt = FusedAdamW([w], lr=1e-3, max_grad_norm=0.1, skip_nonfinite=True)
    assert opt.skip_nonfinite and opt.grad_scale is None and opt.skipped_steps is None and opt.last_step_applied is None
    assert opt.step() is None                                                  # no gradient anywhere: nothing to do
    w.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match='GPU'):
        opt.step()
    assert torch.equal(w.detach(), torch.ones(8)) and len(opt.state) == 0
    plain = FusedAdamW([torch.nn.Parameter(torch.ones(8))], lr=1e-3)
    plain.param_groups[0]['params'][0].grad = torch.ones(8)
    with pytest.raises(RuntimeError, match='GPU'):
        plain.step()
    assert FusedAdamW([w]).skip_nonfinite is False
    b = GradBucket([w], n_extra=2, skip_nonfinite=True)
    assert b.skip_nonfinite and b.layout([5, 3], 2 + 1) == ([0, 8, 12], 15)
    with pytest.raises(RuntimeError, match='n_expected'):
        b.index, b.offsets, b.sizes, b.flat = [0], [0, 8], [8], torch.zeros(11)
        b.attach()
