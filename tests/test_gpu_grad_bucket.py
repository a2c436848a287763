"""GPU: the gradient bucket -- regtr_grad_pack against a numpy float32 restatement, GradBucket in the training loop (k = 1 identity,
k = 2 against the two gradients computed alone and against the float64 step, two emulated ranks), the real collective at world size 1,
and train.py --accumulate / --gpus.

Model set-up as tests/test_gpu_training_loop.py: seeded ModelNet weights, B = 2 raw clouds of 2048 seeded points."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests.util import ROOT, load_cfg

pytestmark = pytest.mark.gpu

_shared = {}


# ---------------------------------------------------------------------------------------------------------------- grad_pack
def _values(rng, n):
    """Mixed signs, magnitudes over 2^-20 .. 2^20: far from the subnormal range, so a power-of-two scale is exact."""
    return (rng.choice([-1.0, 1.0], n) * (1.0 + rng.random(n)) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)


def _pack_case():
    """49 tensors (one more than a chunk): the sizes around the 16-byte group and around the slice, small odd ones for the rest; tensor 5
    is a view that starts 1 float into its storage (the scalar path); a bucket with 7 floats after the tail."""
    if 'pack' not in _shared:
        from regtr_amd import ops
        from regtr_amd.grad_bucket import GradBucket
        sl = ops.grad_pack_slice()
        rng = np.random.default_rng(7)
        sizes = [0, 1, 3, 4, 5, sl - 1, sl, sl + 1] + [int(s) for s in rng.integers(1, 300, 41)]
        assert len(sizes) == 49 > ops.optim_slices()[2]
        offsets, total = GradBucket.layout(sizes, 3)
        g = [[_values(rng, n) for n in sizes] for _ in range(2)]
        none = [{2, 6, 20}, {3, 7, 48}]                                        # None gradients of the assign / the accumulate call (never the misaligned 5)
        before = _values(rng, total + 7)                                       # the segments' contents before the assign
        keep = np.zeros(total + 7, dtype=bool)
        for o, n in zip(offsets, sizes):
            keep[o:o + n] = True
        before[~keep] = 0.0                                                    # padding, tail and the rest: zero, as allocated
        _shared['pack'] = (sizes, offsets, total, g, none, before, keep)
    return _shared['pack']


def _device_grads(arrays, none, misaligned=5):
    out = []
    for i, a in enumerate(arrays):
        if i in none:
            out.append(None)
        elif i == misaligned:
            store = torch.zeros(a.size + 1, dtype=torch.float32, device='cuda')
            store[1:] = torch.from_numpy(a).cuda()
            out.append(store[1:])
            assert out[-1].data_ptr() % 16 == 4
        else:
            out.append(torch.from_numpy(a).cuda())
    return out


def _run_pack(scale):
    from regtr_amd import ops
    sizes, offsets, total, g, none, before, keep = _pack_case()
    bucket = torch.from_numpy(before).cuda()
    ops.grad_pack(_device_grads(g[0], none[0]), offsets[:-1], bucket, scale, False, sizes=sizes)
    first = bucket.cpu().numpy()
    ops.grad_pack(_device_grads(g[1], none[1]), offsets[:-1], bucket, scale, True, sizes=sizes)
    return first, bucket.cpu().numpy()


@pytest.mark.parametrize('scale', [1.0, 0.5, 0.125])
def test_grad_pack_power_of_two_scales_bit_exact(scale):
    """scale g is exact, so the assign is that number and the fused multiply-add is ONE float32 addition: numpy's float32 arithmetic
    gives the same bits."""
    sizes, offsets, total, g, none, before, keep = _pack_case()
    first, second = _run_pack(scale)
    s = np.float32(scale)
    exp1 = before.copy()
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        exp1[o:o + n] = 0.0 if i in none[0] else s * g[0][i]
    exp2 = exp1.copy()
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        if i not in none[1]:
            exp2[o:o + n] = s * g[1][i] + exp1[o:o + n]
    assert exp1.dtype == exp2.dtype == np.float32
    assert np.array_equal(first.view(np.uint32), exp1.view(np.uint32)) and np.array_equal(second.view(np.uint32), exp2.view(np.uint32))
    assert not first[~keep].any() and not second[~keep].any()                  # padding, tail and what follows it stay zero


def test_grad_pack_third_within_one_ulp():
    """scale = 1/3: within 1 ulp of float32(float64(scale32) g + b) -- the float64 product of two float32 numbers is exact, so only the
    double rounding of the sum can differ from the fused multiply-add."""
    sizes, offsets, total, g, none, before, keep = _pack_case()
    first, second = _run_pack(1.0 / 3.0)
    s = np.float64(np.float32(1.0 / 3.0))
    exp1 = before.copy()
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        exp1[o:o + n] = 0.0 if i in none[0] else (s * g[0][i].astype(np.float64)).astype(np.float32)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(first.astype(np.float64) - exp1) <= ulp(exp1))
    exp2 = first.copy()                                                        # (the accumulate starts from what the assign left)
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        if i not in none[1]:
            exp2[o:o + n] = (s * g[1][i].astype(np.float64) + first[o:o + n].astype(np.float64)).astype(np.float32)
    err = np.abs(second.astype(np.float64) - exp2)
    print('worst error in ulp:', float(np.max(err / ulp(exp2))))
    assert np.all(err <= ulp(exp2))
    assert not first[~keep].any() and not second[~keep].any()


def test_grad_pack_python_refusals():
    from regtr_amd import ops
    bucket = torch.zeros(16, device='cuda')
    g = torch.ones(4, device='cuda')
    with pytest.raises(RuntimeError):
        ops.grad_pack([torch.ones(4)], [0], bucket, 1.0, False)                # a CPU gradient
    with pytest.raises(RuntimeError):
        ops.grad_pack([g.double()], [0], bucket, 1.0, False)
    with pytest.raises(RuntimeError):
        ops.grad_pack([g], [0], torch.zeros(16), 1.0, False)                   # a CPU bucket
    with pytest.raises(RuntimeError):
        ops.grad_pack([None], [0], bucket, 1.0, False)                         # a None gradient without its length
    with pytest.raises(RuntimeError, match='invalid argument'):
        ops.grad_pack([g, g], [4, 0], bucket, 1.0, False)                      # what the library refuses
    with pytest.raises(RuntimeError, match='invalid argument'):
        ops.grad_pack([g], [0], bucket, float('nan'), False)
    assert not bucket.any()


# ---------------------------------------------------------------------------------------------------------------- the training loop
def _batches(cfg, n):
    from regtr_amd.augment import modelnet_train_batch
    from tests.test_gpu_training_loop import SEED, _points
    return [modelnet_train_batch(_points(), cfg, SEED, step) for step in range(n)]


def _model(cfg):
    from tests.test_gpu_training_loop import _fresh_model
    model = _fresh_model(cfg)
    model.configure_optimizers()
    return model


def _state(model):
    names = dict(model.named_parameters())
    st = model.optimizer.state
    return {n: (p.detach().clone(), st[p]['exp_avg'].clone(), st[p]['exp_avg_sq'].clone()) for n, p in names.items() if p in st}


def test_k1_bucket_path_is_the_plain_loop_bit_for_bit():
    """Three optimiser steps through the bucket path at k = 1 without a group -- train_loop's bucket path step by step (it takes the
    plain path itself at k = 1 without a group) -- against train_loop's plain path."""
    from regtr_amd import harness
    from regtr_amd.grad_bucket import GradBucket
    cfg = load_cfg('modelnet')
    plain, bucketed = _model(cfg), _model(cfg)
    harness.train_loop(plain, _batches(cfg, 3), 3)
    bucket = None
    for step, batch in enumerate(_batches(cfg, 3), 1):
        bucketed.optimizer.zero_grad()
        _, losses = bucketed.training_step(batch, step, train_backbone=True)
        losses['total'].backward()
        if bucket is None:
            bucket = GradBucket(list(bucketed.named_parameters()), n_extra=len(losses))
        bucket.add(1.0, torch.stack([v.detach() for v in losses.values()]))
        bucketed.optimizer.zero_grad()
        bucket.all_reduce()
        bucket.attach()
        bucketed.optimizer.step()
        bucketed.scheduler.step()
        assert torch.equal(bucket.extra(), torch.stack([v.detach() for v in losses.values()]))
    a, b = _state(plain), _state(bucketed)
    assert list(a) == list(b) and len(a) >= 139
    for n in a:
        assert all(torch.equal(x, y) for x, y in zip(a[n], b[n])), n
    assert all(torch.equal(p, q) for p, q in zip(plain.parameters(), bucketed.parameters()))
    assert torch.equal(plain.optimizer.last_grad_norm, bucketed.optimizer.last_grad_norm)
    assert all(int(s['step']) == 3 for s in bucketed.optimizer.state.values())


def _micro(model, batch):
    model.optimizer.zero_grad()
    _, losses = model.training_step(batch, 1, train_backbone=True)
    losses['total'].backward()
    return losses


def _k2():
    """Shared by the k = 2 tests, computed once: the two micro-batches' gradients computed alone, the bucket after both, the two one-
    micro-batch 'rank' buckets, and the stepped model."""
    if 'k2' not in _shared:
        from regtr_amd.grad_bucket import GradBucket
        cfg = load_cfg('modelnet')
        model = _model(cfg)
        alone, totals = [], []
        for batch in _batches(cfg, 2):
            losses = _micro(model, batch)
            alone.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
            totals.append(losses['total'].detach().clone())
        model.optimizer.zero_grad()
        ranks = []
        for batch in _batches(cfg, 2):                                         # one bucket per emulated rank: its micro-batch, scale 1 / 2
            losses = _micro(model, batch)
            rb = GradBucket(list(model.named_parameters()), n_extra=len(losses))
            rb.add(0.5, torch.stack([v.detach() for v in losses.values()]))
            ranks.append(rb.flat.clone())
        model.optimizer.zero_grad()
        bucket, keys = None, None
        for batch in _batches(cfg, 2):                                         # k = 2 on one rank
            losses = _micro(model, batch)
            if bucket is None:
                keys = list(losses)
                bucket = GradBucket(list(model.named_parameters()), n_extra=len(keys))
            bucket.add(0.5, torch.stack([losses[k].detach() for k in keys]))
        model.optimizer.zero_grad()
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        flat = bucket.flat.clone()
        bucket.all_reduce()                                                    # no group: nothing
        bucket.attach()
        model.optimizer.step()
        _shared['k2'] = dict(cfg=cfg, model=model, alone=alone, totals=totals, ranks=ranks, bucket=bucket, flat=flat, keys=keys, before=before)
    return _shared['k2']


def test_k2_bucket_is_the_float32_mean_of_the_two_gradients_computed_alone():
    s = _k2()
    bucket, (g0, g1) = s['bucket'], s['alone']
    names = [bucket.names[i] for i in bucket.index]
    assert names == list(g0) == list(g1) and len(names) >= 139
    assert torch.equal(bucket.flat, s['flat'])                                 # attach() and the step leave the bucket as it was
    for n, v in zip(names, bucket.views()):
        assert torch.equal(v, 0.5 * g0[n] + 0.5 * g1[n]), n
    t0, t1 = s['totals']
    assert torch.equal(bucket.extra()[s['keys'].index('total')], 0.5 * t0 + 0.5 * t1)      # the logged total: the mean of the two
    # the padding between the segments is still zero
    keep = torch.zeros(bucket.flat.numel(), dtype=torch.bool, device='cuda')
    for o, n in zip(bucket.offsets, bucket.sizes + [bucket.n_extra]):
        keep[o:o + n] = True
    assert not bucket.flat[~keep].any() and all(o % 4 == 0 for o in bucket.offsets)


def test_two_emulated_ranks_sum_to_the_k2_bucket():
    """(k, W) = (1, 2) against (2, 1), where it is exact: rank r packs micro-batch r with scale 1 / 2, the buckets are added in rank
    order (what the all-reduce of two ranks computes), and the sum is the k = 2 bucket bit for bit."""
    s = _k2()
    assert torch.equal(s['ranks'][0] + s['ranks'][1], s['flat'])


def test_k2_step_within_the_float64_bound_and_train_loop_takes_it():
    """One optimiser step from the k = 2 bucket against tests/optim_ref.py's float64 step on the FLOAT64 mean of the two gradients, within
    its derived one-step bound.  The bucket holds fl(g0 / 2 + g1 / 2): a relative u off the float64 mean, element by element, and the
    norm the kernels take of it is therefore a relative u off the float64 mean's -- both enter the bound as a relative error of the
    scaled gradient, i.e. through coef_rel, next to the 6 u of a float32 clip coefficient (tests/test_gpu_optim.py COEF_REL)."""
    from regtr_amd import harness
    s = _k2()
    model, opt = s['model'], s['model'].optimizer
    gr = opt.param_groups[0]
    hp = dict(lr=gr['lr'], wd=gr['weight_decay'], b1=gr['betas'][0], b2=gr['betas'][1], eps=gr['eps'])
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    mean = {n: 0.5 * f64(s['alone'][0][n]) + 0.5 * f64(s['alone'][1][n]) for n in s['alone'][0]}
    norm = R.total_norm(list(mean.values()))
    coef = R.clip_coef(norm, opt.max_grad_norm)
    assert abs(float(opt.last_grad_norm) - norm) <= 4 * R.U * norm              # last_grad_norm: the AVERAGED gradient's norm
    worst = 0.0
    params = dict(model.named_parameters())
    for n, g in mean.items():
        p0, z = f64(s['before'][n]), np.zeros(g.shape)
        st = opt.state[params[n]]
        want = R.adam_update(p0, g, z, z, coef, t=1, decoupled=opt.decoupled, **hp)
        bound = R.step_bound(p0, g, z, z, coef, t=1, decoupled=opt.decoupled, coef_rel=8 * R.U, **hp)
        got = (f64(params[n]), f64(st['exp_avg']), f64(st['exp_avg_sq']))
        worst = max(worst, max(float(np.max(np.abs(a - w) / b)) for a, w, b in zip(got, want, bound)))
    print('worst error / bound of the k = 2 step:', worst)
    assert worst <= 1.0
    # harness.train_loop(accumulate=2) is that step: the same parameters, and its averaged total is the mean of the two totals
    looped = _model(s['cfg'])
    out = harness.train_loop(looped, _batches(s['cfg'], 2), 1, accumulate=2)
    assert out['step'] == 1 and all(torch.equal(p, q) for p, q in zip(looped.parameters(), model.parameters()))
    assert torch.equal(out['loss_avg']['total'], 0.5 * s['totals'][0] + 0.5 * s['totals'][1])


# ---------------------------------------------------------------------------------------------------------------- child processes
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def test_one_rank_rccl_all_reduce_leaves_the_steps_bit_equal():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=1', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'tests', 'grad_bucket_worker.py')]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'two k = 2 steps with the RCCL all-reduce are bit-equal to two without a group' in r.stdout


def _train(tmp, name, *args, ok=True):
    """train.py as a fresh child process under its own time limit, with the arguments of tests/test_gpu_training_loop.py's resume test;
    --dev logs to ../logdev relative to the working directory."""
    cwd = os.path.join(tmp, name, 'work')
    os.makedirs(cwd, exist_ok=True)
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--config', os.path.join(ROOT, 'regtr_amd', 'conf', 'modelnet.yaml'),
           '--synthetic', '4', '--batch', '2', '--num_workers', '0', '--dev', '--validate_every', '2', *args]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=240)
    if ok:
        assert r.returncode == 0, r.stderr[-3000:]
        return os.path.join(tmp, name, 'logdev', 'ckpt')
    return r


@pytest.fixture(scope='module')
def acc2(tmp_path_factory):
    """`train.py --accumulate 2 --steps 2`, run once for the two tests below -> (the temporary root, its checkpoint folder)."""
    tmp = str(tmp_path_factory.mktemp('acc2'))
    return tmp, _train(tmp, 'part', '--accumulate', '2', '--steps', '2')


def _load(folder, step):
    return torch.load(os.path.join(folder, f'model-{step}.pth'), map_location='cpu', weights_only=False)


def test_train_py_accumulate_resume_equals_the_unbroken_run(acc2):
    tmp, part = acc2
    assert open(os.path.join(part, 'checkpoints.txt')).readline().strip() == 'Best step: 2'
    two = _load(part, 2)
    assert sorted(two) == ['accumulate', 'optimizer', 'scheduler', 'state_dict', 'step', 'world']
    assert (two['accumulate'], two['world'], two['step']) == (2, 1, 2)
    full = _train(tmp, 'full', '--accumulate', '2', '--steps', '4')
    resumed = _train(tmp, 'resumed', '--accumulate', '2', '--steps', '2', '--resume', part)
    a, b = _load(full, 4), _load(resumed, 4)
    assert sorted(a) == sorted(b) == sorted(two) and a['step'] == b['step'] == 4
    assert list(a['state_dict']) == list(b['state_dict'])
    assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])
    sa, sb = a['optimizer']['state'], b['optimizer']['state']
    assert sorted(sa) == sorted(sb) and len(sa) >= 139
    for k in sa:
        assert float(sa[k]['step']) == float(sb[k]['step']) == 4.0             # optimiser steps, not micro-batches
        assert torch.equal(sa[k]['exp_avg'], sb[k]['exp_avg']) and torch.equal(sa[k]['exp_avg_sq'], sb[k]['exp_avg_sq'])
    assert a['scheduler'] == b['scheduler'] and a['scheduler']['last_epoch'] == 4
    assert not torch.equal(two['state_dict']['feat_proj.weight'], a['state_dict']['feat_proj.weight'])
    r = _train(tmp, 'refused', '--accumulate', '1', '--steps', '2', '--resume', part, ok=False)
    assert r.returncode != 0 and '2 x 1 = 2' in r.stderr and '1 x 1 = 1' in r.stderr, r.stderr[-2000:]


def test_train_py_gpus_1_writes_the_same_checkpoint(acc2):
    tmp, part = acc2
    ranked = _train(tmp, 'gpus1', '--gpus', '1', '--accumulate', '2', '--steps', '2')
    a, b = _load(part, 2), _load(ranked, 2)
    assert sorted(a) == sorted(b) and (b['accumulate'], b['world'], b['step']) == (2, 1, 2)
    assert list(a['state_dict']) == list(b['state_dict'])
    assert all(torch.equal(a['state_dict'][k], b['state_dict'][k]) for k in a['state_dict'])
    sa, sb = a['optimizer']['state'], b['optimizer']['state']
    assert sorted(sa) == sorted(sb)
    assert all(torch.equal(sa[k]['exp_avg'], sb[k]['exp_avg']) and torch.equal(sa[k]['exp_avg_sq'], sb[k]['exp_avg_sq']) for k in sa)
