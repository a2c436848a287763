"""CPU: the gradient bucket's host side -- the C ABI of regtr_grad_pack (exports, every refusal, nothing launched), GradBucket's layout,
the batch sequence of accumulated / data-parallel training (harness.rank_batch_indices and the two generators' use of it), and on gloo
with two ranks the one-collective helper and the sharded validation."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.util import ROOT

ERR_ARG = -2


class _BT(ctypes.Structure):
    _fields_ = [('g', ctypes.c_void_p), ('n', ctypes.c_longlong), ('offset', ctypes.c_longlong)]


def _table(rows):
    t = (_BT * max(len(rows), 1))()
    for i, (g, n, o) in enumerate(rows):
        t[i].g, t[i].n, t[i].offset = g, n, o
    return t


def test_exports_and_header():
    from regtr_amd import _lib
    lib = _lib.lib()
    txt = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    for name in ('regtr_grad_pack_slice', 'regtr_grad_pack'):
        assert name + '(' in txt and hasattr(lib, name) and name in _lib.SIGNATURES
    assert 'regtr_bucket_tensor_t' in txt and '#define REGTR_ABI_VERSION 11' in txt and _lib.ABI_VERSION == 11
    sl = lib.regtr_grad_pack_slice()
    assert sl > 0 and sl % 1024 == 0                    # whole 16-byte groups for every lane of a 256-thread workgroup
    assert ctypes.sizeof(_BT) == 24
    from regtr_amd import build
    assert 'grad_bucket.hip' in build.SOURCES and build.EXTRA['grad_bucket.hip'] == ['-ffp-contract=off']


def test_every_refusal_returns_err_arg_without_a_launch():
    """No GPU here: a call that got as far as a launch would return the launch error (-1), not -2.  Pointers are made-up addresses with
    the alignment under test; a refused call never looks behind them."""
    from regtr_amd import _lib
    lib = _lib.lib()
    B, G = 0x7f0000001000, 0x7f0000100000               # 16-byte aligned
    def pack(rows, n, bucket=B, n_bucket=64, scale=1.0, acc=0, tab=True):
        t = _table(rows)                                # (alive across the call)
        return lib.regtr_grad_pack(ctypes.addressof(t) if tab else None, n, bucket, n_bucket, scale, acc, None)
    ok_rows = [(G, 5, 0), (G + 64, 8, 8)]
    assert pack(ok_rows, 2, bucket=None) == ERR_ARG                            # NULL bucket with work to do
    assert pack(ok_rows, 2, tab=False) == ERR_ARG                              # NULL tensors with work to do
    assert pack(ok_rows, -1) == ERR_ARG and pack(ok_rows, 2, n_bucket=-1) == ERR_ARG and pack([(G, -1, 0)], 1) == ERR_ARG      # negative counts
    assert pack([(G, 5, 2)], 1) == ERR_ARG and pack([(G, 5, 0), (G, 4, 6)], 2) == ERR_ARG      # an offset that is not a multiple of 4
    assert pack([(G, 5, 60)], 1) == ERR_ARG and pack([(G, 5, 64)], 1) == ERR_ARG and pack([(G, 5, -4)], 1) == ERR_ARG      # outside [0, n_bucket)
    assert pack([(G, 65, 0)], 1) == ERR_ARG
    assert pack([(G, 8, 8), (G, 5, 0)], 2) == ERR_ARG                          # not ascending
    assert pack([(G, 5, 0), (G, 4, 4)], 2) == ERR_ARG                          # overlapping
    assert pack([(G, 4, 0), (G, 4, 0)], 2) == ERR_ARG
    assert pack(ok_rows, 2, bucket=B + 4) == ERR_ARG and pack(ok_rows, 2, bucket=B + 8) == ERR_ARG      # bucket not 16-byte aligned
    assert pack([(G + 2, 5, 0)], 1) == ERR_ARG and pack([(G + 1, 5, 0)], 1, acc=1) == ERR_ARG            # g not 4-byte aligned
    assert pack(ok_rows, 2, scale=float('nan')) == ERR_ARG and pack(ok_rows, 2, scale=float('nan'), acc=1) == ERR_ARG
    # nothing to do is not an error and launches nothing: no tensors; empty tensors; NULL gradients under accumulate
    assert pack([], 0, tab=False) == 0 and pack([], 0, bucket=None, n_bucket=0, tab=False) == 0
    assert pack([(G, 0, 0), (None, 0, 4)], 2) == 0
    assert pack([(None, 5, 0), (None, 8, 8)], 2, acc=1) == 0


def _params(sizes, with_grad):
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
    for p, w in zip(ps, with_grad):
        p.grad = torch.ones_like(p) if w else None
    return ps


def test_layout_offsets_order_tail_and_changed_gradient_set(monkeypatch):
    from regtr_amd import grad_bucket, ops
    from regtr_amd.grad_bucket import GradBucket
    offsets, total = GradBucket.layout([5, 4, 1, 0, 7], 3)
    assert offsets == [0, 8, 12, 16, 16, 24] and total == 27
    assert GradBucket.layout([], 2) == ([0], 2)
    calls = []
    monkeypatch.setattr(ops, 'grad_pack', lambda grads, offsets, bucket, scale, accumulate, sizes=None:
                        calls.append((len(grads), list(offsets), bucket.numel(), scale, bool(accumulate), list(sizes))))
    sizes = [5, 6, 4, 9]
    ps = _params(sizes, [True, False, True, True])                  # params[1] is frozen: not in the layout
    b = GradBucket([(f'w{i}', p) for i, p in enumerate(ps)], n_extra=2)
    assert b.flat is None
    b.add(0.5, torch.zeros(2))
    assert b.index == [0, 2, 3] and b.offsets == [0, 8, 12, 24] and b.sizes == [5, 4, 9] and b.flat.numel() == 26
    assert all(o % 4 == 0 for o in b.offsets) and not b.flat.any()
    b.add(0.5)
    # the first call of a step assigns, the second accumulates; the tail is one more row after the last segment
    assert calls == [(4, [0, 8, 12, 24], 26, 0.5, False, [5, 4, 9, 2]), (4, [0, 8, 12, 24], 26, 0.5, True, [5, 4, 9, 2])]
    b.attach()
    assert [p.grad is not None for p in ps] == [True, False, True, True]
    assert all(p.grad.data_ptr() == b.flat.data_ptr() + 4 * o and p.grad.shape == p.shape for p, o in zip([ps[0], ps[2], ps[3]], b.offsets))
    assert b.extra().data_ptr() == b.flat.data_ptr() + 4 * 24 and b.extra().numel() == 2
    b.add(1.0)
    assert calls[-1][4] is False                                    # after attach() a new step begins
    b.reset()
    b.add(1.0)
    assert calls[-1][4] is False                                    # ... and after reset(), which abandons one
    ps[1].grad = torch.ones(6)                                      # a parameter that had no gradient at the first add
    with pytest.raises(RuntimeError, match='w1'):
        b.add(1.0)
    ps[1].grad, ps[2].grad = None, None
    with pytest.raises(RuntimeError, match='w2'):
        b.add(1.0)
    with pytest.raises(RuntimeError):
        GradBucket(_params([3], [False])).add(1.0)
    assert grad_bucket.all_reduce_sum(torch.ones(3)).tolist() == [1.0, 1.0, 1.0]      # no process group: nothing happens


@pytest.mark.parametrize('n,batch,epochs,k,W', [(10, 2, 3, 2, 2), (7, 2, 5, 3, 2), (4, 2, 4, 2, 1), (9, 4, 2, 1, 4), (5, 1, 1, 2, 4),
                                                (33, 4, 3, 4, 8), (6, 2, 1, 1, 1)])
def test_index_rule(n, batch, epochs, k, W):
    from regtr_amd.harness import rank_batch_indices
    per_epoch = -(-n // batch)
    total = epochs * per_epoch
    n_steps = total // (k * W)
    ranks = [rank_batch_indices(n, batch, epochs, k, r, W) for r in range(W)]
    assert len({len(x) for x in ranks}) == 1 and len(ranks[0]) == n_steps * k          # every rank yields the same count
    assert sorted(sum(ranks, [])) == list(range(n_steps * k * W))                     # a partition of the complete groups
    one = rank_batch_indices(n, batch, epochs, k * W, 0, 1)
    for s in range(n_steps):                                                          # (k, W) and (k W, 1): the same set per optimiser step
        step_set = sorted(j for x in ranks for j in x[s * k:(s + 1) * k])
        assert step_set == one[s * k * W:(s + 1) * k * W] == [s * k * W + i for i in range(k * W)]
        for r in range(W):
            assert ranks[r][s * k:(s + 1) * k] == [(s * k + m) * W + r for m in range(k)]      # j = ((s - 1) k + m) W + r, s from 1
    # first_step counts micro-batches
    f = k * W
    assert [rank_batch_indices(n, batch, epochs, k, r, W, first_step=f) for r in range(W)] == [[j for j in x if j >= f] for x in ranks]
    with pytest.raises(ValueError):
        rank_batch_indices(n, batch, epochs, k, W, W)


def test_generators_build_only_their_ranks_batches(monkeypatch):
    """modelnet_train_batches hands (seed, j) of its rank's batches alone to the augmentation, with the clouds an unsharded run gives
    batch j, and loads no other cloud."""
    from regtr_amd import augment, harness
    n, batch, epochs, k, W, seed = 7, 2, 3, 2, 2, 5

    class Source:
        def __init__(self):
            self.read = []

        def __len__(self):
            return n

        def __getitem__(self, i):
            self.read.append(i)
            return np.full((3, 3), float(i), dtype=np.float32)

    monkeypatch.setattr(augment, 'modelnet_train_batch', lambda clouds, cfg, seed_, step: {'step': step, 'seed': seed_, 'first': [float(c[0, 0]) for c in clouds]})
    run = lambda src, **kw: list(harness.modelnet_train_batches(src, None, batch, seed, epochs=epochs, device='cpu', **kw))
    full = run(Source())
    assert [b['step'] for b in full] == list(range(12)) and [len(b['ids']) for b in full][:4] == [2, 2, 2, 1]
    for r in range(W):
        src = Source()
        mine = run(src, accumulate=k, rank=r, world=W)
        want = harness.rank_batch_indices(n, batch, epochs, k, r, W)
        assert [b['step'] for b in mine] == want and len(want) == 6
        assert all(b['ids'] == full[b['step']]['ids'] and b['first'] == full[b['step']]['first'] and b['seed'] == seed for b in mine)
        assert src.read == [i for b in mine for i in b['ids']]                        # nothing else was loaded
    resumed = run(Source(), accumulate=k, rank=1, world=W, first_step=4)
    assert [b['step'] for b in resumed] == [5, 7, 9, 11]
    assert [b['step'] for b in run(Source(), first_step=3)] == list(range(3, 12))     # the defaults: today's sequence


# ---------------------------------------------------------------------------------------------------- gloo, world size 2
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


class _ValModel(torch.nn.Module):
    """Stands in for RegTR in the sharded validation: per-batch outputs that are a known function of the batch."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def validation_step(self, batch, i):
        self.seen.append(i)
        return {'total': torch.tensor(float(batch) * 0.5)}, {'err': torch.tensor([float(batch), float(batch) + 0.25])}

    def validation_epoch_end(self, outputs):
        total = torch.stack([o[0]['total'] for o in outputs])
        err = torch.cat([o[1]['err'] for o in outputs])
        score = float((err * torch.arange(1, err.numel() + 1)).sum())              # depends on the ORDER of the batches
        return score, {'losses': {'total': total.mean()}, 'n': len(outputs)}


def _gloo_worker(rank, world, port, q):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from regtr_amd import harness
    from regtr_amd.distributed import all_reduce_sum
    from regtr_amd.grad_bucket import GradBucket
    calls = []
    for name in ('all_gather', 'all_gather_into_tensor', 'all_gather_object', 'all_reduce', 'broadcast', 'gather', 'all_to_all'):
        def counted(*a, _f=getattr(dist, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        setattr(dist, name, counted)
    # a flat tensor laid out as GradBucket lays it out: segments of 5 and 6 floats, padding, a tail of 2
    offsets, total = GradBucket.layout([5, 6], 2)
    flat = torch.zeros(total)
    flat[0:5] = torch.arange(5.0) + 10.0 * rank
    flat[8:14] = -(torch.arange(6.0) + 1.0) * (rank + 1)
    flat[16:18] = torch.tensor([1.5, 2.5]) * (rank + 1)
    all_reduce_sum(flat)
    n_reduce = list(calls)
    model = _ValModel()
    score, val = harness._validate(model, lambda: iter([3.0, 1.0, 4.0, 1.5, 9.0]))
    q.put((rank, flat.numpy().copy(), n_reduce, list(calls), score, float(val['losses']['total']), val['n'], model.seen))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_one_collective_and_sharded_validation():
    from regtr_amd import harness
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    results = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    exp = np.zeros(18, dtype=np.float32)
    exp[0:5] = 2 * np.arange(5.0) + 10.0
    exp[8:14] = -3.0 * (np.arange(6.0) + 1.0)
    exp[16:18] = [4.5, 7.5]
    ref_score, ref_val = harness._validate(_ValModel(), lambda: iter([3.0, 1.0, 4.0, 1.5, 9.0]))      # no group: the plain loop
    for rank, flat, n_reduce, calls, score, total, n, seen in results:
        assert np.array_equal(flat, exp) and not flat[5:8].any() and not flat[14:16].any()            # the rank sum; padding stays zero
        assert n_reduce == ['all_reduce'] and calls == ['all_reduce', 'all_gather_object']            # ONE collective each
        assert seen == [i for i in range(5) if i % 2 == rank]                                         # batch i on rank i % W
        assert score == ref_score and total == float(ref_val['losses']['total']) and n == 5           # identical on both ranks
