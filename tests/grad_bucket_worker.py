"""Worker of tests/test_gpu_grad_bucket.py: ONE rank of an RCCL ("nccl") process group on cuda:0.  Two k = 2 optimiser steps of the
seeded ModelNet model through harness.train_loop with the real collective (the start-up broadcast, one all_reduce of the flat bucket per
step), then, the group destroyed, the same two steps without a group: every parameter and both moments must be bit-equal."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    from regtr_amd import harness
    from tests.test_gpu_grad_bucket import _batches, _model, _state
    from tests.util import load_cfg
    cfg = load_cfg('modelnet')
    dist.init_process_group('nccl', device_id=dev)
    assert dist.get_world_size() == 1
    calls = []
    for name in ('all_reduce', 'broadcast', 'all_gather_into_tensor', 'all_gather'):
        def counted(*a, _f=getattr(dist, name), _n=name, **k):
            calls.append(_n)
            return _f(*a, **k)
        setattr(dist, name, counted)
    grouped = _model(cfg)
    out = harness.train_loop(grouped, _batches(cfg, 4), 2, accumulate=2)
    torch.cuda.synchronize()
    assert out['step'] == 2 and calls.count('all_reduce') == 2, calls           # ONE collective per optimiser step
    assert set(calls) == {'all_reduce', 'broadcast'}, set(calls)                # ... beside the start-up broadcast
    dist.barrier()
    dist.destroy_process_group()
    alone = _model(cfg)
    harness.train_loop(alone, _batches(cfg, 4), 2, accumulate=2)
    torch.cuda.synchronize()
    a, b = _state(grouped), _state(alone)
    assert list(a) == list(b) and len(a) >= 139
    for n in a:
        assert all(torch.equal(x, y) for x, y in zip(a[n], b[n])), n
    assert torch.equal(grouped.optimizer.last_grad_norm, alone.optimizer.last_grad_norm)
    print('two k = 2 steps with the RCCL all-reduce are bit-equal to two without a group', flush=True)


if __name__ == '__main__':
    main()
