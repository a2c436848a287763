"""Times the gradient bucket (regtr_amd.grad_bucket.GradBucket, csrc/grad_bucket.hip) at the real gradient sets of the ModelNet and the
3DMatch model, on one GPU in one process, the routes of a comparison taking turns.
    python tools/grad_bucket_bench.py [--reps 15] [--inner 1000] [--step_inner 3] [--out profiles/grad_bucket_bench.txt]
Gradient sets as tools/optim_bench.py builds them (its `build`): one training_step(train_backbone=True) + backward on B = 4 synthetic
2048-point clouds / two synthetic 20000-point pairs.  Three comparisons per model:
  pack        GradBucket.add (one regtr_grad_pack per 48 tensors), assigning and accumulating, against the same arithmetic composed
              from torch.cat and mul_ / add_ (a temporary of the gradients' size and a second pass) -- per call between device events
              (host-bound: the Python side of a call takes longer than its kernels), and, apart from that, the KERNELS' summed device
              time per call (torch.profiler, a run of its own) with the bytes they must move over it;
  accumulate  ONE k = 2 optimiser step (2 x (training_step, backward, add with the stacked losses), attach, step) against TWO plain steps: what accumulation
              costs beside the two forward-backward passes it shares with them;
  plumbing    the bucket path at k = 1 under a ONE-RANK RCCL group (add, all_reduce of the flat bucket, attach, step) against the plain
              step, as a share of the plain step.
A sample is `inner` (`step_inner` for whole steps) consecutive calls between two device events -- about 0.1 s of work either way --
after warm-up calls of every route; `reps` samples per route.  Reported: median and min .. max over the samples (the spread).  No run with more than one GPU is made."""
import argparse
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def stats(samples, unit=1e3):
    s = sorted(samples)
    return {'median': round(unit * s[len(s) // 2], 1), 'min': round(unit * s[0], 1), 'max': round(unit * s[-1], 1)}


def take_turns(routes, reps, inner, warmup=3):
    from optim_bench import events_ms
    for f in routes.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    samples = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            samples[k].append(events_ms(f, inner))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=1000)
    ap.add_argument('--step_inner', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'grad_bucket_bench.txt'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/grad_bucket_bench.py needs an MI355X (HIP) device')
    import torch.distributed as dist
    from optim_bench import build, count_launches
    from regtr_amd.grad_bucket import GradBucket
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lines = []
    for name in ('modelnet', '3dmatch'):
        model, fwd_bwd = build(name, dev)
        optim = model.optimizer
        for _ in range(3):
            fwd_bwd()
        torch.cuda.synchronize()
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        n_elem = sum(g.numel() for g in grads)
        res = {'config': name, 'tensors_with_gradient': len(grads), 'elements': n_elem, 'samples': opt.reps}

        # ---- pack: GradBucket.add against torch.cat + mul_ / add_
        bucket = GradBucket(list(model.named_parameters()))
        bucket.add(0.5)
        composed = torch.zeros(n_elem, dtype=torch.float32, device=dev)

        def hip(fill):
            bucket._filled = fill
            bucket.add(0.5)

        def cat_assign():
            torch.cat([g.reshape(-1) for g in grads], out=composed)
            composed.mul_(0.5)

        def cat_accumulate():
            composed.add_(torch.cat([g.reshape(-1) for g in grads]), alpha=0.5)
        s = take_turns({'hip_assign': lambda: hip(False), 'cat_assign': cat_assign, 'hip_accumulate': lambda: hip(True),
                        'cat_accumulate': cat_accumulate}, opt.reps, opt.inner, warmup=10)
        res['pack_us'] = {k: stats(v) for k, v in s.items()}
        res['pack_calls_per_sample'] = opt.inner
        # the kernels alone: launches and summed device time of ONE call; bytes = g read + bucket written (+ bucket read to accumulate)
        kern = {}
        for k, f, passes in (('hip_assign', lambda: hip(False), 2), ('hip_accumulate', lambda: hip(True), 3), ('cat_assign', cat_assign, 4),
                             ('cat_accumulate', cat_accumulate, 5)):
            launches, us = count_launches(f)
            kern[k] = {'launches': launches, 'kernel_us': us, 'passes_over_the_gradients': passes,
                       'TB_per_s': round(4.0 * n_elem * passes / us / 1e6, 2) if us else None}
        res['pack_kernels'] = kern

        # ---- accumulate: one k = 2 step against two plain steps
        def plain_step():
            fwd_bwd()
            optim.step()

        def bucket_step(k, reduce):
            for _ in range(k):
                losses = fwd_bwd()
                step_bucket.add(1.0 / k, torch.stack([v.detach() for v in losses.values()]))
            optim.zero_grad()
            if reduce:
                step_bucket.all_reduce()
            step_bucket.attach()
            optim.step()
        step_bucket = GradBucket(list(model.named_parameters()), n_extra=len(fwd_bwd()))      # with the loss tail, as train_loop's
        s = take_turns({'two_plain_steps': lambda: (plain_step(), plain_step()), 'one_k2_step': lambda: bucket_step(2, False)},
                       opt.reps, opt.step_inner)
        res['accumulate_ms'] = {k: stats(v, 1.0) for k, v in s.items()}
        res['accumulate_ms']['k2_minus_two_plain_median'] = round(res['accumulate_ms']['one_k2_step']['median'] - res['accumulate_ms']['two_plain_steps']['median'], 3)

        # ---- plumbing: k = 1 under a one-rank RCCL group against the plain step
        if not dist.is_initialized():
            os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
            with socket.socket() as sock:          # a free port: two benches on one host must not meet
                sock.bind(('127.0.0.1', 0))
                os.environ.setdefault('MASTER_PORT', str(sock.getsockname()[1]))
            os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
            dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
        s = take_turns({'plain_step': plain_step, 'bucket_k1_one_rank_group': lambda: bucket_step(1, True)}, opt.reps, opt.step_inner)
        res['plumbing_ms'] = {k: stats(v, 1.0) for k, v in s.items()}
        d = res['plumbing_ms']['bucket_k1_one_rank_group']['median'] - res['plumbing_ms']['plain_step']['median']
        res['plumbing_ms']['difference_median'] = round(d, 3)
        res['plumbing_ms']['difference_share_of_plain_step'] = round(d / res['plumbing_ms']['plain_step']['median'], 4)
        res['step_calls_per_sample'] = opt.step_inner
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        optim.zero_grad()
        del model, fwd_bwd, bucket, step_bucket, composed, grads, optim
        torch.cuda.empty_cache()
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write('tools/grad_bucket_bench.py: device events around runs of consecutive calls; pack in us per call, whole steps in ms per '
                'call; median and min .. max (the spread) over the samples; pack_kernels: the kernels\' device time of one call '
                '(torch.profiler); one GPU, no multi-GPU run\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
