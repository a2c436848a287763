"""Times what skip_nonfinite costs (regtr_amd.optim.FusedAdamW / regtr_amd.grad_bucket.GradBucket with skip_nonfinite=True;
csrc/optim.hip, csrc/grad_bucket.hip) at the real gradient sets of the ModelNet and the 3DMatch model, on one GPU in one process, the
routes of a comparison taking turns.
    python tools/nonfinite_guard_bench.py [--reps 15] [--inner 20] [--pack_inner 1000] [--step_inner 3] [--out profiles/nonfinite_guard_bench.txt]
Gradient sets as tools/optim_bench.py builds them (its `build`).  Three comparisons per model, the protocol of tools/optim_bench.py and
tools/grad_bucket_bench.py (consecutive calls between two device events; median and min .. max over `reps` samples):
  step        FusedAdamW.step guarded against unguarded, each on its own clones of the parameters with the same gradients -- per step,
              with the launches and the kernels' summed device time of ONE step (torch.profiler, a run of its own);
  add         GradBucket.add guarded (the flag pass: one more read of the gradients, then the pack under the flag) against unguarded,
              assigning and accumulating -- per call, launches and kernel time likewise;
  k2          ONE k = 2 optimiser step each way, as train_loop runs it (2 x (training_step, backward, add with the stacked losses --
              guarded: the finite-only sums and counts), attach, step).
Also recorded: whether three finite steps guarded and unguarded end bit-equal and the largest difference in float32 ulp (a
MEASUREMENT: the device forms beta^t by binary exponentiation where the host calls pow), and the launches of the flag-off paths, to be
held against the same tool's figures on the commit before the feature -- there the guarded routes are reported as absent and the
unguarded ones are measured alone."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HP = dict(lr=1e-4, weight_decay=1e-4)
CLIP = 0.1


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
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--pack_inner', type=int, default=1000)
    ap.add_argument('--step_inner', type=int, default=3)
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'nonfinite_guard_bench.txt'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/nonfinite_guard_bench.py needs an MI355X (HIP) device')
    from optim_bench import build, count_launches
    from regtr_amd.grad_bucket import GradBucket
    from regtr_amd.optim import FusedAdamW
    try:
        FusedAdamW([torch.nn.Parameter(torch.zeros(1))], skip_nonfinite=True)
        have_guard = True
    except TypeError:
        have_guard = False                # the commit before the feature: the unguarded routes alone
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    lines = []
    for name in ('modelnet', '3dmatch'):
        model, fwd_bwd = build(name, dev)
        for _ in range(3):
            fwd_bwd()
        torch.cuda.synchronize()
        with_grad = [p for p in model.parameters() if p.grad is not None]
        grads = [p.grad.detach().clone() for p in with_grad]
        n_elem = sum(p.numel() for p in with_grad)
        res = {'config': name, 'guard_available': have_guard, 'tensors_with_gradient': len(with_grad), 'elements': n_elem,
               'samples': opt.reps}

        # ---- step: FusedAdamW.step guarded against unguarded
        def clones():
            ps = [torch.nn.Parameter(p.detach().clone()) for p in with_grad]
            for p, g in zip(ps, grads):
                p.grad = g.clone()
            return ps
        routes = {'unguarded': FusedAdamW(clones(), max_grad_norm=CLIP, **HP).step}
        if have_guard:
            routes['guarded'] = FusedAdamW(clones(), max_grad_norm=CLIP, skip_nonfinite=True, **HP).step
        s = take_turns(routes, opt.reps, opt.inner, warmup=10)
        res['step_us'] = {k: stats(v) for k, v in s.items()}
        res['step_kernels'] = {}
        for k, f in routes.items():
            launches, us = count_launches(f)
            res['step_kernels'][k] = {'launches': launches, 'kernel_us': us}
        res['steps_per_sample'] = opt.inner
        if have_guard:
            res['step_us']['guarded_minus_unguarded_median'] = round(res['step_us']['guarded']['median'] - res['step_us']['unguarded']['median'], 1)
            # three finite steps each way from the same start: bit-equal?  (a measurement, not a requirement)
            pa, pb = clones(), clones()
            oa, ob = FusedAdamW(pa, max_grad_norm=CLIP, skip_nonfinite=True, **HP), FusedAdamW(pb, max_grad_norm=CLIP, **HP)
            for _ in range(3):
                oa.step(); ob.step()
            ulp = max(int((a.detach().view(torch.int32) - b.detach().view(torch.int32)).abs().max()) for a, b in zip(pa, pb))
            res['three_steps_on_against_off'] = {'bit_equal': ulp == 0, 'largest_difference_ulp': ulp, 'skipped_steps': int(oa.skipped_steps)}

        # ---- add: GradBucket.add guarded against unguarded
        buckets = {'unguarded': GradBucket(list(model.named_parameters()))}
        if have_guard:
            buckets['guarded'] = GradBucket(list(model.named_parameters()), skip_nonfinite=True)

        def add(b, fill):
            b._filled = fill
            b.add(0.5)
        routes = {}
        for k, b in buckets.items():
            b.add(0.5)
            routes[f'{k}_assign'] = lambda b=b: add(b, False)
            routes[f'{k}_accumulate'] = lambda b=b: add(b, True)
        s = take_turns(routes, opt.reps, opt.pack_inner, warmup=10)
        res['add_us'] = {k: stats(v) for k, v in s.items()}
        res['add_kernels'] = {}
        for k, f in routes.items():
            launches, us = count_launches(f)
            res['add_kernels'][k] = {'launches': launches, 'kernel_us': us}
        res['add_calls_per_sample'] = opt.pack_inner

        # ---- k2: one k = 2 optimiser step each way, as train_loop runs it
        def k2(bucket, optim, guarded):
            for _ in range(2):
                losses = fwd_bwd()
                stacked = torch.stack([v.detach() for v in losses.values()])
                if guarded:
                    fin = torch.isfinite(stacked)
                    stacked = torch.cat([torch.where(fin, stacked, torch.zeros_like(stacked)), fin.to(stacked.dtype)])
                bucket.add(0.5, stacked)
            model.optimizer.zero_grad()
            if guarded:
                bucket.attach(2, optim)
            else:
                bucket.attach()
            optim.step()
        n_keys = len(fwd_bwd())
        plain_opt = model.optimizer
        routes = {'unguarded': lambda b=GradBucket(list(model.named_parameters()), n_extra=n_keys): k2(b, plain_opt, False)}
        if have_guard:
            g_opt = FusedAdamW(list(model.parameters()), max_grad_norm=plain_opt.max_grad_norm, decoupled=plain_opt.decoupled,
                               skip_nonfinite=True, **{k: plain_opt.param_groups[0][k] for k in ('lr', 'betas', 'eps', 'weight_decay')})
            routes['guarded'] = lambda b=GradBucket(list(model.named_parameters()), n_extra=2 * n_keys, skip_nonfinite=True): k2(b, g_opt, True)
        s = take_turns(routes, opt.reps, opt.step_inner)
        res['k2_step_ms'] = {k: stats(v, 1.0) for k, v in s.items()}
        if have_guard:
            res['k2_step_ms']['guarded_minus_unguarded_median'] = round(res['k2_step_ms']['guarded']['median'] - res['k2_step_ms']['unguarded']['median'], 3)
            res['k2_skipped'] = {'steps': int(g_opt.skipped_steps)}
        res['k2_steps_per_sample'] = opt.step_inner
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        model.optimizer.zero_grad()
        del model, fwd_bwd, routes, buckets, grads, with_grad
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write('tools/nonfinite_guard_bench.py: device events around runs of consecutive calls; step and add in us per call, whole k = 2 '
                'steps in ms per call; median and min .. max (the spread) over the samples; *_kernels: launches and the kernels\' device time '
                'of one call (torch.profiler); one GPU\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
