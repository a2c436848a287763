"""Times the optimiser step at the real parameter sets: regtr_amd.optim.FusedAdamW (clip + AdamW in three HIP kernels) against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in its default (foreach) form and with fused=True (where this torch build accepts
it), on the same GPU in the same process, alternating.
    python tools/optim_bench.py [--reps 15] [--inner 20] [--out profiles/optim_bench.txt]
Parameter sets: the ModelNet model after one training_step(train_backbone=True) + backward on B = 4 synthetic 2048-point clouds, and
the 3DMatch model after one on two synthetic 20000-point pairs -- so the tensors that hold gradients and the gradients' magnitudes are
the real ones.  Every route steps its own clones of the parameters with those gradients.
A sample is `inner` consecutive steps between two device events (so it holds whichever of launch issue and kernel time is longer, as
a training loop does); `reps` samples per route, the routes taking turns.  Reported per step: median, minimum and maximum over the
samples (the spread), kernel launches and the kernels' summed device time (torch.profiler, a run of its own), the 8-pass HBM bound --
g once for the norm, p g m v read and p m v written: 32 bytes per element at 8 TB/s -- and the fused step's median and its kernels'
time as multiples of it; and the fused step as a share of training_step + backward on the same batch."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12
HP = dict(lr=1e-4, weight_decay=1e-4)
CLIP = 0.1


def events_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
        return sum(e.count for e in ev), round(sum(e.self_device_time_total for e in ev), 1)
    except Exception as exc:      # the profiler is optional equipment of a torch build
        return f'unavailable ({type(exc).__name__})', None


def build(name, dev):
    from regtr_amd import RegTR, load_config
    from regtr_amd.augment import modelnet_train_batch, train_batch
    from regtr_amd.synthetic import synth_modelnet_cloud, synth_pair
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, 'regtr_amd', 'conf', f'{name}.yaml'))
    torch.manual_seed(0)
    model = RegTR(cfg).to(dev).eval()
    model.configure_optimizers()
    if name == 'modelnet':
        pts = [torch.from_numpy(synth_modelnet_cloud(i)).to(dev) for i in range(4)]
        make = lambda: modelnet_train_batch(pts, cfg, 1, 0)
    else:
        pairs = [synth_pair(100 + i, 20000, return_pose=True) for i in range(2)]
        src = [torch.from_numpy(p[0]).to(dev) for p in pairs]
        tgt = [torch.from_numpy(p[1]).to(dev) for p in pairs]
        pose = torch.from_numpy(np.stack([np.asarray(p[2], np.float32)[:3] for p in pairs])).to(dev)
        make = lambda: train_batch(src, tgt, pose, cfg, 1, 0)

    def fwd_bwd():
        model.optimizer.zero_grad()
        _, losses = model.training_step(make(), train_backbone=True)
        losses['total'].backward()
        return losses
    return model, fwd_bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'optim_bench.txt'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/optim_bench.py needs an MI355X (HIP) device')
    from regtr_amd.optim import FusedAdamW
    dev = torch.device('cuda', 0)
    lines = []
    for name in ('modelnet', '3dmatch'):
        model, fwd_bwd = build(name, dev)
        for _ in range(3):
            fwd_bwd()
        torch.cuda.synchronize()
        step_ms = sorted(events_ms(fwd_bwd, 3) for _ in range(5))
        with_grad = [p for p in model.parameters() if p.grad is not None]
        grads = [p.grad.detach().clone() for p in with_grad]
        n_elem = sum(p.numel() for p in with_grad)
        gnorm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))

        def clones():
            ps = [torch.nn.Parameter(p.detach().clone()) for p in with_grad]
            for p, g in zip(ps, grads):
                p.grad = g.clone()
            return ps

        routes = {}
        pf = clones()
        of = FusedAdamW(pf, max_grad_norm=CLIP, **HP)
        routes['fused_hip'] = of.step
        for label, kw in (('torch_foreach', {}), ('torch_fused', {'fused': True})):
            pt = clones()
            try:
                ot = torch.optim.AdamW(pt, **HP, **kw)

                def run(ps=pt, o=ot):
                    torch.nn.utils.clip_grad_norm_(ps, max_norm=CLIP)
                    o.step()
                run()
                routes[label] = run
            except Exception as exc:
                routes[label] = f'not accepted by this torch build ({type(exc).__name__}: {exc})'
        live = {k: f for k, f in routes.items() if callable(f)}
        for f in live.values():
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        samples = {k: [] for k in live}
        for _ in range(opt.reps):
            for k, f in live.items():
                samples[k].append(events_ms(f, opt.inner))
        bound_us = 32.0 * n_elem / HBM_BYTES_PER_S * 1e6
        res = {'config': name, 'tensors_with_gradient': len(with_grad), 'elements': n_elem, 'gradient_norm': gnorm,
               'hbm_bound_us_8_passes': round(bound_us, 1), 'training_step_plus_backward_ms_median': round(step_ms[len(step_ms) // 2], 3),
               'samples': opt.reps, 'steps_per_sample': opt.inner, 'routes': {}}
        for k, f in routes.items():
            if not callable(f):
                res['routes'][k] = f
                continue
            s = sorted(samples[k])
            launches, kernel_us = count_launches(f)
            res['routes'][k] = {'us_median': round(1e3 * s[len(s) // 2], 1), 'us_min': round(1e3 * s[0], 1), 'us_max': round(1e3 * s[-1], 1),
                                'launches_per_step': launches, 'kernel_us_per_step': kernel_us}
        fm = res['routes']['fused_hip']['us_median']
        res['fused_step_over_hbm_bound'] = round(fm / bound_us, 2)
        fk = res['routes']['fused_hip']['kernel_us_per_step']
        res['fused_kernels_over_hbm_bound'] = round(fk / bound_us, 2) if fk else None
        res['fused_share_of_training_step_plus_backward'] = round(fm / 1e3 / res['training_step_plus_backward_ms_median'], 4)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del model, fwd_bwd, routes, live
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write('tools/optim_bench.py: per optimiser step, device events around runs of consecutive steps (us); spread = min .. max over the samples\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
