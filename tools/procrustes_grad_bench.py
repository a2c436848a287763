"""Times the differentiable pose solve: ops.weighted_procrustes + ops.weighted_procrustes_bwd (one HIP launch each, csrc/procrustes.hip)
against the reference's formulation -- sigmoid, normalised weights, centroids, covariance, a 3x3 SVD, the determinant's sign, per pair
in a Python loop as models/regtr.py:185-203 runs it -- in stock torch ops with autograd, on the same GPU in the same process, taking turns.
    python tools/procrustes_grad_bench.py [--reps 15] [--inner 10] [--out profiles/procrustes_grad_bench.txt]
Shapes: 2 pairs of (410, 339) coarse tokens (the 3DMatch kitchen pair's) and 64 such pairs, one decoder layer (what RegTR.forward_grad
solves).  Then training_step(train_backbone=True) + backward on two synthetic 20000-point 3DMatch pairs with cfg.wt_pose absent and 1.
A sample is `inner` consecutive calls between two device events; `reps` samples per route.  Reported per call: median and min .. max
over the samples.  Nothing is fixed in advance: the file holds what was measured."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def events_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def torch_kabsch(a, b, w):
    """Weighted Kabsch of one pair in stock torch ops (a, b (n, 3), w (n,)) -> (3, 4)."""
    wn = (w / w.sum().clamp_min(1e-6)).unsqueeze(1)
    ca, cb = (a * wn).sum(0), (b * wn).sum(0)
    H = (a - ca).t() @ ((b - cb) * wn)
    U, _, Vh = torch.linalg.svd(H)
    V = Vh.t()
    flip = torch.ones(3, dtype=a.dtype, device=a.device)
    flip[2] = torch.sign(torch.det(V @ U.t()))
    Rm = (V * flip) @ U.t()
    return torch.cat([Rm, (cb - Rm @ ca).unsqueeze(1)], dim=1)


def op_case(n_pairs, dev, rng):
    from regtr_amd import head_grad
    lens = [410] * n_pairs + [339] * n_pairs
    off = np.concatenate([[0], np.cumsum(lens)])
    N = int(off[-1])
    kp = torch.from_numpy(rng.standard_normal((N, 3)).astype(np.float32)).to(dev)
    corr = (kp @ torch.diag(torch.tensor([1.0, 0.8, 0.6], device=dev)) + 0.1 * torch.randn((1, N, 3), device=dev)).requires_grad_()
    logit = torch.from_numpy(rng.uniform(-2, 2, (1, N)).astype(np.float32)).to(dev).requires_grad_()
    seg = torch.from_numpy(off.astype(np.int32)).to(dev)
    d_pose = torch.randn((1, n_pairs, 3, 4), device=dev)

    def hip():
        corr.grad = logit.grad = None
        (head_grad.procrustes_forward_grad(kp, corr, logit, seg, n_pairs) * d_pose).sum().backward()

    def stock():
        corr.grad = logit.grad = None
        poses = []
        for p in range(n_pairs):
            s, t = slice(off[p], off[p + 1]), slice(off[n_pairs + p], off[n_pairs + p + 1])
            poses.append(torch_kabsch(torch.cat([kp[s], corr[0, t]]), torch.cat([corr[0, s], kp[t]]),
                                      torch.sigmoid(torch.cat([logit[0, s], logit[0, t]]))))
        (torch.stack(poses)[None] * d_pose).sum().backward()

    hip()
    g_hip = (corr.grad.clone(), logit.grad.clone())
    stock()
    agree = max(float((corr.grad - g_hip[0]).abs().max() / g_hip[0].abs().max()), float((logit.grad - g_hip[1]).abs().max() / g_hip[1].abs().max()))
    return {'hip_forward_backward': hip, 'torch_ops_autograd': stock}, agree


def training_case(wt_pose, dev):
    from regtr_amd import RegTR, load_config
    from regtr_amd.augment import train_batch
    from regtr_amd.synthetic import synth_pair
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, 'regtr_amd', 'conf', '3dmatch.yaml'))
    if wt_pose:
        cfg.wt_pose = wt_pose
    torch.manual_seed(0)
    model = RegTR(cfg).to(dev).eval()
    model.configure_optimizers()
    pairs = [synth_pair(100 + i, 20000, return_pose=True) for i in range(2)]
    src = [torch.from_numpy(p[0]).to(dev) for p in pairs]
    tgt = [torch.from_numpy(p[1]).to(dev) for p in pairs]
    pose = torch.from_numpy(np.stack([np.asarray(p[2], np.float32)[:3] for p in pairs])).to(dev)

    def fwd_bwd():
        model.optimizer.zero_grad()
        _, losses = model.training_step(train_batch(src, tgt, pose, cfg, 1, 0), train_backbone=True)
        losses['total'].backward()
    return fwd_bwd


def summary(samples):
    s = sorted(samples)
    return {'ms_median': round(s[len(s) // 2], 4), 'ms_min': round(s[0], 4), 'ms_max': round(s[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'procrustes_grad_bench.txt'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/procrustes_grad_bench.py needs an MI355X (HIP) device')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    lines = []
    for n_pairs in (2, 64):
        routes, agree = op_case(n_pairs, dev, rng)
        for f in routes.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        samples = {k: [] for k in routes}
        for _ in range(opt.reps):
            for k, f in routes.items():
                samples[k].append(events_ms(f, opt.inner if n_pairs == 2 else max(opt.inner // 5, 1)))
        res = {'case': f'operator forward + backward, {n_pairs} pairs of (410, 339) tokens, 1 layer', 'samples': opt.reps,
               'gradients_max_rel_difference_between_routes': agree, 'routes': {k: summary(v) for k, v in samples.items()}}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    steps = {('wt_pose 1' if w else 'wt_pose absent'): training_case(w, dev) for w in (0, 1.0)}
    for f in steps.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    samples = {k: [] for k in steps}
    for _ in range(opt.reps):
        for k, f in steps.items():
            samples[k].append(events_ms(f, 2))
    res = {'case': 'training_step(train_backbone=True) + backward, 3dmatch.yaml, 2 synthetic 20000-point pairs', 'samples': opt.reps,
           'routes': {k: summary(v) for k, v in samples.items()}}
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write('tools/procrustes_grad_bench.py: per call, device events around runs of consecutive calls (ms); spread = min .. max over the samples\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
