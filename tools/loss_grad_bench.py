"""Times forward + backward of the training-loss drop-ins (regtr_amd/losses.py: InfoNCELossFull + CorrCriterion) against the same
losses written with torch ops the way the reference writes them (feature_loss.py:281-314 per pair: einsum, cdist, topk, scatter_,
masked logits, logsumexp, gather; corr_loss.py:18-40), restated here since the reference tree is not on a GPU machine.
    python tools/loss_grad_bench.py [--reps 50] [--warmup 10]
Shapes: 'kitchen_b2' = 2 pairs (the reference's train_batch_size) at the kitchen golden's coarsest-level sizes (410 x 339 tokens);
'synthetic_b64' = 64 pairs of 330-460 x 330-460 tokens (the 64-pair benchmark's coarsest level has ~394 src tokens per pair), D = 256.
Prints one JSON line per shape with the median ms of each path (CUDA events around fwd + bwd, after warm-up)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_losses(W, src, tgt, sxyz, txyz, kp, warped, pose, w, r_p, r_n):
    """The reference's two losses in torch ops (float32)."""
    Wt = torch.triu(W)
    Ws = Wt + Wt.T
    per = []
    for b in range(len(src)):
        logits = torch.einsum('ic,cd,jd->ij', src[b], Ws, tgt[b])
        with torch.no_grad():
            d = torch.cdist(sxyz[b], txyz[b])
            dist1, idx1 = d.topk(k=1, dim=-1, largest=False)
            mask = dist1[..., 0] < r_p
            ignore = d < r_n
            ignore.scatter_(-1, idx1, 0)
        logits = logits.masked_fill(ignore, float('-inf'))
        loss = -torch.gather(logits, -1, idx1).squeeze(-1) + torch.logsumexp(logits, dim=-1)
        per.append(torch.sum(loss[mask]) / torch.sum(mask))
    feat = torch.mean(torch.stack(per))
    gt = [kp[b] @ pose[b, :, :3].T + pose[b, :, 3] for b in range(len(kp))]
    err = torch.sum(torch.abs(torch.cat(warped) - torch.cat(gt)), dim=-1)
    ww = torch.cat(w)
    return feat + torch.sum(ww * err) / torch.clamp_min(torch.sum(ww), 1e-6)


def make(sizes, D, seed, dev):
    rng = np.random.default_rng(seed)
    t = lambda x, g=False: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).requires_grad_(g)
    src, tgt, sx, tx, wp, w = [], [], [], [], [], []
    for ns, nt in sizes:
        side = 0.25 * (max(ns, nt) ** (1 / 3)) * 1.5
        sx.append(t(rng.uniform(0, side, (ns, 3))))
        tx.append(t(rng.uniform(0, side, (nt, 3))))
        src.append(t(rng.normal(0, 0.2, (ns, D)), True))
        tgt.append(t(rng.normal(0, 0.2, (nt, D)), True))
        wp.append(t(sx[-1].detach().cpu().numpy() + rng.normal(0, 0.05, (ns, 3)), True))
        w.append(t(rng.uniform(0, 1, ns)))
    pose = t(np.stack([np.eye(4)[:3]] * len(sizes)))
    return src, tgt, sx, tx, wp, w, pose, t(rng.normal(0, 0.1, (D, D)), True)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    from regtr_amd.losses import CorrCriterion, InfoNCELossFull
    dev = torch.device('cuda:0')
    r_p, r_n, D = 0.2, 0.4, 256
    rng = np.random.default_rng(0)
    shapes = {'kitchen_b2': [(410, 339)] * 2,
              'synthetic_b64': [(int(rng.integers(330, 461)), int(rng.integers(330, 461))) for _ in range(64)]}
    for name, sizes in shapes.items():
        src, tgt, sx, tx, wp, w, pose, W = make(sizes, D, 1, dev)
        feat = InfoNCELossFull(D, r_p, r_n).to(dev)
        with torch.no_grad():
            feat.W.copy_(W)
        corr = CorrCriterion('mae')
        params = [feat.W, W, *src, *tgt, *wp]

        def fused():
            for p in params:
                p.grad = None
            (feat(src, tgt, sx, tx) + corr(sx, wp, pose, w)).backward()

        def eager():
            for p in params:
                p.grad = None
            torch_losses(W, src, tgt, sx, tx, sx, wp, pose, w, r_p, r_n).backward()
        ms_f = median_ms(fused, args.reps, args.warmup)
        ms_e = median_ms(eager, args.reps, args.warmup)
        print(json.dumps({'shape': name, 'pairs': len(sizes), 'D': D, 'fused_fwd_bwd_ms': round(ms_f, 3),
                          'torch_ops_fwd_bwd_ms': round(ms_e, 3), 'speedup': round(ms_e / ms_f, 2), 'reps': args.reps}))


if __name__ == '__main__':
    main()
