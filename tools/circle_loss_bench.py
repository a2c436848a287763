"""Times forward + backward of the CircleLossFull drop-in (regtr_amd/losses.py, csrc/circle_loss.hip) against the same loss written with
stock torch ops and autograd on the same GPU: per pair the (N, M, D) difference tensor, its norm, the two masked terms, four
logsumexps, softplus and the selected means -- restated here from the closed form (include/regtr_hip.h, regtr_circle_rows), since the
reference tree is not on a GPU machine.
    python tools/circle_loss_bench.py [--reps 30] [--warmup 5]
Shapes: 'kitchen_b2' = 2 pairs at the kitchen golden's coarsest-level sizes (410 x 339 tokens); 'synthetic_b64' = 64 pairs of
330-460 x 330-460 tokens, D = 256.  The two paths alternate inside one process (CUDA events around forward + backward, after
warm-up).  Prints one JSON line per shape: median and minimum ms and the peak device memory above the inputs of each path, and the
two loss values.  A stock path that cannot hold its temporaries is reported as such ('torch_ops': 'out of memory'), not shrunk."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, PM, NM = 10.0, 0.1, 1.4


def torch_circle(src, tgt, sxyz, txyz, r_p, r_n):
    per = []
    for a, b, ax, bx in zip(src, tgt, sxyz, txyz):
        with torch.no_grad():
            cd = torch.cdist(ax, bx, compute_mode='donot_use_mm_for_euclid_dist')
            pos, neg = cd < r_p, cd > r_n
            row_sel = pos.any(1) & neg.any(1)
            col_sel = pos.any(0) & neg.any(0)
        d = torch.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) + 1e-12)                  # the (N, M, D) temporary
        wp = (torch.clamp_min(d - PM, 0) * pos).detach()
        wn = (torch.clamp_min(NM - d, 0) * neg).detach()
        tp, tn = S * (d - PM) * wp, S * (NM - d) * wn
        row = F.softplus(torch.logsumexp(tp, 1) + torch.logsumexp(tn, 1)) / S
        col = F.softplus(torch.logsumexp(tp, 0) + torch.logsumexp(tn, 0)) / S
        per.append((row[row_sel].mean() + col[col_sel].mean()) / 2)
    return torch.stack(per).mean()


def make(sizes, D, seed, dev):
    rng = np.random.default_rng(seed)
    t = lambda x, g=False: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev).requires_grad_(g)

    def feat(n):
        v = rng.normal(0, 1, (n, D))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.3, 1.3, (n, 1)) / np.sqrt(2.0)
    src, tgt, sx, tx = [], [], [], []
    for ns, nt in sizes:
        side = 0.25 * (max(ns, nt) ** (1 / 3)) * 1.5
        sx.append(t(rng.uniform(0, side, (ns, 3))))
        tx.append(t(rng.uniform(0, side, (nt, 3))))
        src.append(t(feat(ns), True))
        tgt.append(t(feat(nt), True))
    return src, tgt, sx, tx


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    from regtr_amd.losses import CircleLossFull
    dev = torch.device('cuda:0')
    r_p, r_n, D = 0.2, 0.4, 256
    rng = np.random.default_rng(0)
    shapes = {'kitchen_b2': [(410, 339)] * 2,
              'synthetic_b64': [(int(rng.integers(330, 461)), int(rng.integers(330, 461))) for _ in range(64)]}
    for name, sizes in shapes.items():
        src, tgt, sx, tx = make(sizes, D, 1, dev)
        crit = CircleLossFull('euclidean', r_p=r_p, r_n=r_n)
        vals = {}

        def clear():
            for p in src + tgt:
                p.grad = None

        def fused():
            clear()
            loss = crit(src, tgt, sx, tx)
            loss.backward()
            vals['fused'] = loss.detach()

        def eager():
            clear()
            loss = torch_circle(src, tgt, sx, tx, r_p, r_n)
            loss.backward()
            vals['eager'] = loss.detach()
        rec = {'shape': name, 'pairs': len(sizes), 'D': D, 'reps': args.reps,
               'nmd_temporary_mb_per_pair': round(max(a * b for a, b in sizes) * D * 4 / 2 ** 20, 1)}
        try:
            for _ in range(args.warmup):
                eager()
            have_eager = True
        except torch.OutOfMemoryError:
            have_eager = False
            clear()
            torch.cuda.empty_cache()
            rec['torch_ops'] = 'out of memory: the stock formulation cannot hold these pairs\' (N, M, D) temporaries'
        for _ in range(args.warmup):
            fused()
        torch.cuda.synchronize()
        tf, te = [], []
        for _ in range(args.reps):                            # alternating, one process
            tf.append(timed(fused))
            if have_eager:
                te.append(timed(eager))
        rec.update(fused_fwd_bwd_ms_median=round(float(np.median(tf)), 3), fused_fwd_bwd_ms_min=round(min(tf), 3),
                   fused_peak_mb=round(peak_mb(fused), 1), fused_loss=float(vals['fused']))
        if have_eager:
            rec.update(torch_ops_fwd_bwd_ms_median=round(float(np.median(te)), 3), torch_ops_fwd_bwd_ms_min=round(min(te), 3),
                       torch_ops_peak_mb=round(peak_mb(eager), 1), torch_ops_loss=float(vals['eager']),
                       speedup_median=round(float(np.median(te) / np.median(tf)), 1))
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
