"""Times forward + backward of the differentiable KPConv operator (KPConv.forward_grad: ops.kpconv forward, csrc/kpconv_bwd.hip backward)
on the real neighbour tables of the bench workload, against the reference's formulation (kpconv_blocks.py:309-412) written in stock
torch ops on the same GPU with autograd (tests/kpconv_grads_ref.py: torch_forward, which materialises the (Nq, H, 15) influences and the
(Nq, H, Cin) gathered features as the reference does).
    python tools/kpconv_grad_bench.py [--pairs 2,64] [--reps 10] [--warmup 3] > profiles/kpconv_grad_bench.txt
The four conv shapes of the 3DMatch encoder (Cin = Cout = 32 / 64 / 128 / 256 at levels 0-3, H = 40; level sizes are those of
regtr_amd/synthetic.py's kitchen-sized pairs).  Per line, medians of CUDA-event times after warm-up, one process: forward + backward
with the transposed table built once outside (`hip_fwd_bwd_ms`, what a level's blocks pay when they share it), the table build alone
(`table_ms`), the dX kernel alone (`gather_bwd_ms`), the forward alone, and the torch formulation's forward + backward -- or why it did
not run (it needs Nq x H x (15 x 4 + 2 Cin) floats at once)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from regtr_amd import load_config, ops  # noqa: E402
from regtr_amd.kpconv import KPConv, Preprocessor  # noqa: E402
from tests.kpconv_grads_ref import torch_forward  # noqa: E402


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
    ap.add_argument('--pairs', default='2,64')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-max-gb', type=float, default=64.0, help='skip the torch formulation when its gathered tensors alone exceed this')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    cfg = load_config(os.path.join(bench.ROOT, 'regtr_amd', 'conf', '3dmatch.yaml'))
    r0 = cfg.first_subsampling_dl * cfg.conv_radius
    np.random.seed(0)
    for n_pairs in (int(p) for p in args.pairs.split(',')):
        pairs = [bench.synth_pair(i, 20000) for i in range(n_pairs)]
        pts = [torch.from_numpy(s).to(dev) for s, _ in pairs] + [torch.from_numpy(t).to(dev) for _, t in pairs]
        meta = Preprocessor(cfg)(pts)
        for layer, C in enumerate((32, 64, 128, 256)):
            s_pts, nbr = meta['points'][layer], meta['_neighbors_i32'][layer]
            n, H = nbr.shape
            radius = r0 * 2 ** layer
            conv = KPConv(15, 3, C, C, radius * cfg.KP_extent / cfg.conv_radius, radius).to(dev)
            gen = torch.Generator(device='cpu').manual_seed(layer)
            x = torch.randn((n, C), generator=gen).to(dev).requires_grad_()
            g = torch.randn((n, C), generator=gen).to(dev)
            table = ops.nbr_transpose(nbr, n)

            def hip():
                x.grad = None
                conv.weights.grad = None
                conv.forward_grad(s_pts, s_pts, nbr, x, transposed=table).backward(g)

            def fwd():
                with torch.no_grad():
                    conv(s_pts, s_pts, nbr, x)
            dwf = torch.randn((n, 15 * C), generator=gen).to(dev)
            rec = {'pairs': n_pairs, 'level': layer, 'rows': n, 'H': H, 'Cin': C, 'Cout': C,
                   'hip_fwd_bwd_ms': round(median_ms(hip, args.reps, args.warmup), 3),
                   'hip_fwd_ms': round(median_ms(fwd, args.reps, args.warmup), 3),
                   'table_ms': round(median_ms(lambda: ops.nbr_transpose(nbr, n), args.reps, args.warmup), 3),
                   'gather_bwd_ms': round(median_ms(lambda: ops.kpconv_gather_bwd(dwf, s_pts, s_pts, H, conv.kernel_points.detach(),
                                                                                   conv.KP_extent, table), args.reps, args.warmup), 3)}
            del dwf
            need_gb = n * H * (15 * 4 + 2 * C) * 4 / 1e9
            if need_gb > args.torch_max_gb:
                rec['torch_fwd_bwd_ms'] = None
                rec['torch_note'] = f'not run: the (Nq, H, 15, 3) differences and (Nq, H, Cin) gathered rows alone are {need_gb:.0f} GB'
            else:
                nbr64 = nbr.long()
                w = conv.weights.detach().clone().requires_grad_()
                kp = conv.kernel_points.detach()

                def stock():
                    x.grad = None
                    w.grad = None
                    torch_forward(s_pts, s_pts, nbr64, x, w, kp, conv.KP_extent).backward(g)
                try:
                    rec['torch_fwd_bwd_ms'] = round(median_ms(stock, max(args.reps // 2, 2), 1), 3)
                    rec['speedup'] = round(rec['torch_fwd_bwd_ms'] / rec['hip_fwd_bwd_ms'], 2)
                except torch.cuda.OutOfMemoryError:
                    rec['torch_fwd_bwd_ms'] = None
                    rec['torch_note'] = 'not run: out of memory'
                    torch.cuda.empty_cache()
            print(json.dumps(rec), flush=True)
            del x, g, table, conv
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
