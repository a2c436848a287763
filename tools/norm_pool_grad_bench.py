"""Times forward + backward of the differentiable InstanceNorm and max-pool operators (regtr_amd/backbone_grad.py: the plain forward ops,
csrc/norm_pool_bwd.hip backward) at the encoder's level shapes of the bench workload (regtr_amd/workload.py: 3DMatch-sized synthetic
pairs through the model's own preprocessor), against the same maths in stock torch ops on the same GPU with autograd, in the same run:
per-cloud F.instance_norm + F.leaky_relu, and index-gather + max (kpconv_blocks.py:127-143,510-519 of the reference).
    python tools/norm_pool_grad_bench.py [--pairs 64] [--reps 10] [--warmup 3] > profiles/norm_pool_grad_bench.txt
Per level l of the 3DMatch encoder: InstanceNorm + LeakyReLU over the level's rows at the bottleneck blocks' output width (128 x 2^l),
without a shortcut and with a normalised one; max-pool of those rows through the level's pooling table (levels 0-2).  Per line, medians
of CUDA-event times after warm-up, one process: forward + backward (`hip_fwd_bwd_ms`; the pool's with the transposed table built once
outside, `table_ms` beside it), the plain forward alone, the backward launches alone, and the torch formulation's forward + backward --
or why it did not run (the gather materialises Nq x H x C floats).  The pool lines also time the differentiable forward's two launches
(ops.maxpool + ops.maxpool_argmax) against the fused ops.maxpool_fwd_argmax, alternating, three rounds each.  No ratio here is a pass
criterion."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from regtr_amd import backbone_grad, ops, workload  # noqa: E402
from regtr_amd.kpconv import Preprocessor  # noqa: E402


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


def torch_instance_norm(x, lens, res=None, slope=0.1):
    def norm(v):
        return torch.cat([F.instance_norm(seg.t().unsqueeze(0)).squeeze(0).t() for seg in torch.split(v, lens)])
    z = norm(x)
    if res is not None:
        z = z + norm(res)
    return F.leaky_relu(z, slope)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-max-gb', type=float, default=64.0, help='skip the torch pool when its gathered tensor alone exceeds this')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    cfg, _, _, batch = workload.build_workload('3dmatch', args.pairs, args.points, False, 0, dev, 'fp32', head_init='uniform')
    meta = Preprocessor(cfg)(batch['src_xyz'] + batch['tgt_xyz'])
    timed = lambda fn: round(median_ms(fn, args.reps, args.warmup), 3)
    for level in range(len(meta['points'])):
        n, C = meta['points'][level].shape[0], 128 << level
        seg, lens = meta['_seg_off'][level], [int(v) for v in meta['_lens_host'][level]]
        gen = torch.Generator(device='cpu').manual_seed(level)
        x = torch.randn((n, C), generator=gen).to(dev).requires_grad_()
        r = torch.randn((n, C), generator=gen).to(dev).requires_grad_()
        g = torch.randn((n, C), generator=gen).to(dev)
        st = ops.instnorm_stats(x, seg, max(lens))
        for shortcut in (False, True):
            res, rst = (r, ops.instnorm_stats(r, seg, max(lens))) if shortcut else (None, None)

            def hip():
                x.grad = r.grad = None
                backbone_grad.instance_norm(x, seg, max(lens), res, shortcut, True).backward(g)

            def stock():
                x.grad = r.grad = None
                torch_instance_norm(x, lens, res).backward(g)
            with torch.no_grad():
                rec = {'op': 'instance_norm', 'pairs': args.pairs, 'level': level, 'rows': n, 'C': C, 'clouds': len(lens), 'normed_shortcut': shortcut,
                       'hip_fwd_ms': timed(lambda: ops.instnorm_apply(x, seg, max(lens), ops.instnorm_stats(x, seg, max(lens)), res,
                                                                      ops.instnorm_stats(r, seg, max(lens)) if shortcut else None, lrelu=True)),
                       'hip_bwd_ms': timed(lambda: ops.instnorm_bwd(x, seg, max(lens), st, g, res, rst, True, want_dres=shortcut))}
            rec['hip_fwd_bwd_ms'] = timed(hip)
            rec['torch_fwd_bwd_ms'] = round(median_ms(stock, max(args.reps // 2, 2), 1), 3)
            rec['speedup'] = round(rec['torch_fwd_bwd_ms'] / rec['hip_fwd_bwd_ms'], 2)
            print(json.dumps(rec), flush=True)
        if level + 1 < len(meta['points']):
            nbr, width = meta['_pools_i32'][level], int(meta['_pool_width'][level])
            nq, H = nbr.shape[0], width
            gq = torch.randn((nq, C), generator=gen).to(dev)
            table = ops.nbr_transpose(nbr if width == nbr.shape[1] else nbr[:, :width].contiguous(), n)
            arg = ops.maxpool_argmax(x.detach(), nbr, width)

            def hip_pool():
                x.grad = None
                backbone_grad.max_pool(x, nbr, width, transposed=table).backward(gq)
            with torch.no_grad():
                rec = {'op': 'max_pool', 'pairs': args.pairs, 'level': level, 'rows': n, 'queries': nq, 'H': H, 'C': C,
                       'hip_fwd_ms': timed(lambda: ops.maxpool(x, nbr, width)), 'argmax_ms': timed(lambda: ops.maxpool_argmax(x, nbr, width)),
                       'hip_bwd_ms': timed(lambda: ops.maxpool_bwd(gq, arg, H, table)),
                       'table_ms': timed(lambda: ops.nbr_transpose(nbr if width == nbr.shape[1] else nbr[:, :width].contiguous(), n))}
                # the forward's two launches (ops.maxpool, ops.maxpool_argmax) against the one fused launch, alternating, three rounds: the
                # spread between rounds is beside the difference
                out_b, arg_b = torch.empty((nq, C), device=dev), torch.empty((nq, C), dtype=torch.int16, device=dev)
                two, fused = [], []
                for _ in range(3):
                    two.append(timed(lambda: (ops.maxpool(x, nbr, width), ops.maxpool_argmax(x, nbr, width, out=arg_b))))
                    fused.append(timed(lambda: ops.maxpool_fwd_argmax(x, nbr, width, out=out_b, out_arg=arg_b)))
                rec['fwd_two_launches_ms'], rec['fwd_fused_ms'] = two, fused
            rec['hip_fwd_bwd_ms'] = timed(hip_pool)
            need_gb = nq * H * C * 4 / 1e9
            if need_gb > args.torch_max_gb:
                rec['torch_fwd_bwd_ms'] = None
                rec['torch_note'] = f'not run: the gathered (Nq, H, C) rows alone are {need_gb:.0f} GB'
            else:
                idx = nbr[:, :width].long()

                def stock_pool():
                    x.grad = None
                    torch.cat([x, torch.zeros_like(x[:1])])[idx].max(1)[0].backward(gq)
                try:
                    rec['torch_fwd_bwd_ms'] = round(median_ms(stock_pool, max(args.reps // 2, 2), 1), 3)
                    rec['speedup'] = round(rec['torch_fwd_bwd_ms'] / rec['hip_fwd_bwd_ms'], 2)
                except torch.cuda.OutOfMemoryError:
                    rec['torch_fwd_bwd_ms'] = None
                    rec['torch_note'] = 'not run: out of memory'
                    torch.cuda.empty_cache()
            print(json.dumps(rec), flush=True)
        del x, r, g
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
