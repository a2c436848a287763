"""Times training with the KPConv backbone in the graph (KPFEncoder.forward_grad, RegTR.training_step(train_backbone=True)) on the bench
workload (regtr_amd/workload.py: kitchen-sized synthetic 3DMatch pairs, GT poses and overlap masks from the generator's own motions).
ONE measurement per process -- a fault or a hang in one cannot start the next:
    python tools/backbone_grad_bench.py --what encoder --pairs 2        encoder forward_grad + backward on a built pyramid
    python tools/backbone_grad_bench.py --what step --pairs 2           training_step(train_backbone=True) + backward(), whole step
    python tools/backbone_grad_bench.py --what frozen --pairs 2         training_step() + backward() above the frozen backbone
    python tools/backbone_grad_bench.py --what torch --pairs 2          the same encoder in stock torch ops with autograd (float32)
each appending one JSON line to stdout; profiles/backbone_grad_bench.txt is the eight lines of
    for p in 2 64; do for w in encoder step frozen torch; do timeout -k 10 300 python tools/backbone_grad_bench.py --what $w --pairs $p --reps 5 || break 2; done; done
Per line: the median and min .. max over `reps` of the time of one call after `warmup` calls (CUDA events for `encoder` / `torch`, whose
window holds no host wait; a host clock around a synchronised step for `step` / `frozen`, which contain the preprocessor's size
read-back), and the peak allocated memory of the timed calls.  `torch` materialises the (Nq, H, 15) influences and the (Nq, H, C)
gathered rows of every convolution and pool for autograd, as the reference does: where the estimate of what it keeps alive exceeds
the device's memory the line says n/a instead of running."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from regtr_amd import context, overlap, workload                 # noqa: E402
from regtr_amd.kpconv import ResnetBottleneckBlock, SimpleBlock, UnaryBlock, _LevelView   # noqa: E402
from regtr_amd.synthetic import synth_pair                       # noqa: E402
from tests.kpconv_grads_ref import torch_forward                 # noqa: E402


def stats(ts):
    return {'ms': round(float(np.median(ts)), 3), 'spread_ms': [round(min(ts), 3), round(max(ts), 3)]}


def timed_events(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return stats(ts)


def timed_host(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


# ---- the encoder in stock torch ops (float32, autograd): kpconv_blocks.py:533-567, 590-646, 649-741 of the reference
def _t_norm(x, lens):
    return torch.cat([F.instance_norm(seg.t().unsqueeze(0)).squeeze(0).t() for seg in torch.split(x, lens)])


def _t_unary(u, x, lens, relu=True):
    y = _t_norm(x @ u.mlp.weight.t(), lens)
    return F.leaky_relu(y, 0.1) if relu else y


def _t_block(blk, x, meta, tables):
    v = _LevelView(meta, blk.layer_ind, 'strided' in blk.block_name)
    inds = tables[(blk.layer_ind, 'strided' in blk.block_name)]
    lens_pre = [int(n) for n in meta['_lens_host'][blk.layer_ind]]
    lens_post = [int(n) for n in meta['_lens_host'][blk.layer_ind + (1 if 'strided' in blk.block_name else 0)]]
    conv = lambda f: torch_forward(v.q_pts, v.s_pts, inds, f, blk.KPConv.weights, blk.KPConv.kernel_points, blk.KPConv.KP_extent)
    if isinstance(blk, SimpleBlock):
        return F.leaky_relu(_t_norm(conv(x), lens_post), 0.1)
    y = _t_unary(blk.unary1, x, lens_pre) if isinstance(blk.unary1, UnaryBlock) else x
    y = F.leaky_relu(_t_norm(conv(y), lens_post), 0.1)
    y = _t_unary(blk.unary2, y, lens_post, relu=False)
    sc = x
    if 'strided' in blk.block_name:
        sc = torch.cat([x, torch.zeros_like(x[:1])])[inds[:, :v.pool_width]].max(1)[0]
    if isinstance(blk.unary_shortcut, UnaryBlock):
        sc = _t_unary(blk.unary_shortcut, sc, lens_post, relu=False)
    return F.leaky_relu(y + sc, 0.1)


def torch_encoder_bytes(enc, meta):
    """What autograd keeps alive at least: per convolution the (Nq, H, 15) influences, their distances and the (Nq, H, Cin) gathered rows,
    per pool the (Nq, H, C) gathered rows."""
    total = 0
    for blk in enc.encoder_blocks:
        strided = 'strided' in blk.block_name
        nbr = meta['_pools_i32' if strided else '_neighbors_i32'][blk.layer_ind]
        nq, H = nbr.shape
        total += nq * H * (15 * 3 + blk.KPConv.in_channels) * 4
        if strided and isinstance(blk, ResnetBottleneckBlock):
            total += nq * H * blk.KPConv.in_channels * 4 * 4
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', choices=('encoder', 'step', 'frozen', 'torch'), required=True)
    ap.add_argument('--pairs', type=int, default=2)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    cfg, model, pairs, batch = workload.build_workload('3dmatch', args.pairs, args.points, False, 0, dev, 'fp32', head_init='uniform')
    enc = model.kpf_encoder
    rec = {'what': args.what, 'pairs': args.pairs, 'points_level0': int(sum(p.shape[0] for p in batch['src_xyz'] + batch['tgt_xyz']))}
    arith = lambda: context.forward(dev, f16_pair=False, force_x3=True, status=None)
    if args.what in ('step', 'frozen'):
        poses = torch.from_numpy(np.stack([synth_pair(i, args.points, False, return_pose=True)[2] for i in range(args.pairs)])).to(dev)
        with torch.no_grad():
            src_m, tgt_m = overlap.compute_overlap_masks(batch['src_xyz'], batch['tgt_xyz'], poses, 0.0375)
        batch.update(pose=poses, src_overlap=src_m, tgt_overlap=tgt_m)
        params = model.trainable_parameters(backbone=args.what == 'step')

        def step():
            for p in params:
                p.grad = None
            _, losses = model.training_step(batch, train_backbone=args.what == 'step')
            losses['total'].backward()
        rec.update(timed_host(step, args.reps, args.warmup))
        assert all(p.grad is not None for p in params)
    else:
        with torch.no_grad(), arith():
            meta = model.preprocessor(batch['src_xyz'] + batch['tgt_xyz'])
        ones = torch.ones((meta['points'][0].shape[0], 1), device=dev)
        gen = torch.Generator(device='cpu').manual_seed(0)
        d_out = torch.randn((meta['points'][-1].shape[0], enc.encoder_skip_dims[-1]), generator=gen).to(dev)
        rec['rows_per_level'] = [int(p.shape[0]) for p in meta['points']]
        if args.what == 'encoder':
            def run():
                enc.zero_grad(set_to_none=True)
                with arith():
                    enc.forward_grad(ones, meta).backward(d_out)
            rec.update(timed_events(run, args.reps, args.warmup))
        else:
            need, have = torch_encoder_bytes(enc, meta), torch.cuda.get_device_properties(dev).total_memory
            rec['torch_keeps_gb'] = round(need / 1e9, 1)
            if need > 0.8 * have:
                rec.update(ms='n/a', note=f'not run: autograd would keep {need / 1e9:.0f} GB alive, the device has {have / 1e9:.0f} GB')
                print(json.dumps(rec), flush=True)
                return
            tables = {(l, False): meta['_neighbors_i32'][l].long() for l in range(len(meta['points']))}
            tables.update({(l, True): meta['_pools_i32'][l].long() for l in range(len(meta['points']) - 1)})

            def run():
                enc.zero_grad(set_to_none=True)
                x = ones
                for blk in enc.encoder_blocks:
                    x = _t_block(blk, x, meta, tables)
                x.backward(d_out)
            try:
                rec.update(timed_events(run, max(args.reps // 2, 2), 1))
            except torch.cuda.OutOfMemoryError:
                rec.update(ms='n/a', note='not run: out of memory')
                print(json.dumps(rec), flush=True)
                return
    rec['peak_allocated_gb'] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
