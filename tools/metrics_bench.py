"""Times the device test metrics -- regtr_amd.metrics.modelnet_metrics: pose errors, Euler terms and the modified Chamfer distance -- on
717 / 717 / 2048-point clouds (source, reference, raw) at B = 4 and B = 256, next to
  * regtr_amd.evaluation.modelnet_metrics on one host core (scipy KD-trees, one pair at a time: what test.py --metrics host runs),
  * the reference's formulation in stock torch ops on the GPU (benchmark_modelnet.py:44-45, 69-76: a (B, N, M, 3) broadcast), skipped with a
    note when that temporary does not fit,
and the forward, a validation_step and a test_step at each B, with the share of the validation_step that compute_metrics takes and the
share of the forward and of the test_step that modelnet_metrics takes.

    python tools/metrics_bench.py            # rewrites profiles/metrics_bench.txt

Device times: medians of `--reps` event-timed calls after `--warmup`, over `--rounds` rounds (median of the medians, with their spread).
Host times: wall clock of one process with one thread over `--host-pairs` pairs."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('OMP_NUM_THREADS', '1')

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cross_encoder_grad_bench import median_ms               # noqa: E402
from tools.modelnet_train_input_bench import cloud                  # noqa: E402


def torch_reference_chamfer(src, ref, raw, pred, gt):
    """The reference's own formulation on stacked (B, n, 3) clouds in stock torch ops."""
    def cat(a, b):
        return torch.cat([a[:, :, :3] @ b[:, :, :3], a[:, :, :3] @ b[:, :, 3:] + a[:, :, 3:]], 2)

    def inv(a):
        rt = a[:, :, :3].transpose(1, 2)
        return torch.cat([rt, -rt @ a[:, :, 3:]], 2)

    def apply(a, p):
        return p @ a[:, :, :3].transpose(1, 2) + a[:, None, :, 3]

    def sqdist(a, b):
        return torch.sum((a[:, :, None, :] - b[:, None, :, :]) ** 2, dim=-1)

    d_src = torch.min(sqdist(apply(pred, src), raw), dim=-1)[0]
    d_ref = torch.min(sqdist(ref, apply(cat(pred, inv(gt)), raw)), dim=-1)[0]
    return d_src.mean(1) + d_ref.mean(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--host-pairs', type=int, default=32)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'metrics_bench.txt'))
    args = ap.parse_args()
    from oracle import seeded_weights
    from regtr_amd import RegTR, augment, evaluation, load_config, metrics, ops
    from regtr_amd.kernel_points import K015_CENTER
    torch.set_num_threads(1)
    cfg = load_config(os.path.join(ROOT, 'regtr_amd', 'conf', 'modelnet.yaml'))
    rng = np.random.default_rng(0)
    points = [torch.from_numpy(cloud(rng)).cuda() for _ in range(256)]
    model = RegTR(cfg)
    model.load_state_dict(seeded_weights.seeded_state_dict(cfg, 0, K015_CENTER))
    model = model.cuda().eval()
    med = lambda fn: sorted(median_ms(fn, args.reps, args.warmup) for _ in range(args.rounds))
    mid = lambda xs: xs[len(xs) // 2]
    lines = []
    for B in (4, 256):
        batch = augment.modelnet_train_batch(points[:B], cfg, 20240611, 0)           # 717-point source / reference clouds, the GT pose
        batch['tgt_raw'] = points[:B]
        pred_all = model(batch)
        pred = pred_all['pose'][-1].contiguous()
        fwd = med(lambda: model(batch))
        val = med(lambda: model.validation_step(batch))
        tst = med(lambda: model.test_step(batch))
        cm_ms = med(lambda: model.compute_metrics(pred_all, batch))
        dev_ms = med(lambda: metrics.modelnet_metrics(pred, batch))
        m = metrics.modelnet_metrics(pred, batch)
        src, ref, raw = (torch.stack(list(batch[k])) for k in ('src_xyz', 'tgt_xyz', 'tgt_raw'))
        # the nearest-neighbour launch alone (2B query clouds, both poses; its offsets' upload included), on packed inputs
        q_xyz, s_xyz = torch.cat([src, ref]).view(-1, 3), torch.cat([raw, raw]).view(-1, 3)
        q_off, s_off = [717 * i for i in range(2 * B + 1)], [2048 * i for i in range(2 * B + 1)]
        poses = torch.cat([pred, batch['pose'][:, :3, :]]).contiguous()
        nn_ms = med(lambda: ops.nearest(q_xyz, q_off, s_xyz, s_off, q_pose=poses, s_pose=poses, return_idx=False))
        rec = {'pairs': B, 'points_src_ref_raw': [717, 717, 2048], 'reps': args.reps, 'rounds': args.rounds,
               'device_modelnet_metrics_ms': round(mid(dev_ms), 4), 'device_spread_ms': [round(dev_ms[0], 4), round(dev_ms[-1], 4)],
               'device_pairs_per_s': round(1e3 * B / mid(dev_ms), 1), 'nearest_launch_alone_ms': round(mid(nn_ms), 4),
               'nearest_distance_evaluations': 2 * B * 717 * 2048,
               'forward_ms': round(mid(fwd), 3), 'modelnet_metrics_share_of_forward_percent': round(100 * mid(dev_ms) / mid(fwd), 2),
               'validation_step_ms': round(mid(val), 3), 'compute_metrics_ms': round(mid(cm_ms), 4),
               'compute_metrics_share_of_validation_step_percent': round(100 * mid(cm_ms) / mid(val), 2), 'test_step_ms': round(mid(tst), 3),
               'modelnet_metrics_share_of_test_step_percent': round(100 * mid(dev_ms) / mid(tst), 2)}
        # the reference's formulation in stock torch ops: two (B, 717, 2048, 3) float32 temporaries at a time, and their squares
        need = 3 * B * 717 * 2048 * 3 * 4
        free = torch.cuda.mem_get_info()[0]
        if need < 0.5 * free:
            gt = batch['pose'].contiguous()
            ref_ms = med(lambda: torch_reference_chamfer(src, ref, raw, pred, gt))
            want = torch_reference_chamfer(src, ref, raw, pred, gt)
            rec.update(torch_broadcast_chamfer_ms=round(mid(ref_ms), 3), torch_broadcast_temporary_gb=round(need / 2 ** 30, 2),
                       chamfer_max_rel_diff_vs_torch=float(((m['chamfer_dist'] - want).abs() / want).max()))
        else:
            rec['torch_broadcast_chamfer_ms'] = f'skipped: the broadcast temporaries need {need / 2 ** 30:.1f} GiB, {free / 2 ** 30:.1f} GiB free'
        # the host function on one core, one pair at a time (test.py --metrics host)
        n_host = min(B, args.host_pairs)
        hp, hg = pred[:n_host].cpu().numpy(), batch['pose'][:n_host].cpu().numpy()
        hs, hr, hw = src[:n_host].cpu().numpy(), ref[:n_host].cpu().numpy(), raw[:n_host].cpu().numpy()
        evaluation.modelnet_metrics(hp[:1], hg[:1], hs[:1], hr[:1], hw[:1])          # (scipy's first call: imports, not metrics)
        t0 = time.perf_counter()
        host = [evaluation.modelnet_metrics(hp[b:b + 1], hg[b:b + 1], hs[b:b + 1], hr[b:b + 1], hw[b:b + 1]) for b in range(n_host)]
        host_ms = 1e3 * (time.perf_counter() - t0) / n_host
        hc = np.concatenate([h['chamfer_dist'] for h in host])
        rec.update(host_pairs_timed=n_host, host_ms_per_pair_one_core=round(host_ms, 3), host_pairs_per_s_one_core=round(1e3 / host_ms, 1),
                   chamfer_max_rel_diff_vs_host=float(np.abs(m['chamfer_dist'][:n_host].cpu().numpy() - hc).max() / hc.min()))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
