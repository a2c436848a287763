"""Times regtr_amd.refine.icp (csrc/icp.hip) -- the fused route against the composed route (ops.se3_transform, regtr_nearest_in_radius, torch
gathers and sums, se3.compute_rigid_transform), alternating in one process -- and reports what the refinement buys.
    python tools/icp_bench.py [--reps 15] [--iters 30] [--pairs 2,64] [--out profiles/icp_bench.txt]
Inputs: the project's synthetic 3DMatch-sized rooms (regtr_amd.synthetic.synth_pair, ~20 k points per cloud) with their ground-truth
poses; pose0 = the ground truth composed with a RegTR-sized error, a seeded draw of about 1.5 degrees about a random axis and 5 cm in a
random direction; max_dist = 2 x first_subsampling_dl.  Per batch size one JSON line: median and min .. max over the samples, between
device events, of one whole refine.icp call (grid build + iters + 1 steps) on each route; the kernel launches of one call of each
(torch.profiler, a run of its own); the mean rotation / translation error against the ground truth before and after; fitness and
inlier_rmse before and after; iterations run; the time of a RegTR forward at the same batch and refine's share of it; and the bytes the
fused accumulate pass must move per iteration (computed from the shapes: 12 B per source row, 27 slots of 32 B, 16 B per candidate met)
over the measured time per iteration, beside the launch count -- which of the two bounds the pass sits against."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def perturb(gt, rng, deg=1.5, shift=0.05):
    """gt (3, 4) composed with a rotation of `deg` about a random axis through the target cloud's frame origin and a shift of `shift`."""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.radians(deg)
    dR = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    d = rng.standard_normal(3)
    d *= shift / np.linalg.norm(d)
    return np.concatenate([dR @ gt[:, :3], (dR @ gt[:, 3] + d)[:, None]], axis=1)


def errors(pose, gt):
    pose, gt = np.asarray(pose, np.float64), np.asarray(gt, np.float64)
    Rd = np.einsum('nij,nkj->nik', pose[:, :, :3], gt[:, :, :3])
    ang = np.degrees(np.arccos(np.clip((np.trace(Rd, axis1=1, axis2=2) - 1) / 2, -1, 1)))
    return float(ang.mean()), float(np.linalg.norm(pose[:, :, 3] - gt[:, :, 3], axis=1).mean())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.key_averages() if 'memcpy' not in e.key.lower() and 'memset' not in e.key.lower()]
    return int(sum(e.count for e in ev))


def stats(v):
    return {'median': round(float(np.median(v)), 3), 'min': round(float(min(v)), 3), 'max': round(float(max(v)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--pairs', type=str, default='2,64')
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'icp_bench.txt'))
    opt = ap.parse_args()
    from regtr_amd import RegTR, load_config, refine
    from regtr_amd.synthetic import synth_pair
    dev = torch.device('cuda:0')
    cfg = load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'regtr_amd', 'conf', '3dmatch.yaml'))
    md = 2 * cfg.first_subsampling_dl
    torch.manual_seed(0)
    model = RegTR(cfg).to(dev).eval()
    lines = []
    for B in [int(x) for x in opt.pairs.split(',')]:
        rng = np.random.default_rng(1000 + B)
        gen = [synth_pair(5000 + i, opt.points, return_pose=True) for i in range(min(B, 8))]      # (64 pairs: eight rooms, eight times)
        items = [gen[i % len(gen)] for i in range(B)]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        src, tgt = [up(it[0]) for it in items], [up(it[1]) for it in items]
        gt = np.stack([np.asarray(it[2], np.float64)[:3] for it in items])
        pose0_np = np.stack([perturb(g, rng) for g in gt])
        pose0 = up(pose0_np)
        out = {}

        def run(fused, iters=opt.iters):
            prev = refine.use_fused_icp(fused)
            try:
                out['fused' if fused else 'composed'] = refine.icp(src, tgt, pose0, md, iters=iters)
            finally:
                refine.use_fused_icp(prev)

        def forward():
            with torch.no_grad():
                model({'src_xyz': src, 'tgt_xyz': tgt})
        for _ in range(opt.warmup):
            run(True); run(False); forward()
        torch.cuda.synchronize()
        t = {'fused': [], 'composed': [], 'forward': [], 'evaluate': []}
        for _ in range(opt.reps):                       # alternating, one process
            t['fused'].append(timed(lambda: run(True)))
            t['composed'].append(timed(lambda: run(False)))
            t['forward'].append(timed(forward))
            t['evaluate'].append(timed(lambda: refine.evaluate_registration(src, tgt, pose0, md)))
        rf, rc = out['fused'], out['composed']
        before = refine.evaluate_registration(src, tgt, pose0, md)
        n_src = sum(int(s.shape[0]) for s in src)
        # bytes one accumulate pass must move: the source rows, 27 packed slots per row, and the candidates of the occupied cells (an
        # estimate of the last: 27 target rows per source row, about what cells of 2 x the voxel size hold around a surface point)
        bytes_pass = n_src * (12 + 27 * 32 + 16 * 27)
        rec = {'pairs': B, 'points_per_cloud': opt.points, 'source_rows': n_src, 'max_dist': md, 'iters_max': opt.iters, 'samples': opt.reps,
               'icp_ms': {'fused': stats(t['fused']), 'composed': stats(t['composed'])},
               'speedup_median': round(float(np.median(t['composed']) / np.median(t['fused'])), 2),
               'evaluate_registration_ms': stats(t['evaluate']),
               'launches_per_call': {'fused': launches(lambda: run(True)), 'composed': launches(lambda: run(False))},
               'iters_run_mean': round(float(rf.iters_run.double().mean()), 2), 'iters_run_max': int(rf.iters_run.max()),
               'routes_same_matches': bool(torch.equal(rf.n_inliers, rc.n_inliers)),
               'rot_err_deg_trans_err_m': {'before': [round(x, 5) for x in errors(pose0_np, gt)],
                                           'after_fused': [round(x, 5) for x in errors(rf.pose.cpu().numpy(), gt)],
                                           'after_composed': [round(x, 5) for x in errors(rc.pose.cpu().numpy(), gt)]},
               'fitness': {'before': round(float(before[0].mean()), 4), 'after': round(float(rf.fitness.mean()), 4)},
               'inlier_rmse': {'before': round(float(before[1].mean()), 5), 'after': round(float(rf.inlier_rmse.mean()), 5)},
               'forward_ms': stats(t['forward']),
               'refine_share_of_forward': round(float(np.median(t['fused']) / np.median(t['forward'])), 3),
               'fused_ms_per_step_mean': round(float(np.median(t['fused'])) / (opt.iters + 1), 4),
               'accumulate_bytes_per_pass_mb': round(bytes_pass / 2 ** 20, 1),
               'accumulate_at_hbm_peak_us': round(bytes_pass / 6.3e12 * 1e6, 1)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del src, tgt, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write('tools/icp_bench.py: device events around one refine.icp call (grid build + up to iters + 1 steps), fused and composed routes '
                'alternating in one process; median and min .. max over the samples; launches: kernels of one call (torch.profiler, a run '
                'of its own); errors against the synthetic ground truth; one MI355X.  Not measured: per-kernel times and counters.\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
