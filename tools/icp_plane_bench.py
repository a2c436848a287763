"""Times point-to-plane ICP (regtr_amd.refine.icp(method='point_to_plane'), csrc/icp_plane.hip) against point-to-point ICP at the same commit,
alternating in one process, and reports what each buys.
    python tools/icp_plane_bench.py [--reps 15] [--iters 30] [--pairs 2,64] [--out profiles/icp_plane_bench.txt]
The setup is tools/icp_bench.py's: the synthetic 3DMatch-sized rooms (~20 k points per cloud), pose0 = the ground truth composed with a
seeded error of 1.5 degrees / 5 cm, max_dist = 2 x first_subsampling_dl.  Per batch size one JSON line: median and min .. max over the
samples, between device events, of one whole call of
    point_to_point            refine.icp (grid build + iters + 1 steps)
    point_to_plane            the fused route, normals included: the matching grid, a second grid when normal_radius asks for wider cells,
                              regtr_estimate_normals, iters + 1 steps
    point_to_plane_composed   the same iteration from the separate operators (refine.use_fused_icp(False))
and of estimate_normals alone (its own grid build included) beside the bytes it must move, computed from the shapes: per point 12 B read,
27 slots of 32 B, 16 B per candidate of the 27 cells (an estimate: the mean neighbour count the run reports, times the ratio of the
27-cell volume to the ball's, 27 / (4 pi / 3)), 16 B written; iterations run, errors against the ground truth before and after, and the
kernel launches of one call of each (torch.profiler, a run of its own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from icp_bench import errors, launches, perturb, stats, timed      # noqa: E402  (the point-to-point bench's setup, exactly)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--pairs', type=str, default='2,64')
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--normal_radius', type=float, default=None, help='default: max_dist (the matching grid serves the normals)')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'icp_plane_bench.txt'))
    opt = ap.parse_args()
    from regtr_amd import load_config, refine
    from regtr_amd.synthetic import synth_pair
    dev = torch.device('cuda:0')
    cfg = load_config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'regtr_amd', 'conf', '3dmatch.yaml'))
    md = 2 * cfg.first_subsampling_dl
    nr = md if opt.normal_radius is None else opt.normal_radius
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

        def run(route):
            prev = refine.use_fused_icp(route != 'point_to_plane_composed')
            try:
                kw = {} if route == 'point_to_point' else {'method': 'point_to_plane', 'normal_radius': nr}
                out[route] = refine.icp(src, tgt, pose0, md, iters=opt.iters, **kw)
            finally:
                refine.use_fused_icp(prev)

        def normals():
            out['normals'] = refine.estimate_normals(tgt, nr, return_moments=True)
        routes = ('point_to_point', 'point_to_plane', 'point_to_plane_composed')
        for _ in range(opt.warmup):
            for r in routes:
                run(r)
            normals()
        torch.cuda.synchronize()
        t = {r: [] for r in routes + ('estimate_normals',)}
        for _ in range(opt.reps):                       # alternating, one process
            for r in routes:
                t[r].append(timed(lambda: run(r)))
            t['estimate_normals'].append(timed(normals))
        n_tgt = sum(int(c.shape[0]) for c in tgt)
        nbr = float(torch.cat(out['normals'][2])[:, 0].double().mean())
        valid = float(torch.cat(out['normals'][1]).double().mean())
        bytes_normals = n_tgt * (12 + 27 * 32 + 16 * nbr * 27 / (4 * np.pi / 3) + 16)
        med = {r: float(np.median(t[r])) for r in t}
        rec = {'pairs': B, 'points_per_cloud': opt.points, 'target_rows': n_tgt, 'max_dist': md, 'normal_radius': nr, 'iters_max': opt.iters,
               'samples': opt.reps, 'icp_ms': {r: stats(t[r]) for r in routes},
               'plane_over_point_median': round(med['point_to_plane'] / med['point_to_point'], 3),
               'composed_over_fused_median': round(med['point_to_plane_composed'] / med['point_to_plane'], 2),
               'estimate_normals_ms': stats(t['estimate_normals']),
               'normals_share_of_plane_call': round(med['estimate_normals'] / med['point_to_plane'], 3),
               'normals_neighbours_mean': round(nbr, 2), 'normals_valid_share': round(valid, 5),
               'normals_bytes_mb': round(bytes_normals / 2 ** 20, 1), 'normals_at_hbm_peak_us': round(bytes_normals / 6.3e12 * 1e6, 1),
               'launches_per_call': {r: launches(lambda: run(r)) for r in routes},
               'iters_run_mean': {r: round(float(out[r].iters_run.double().mean()), 2) for r in routes},
               'iters_run_max': {r: int(out[r].iters_run.max()) for r in routes},
               'routes_same_matches': bool(torch.equal(out['point_to_plane'].n_inliers, out['point_to_plane_composed'].n_inliers)),
               'rot_err_deg_trans_err_m': dict({'before': [round(x, 5) for x in errors(pose0_np, gt)]},
                                               **{r: [round(x, 5) for x in errors(out[r].pose.cpu().numpy(), gt)] for r in routes}),
               'fitness': {r: round(float(out[r].fitness.mean()), 4) for r in routes},
               'inlier_rmse': {r: round(float(out[r].inlier_rmse.mean()), 5) for r in routes}}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del src, tgt, out
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write('tools/icp_plane_bench.py: device events around one refine.icp call, point to point (grid build + up to iters + 1 steps), point '
                'to plane fused (normals and every grid build included) and point to plane composed, alternating in one process, and around '
                'estimate_normals alone (its grid build included); median and min .. max over the samples; launches: kernels of one call '
                '(torch.profiler, a run of its own); errors against the synthetic ground truth; normals_bytes_mb: computed from the shapes, '
                'not measured; one MI355X.  Not measured: per-kernel times and counters.\n')
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
