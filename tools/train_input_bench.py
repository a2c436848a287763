"""Times the input side of training -- regtr_amd.augment.train_batch: ground-truth overlap masks of the clean clouds, then the reference's
augmentation chain, all on the device -- on resident raw pairs, and next to it the same work on the host: the numpy restatement of the
chain (tests/augment_ref.py) plus a CPU mask computation of the reference's shape (utils/pointcloud.py:8-65: one KD-tree nearest-neighbour
query each way per pair, scipy's cKDTree standing in for open3d's KDTreeFlann).

    python tools/train_input_bench.py [--reps 20] [--warmup 5] [--rounds 3] [--host-pairs 4] [--out profiles/train_input_bench.txt]

Shapes: 'kitchen_b2' = 2 and 'synthetic_b64' = 64 synthetic 3DMatch-sized pairs (regtr_amd/synthetic.py, 20000 points a cloud before the
generator's own voxel thinning), the batches tools/backbone_grad_bench.py times a training step on.  Device times: CUDA events around one
train_batch call with `step` counting up, median over `reps`, repeated `rounds` times -> median of the rounds' medians and their min .. max;
the masks and the augmentation are also timed apart.  Host times: wall clock of one process on one core over the first `--host-pairs` pairs,
per pair (a loader pool divides it by its worker count at best).  The share of a training step is taken against the `step` rows of
profiles/backbone_grad_bench.txt (not re-measured here).  One JSON line per shape, written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.cross_encoder_grad_bench import median_ms      # noqa: E402


def step_ms(pairs):
    """ms of training_step(train_backbone=True) + backward at `pairs` pairs from profiles/backbone_grad_bench.txt (None when absent)."""
    path = os.path.join(ROOT, 'profiles', 'backbone_grad_bench.txt')
    if not os.path.exists(path):
        return None
    for line in open(path):
        rec = json.loads(line)
        if rec.get('what') == 'step' and rec.get('pairs') == pairs:
            return rec['ms']
    return None


def host_pair_ms(pairs, cfg, seed, n):
    """Wall-clock ms per pair of the host path over the first n pairs: (masks, chain)."""
    from scipy.spatial import cKDTree
    from tests import augment_ref as R
    n = min(n, len(pairs))
    t_mask = t_chain = 0.0
    sizes = ([len(p[0]) for p in pairs[:n]], [len(p[1]) for p in pairs[:n]])
    t0 = time.perf_counter()
    d = R.draws(seed, 0, sizes, perturb_pose=cfg.get('perturb_pose', 'small'))
    t_chain += time.perf_counter() - t0
    for b, (src, tgt, pose) in enumerate(pairs[:n]):
        t0 = time.perf_counter()
        sw = src.astype(np.float64) @ pose[:3, :3].astype(np.float64).T + pose[:3, 3]
        r = cfg.overlap_radius
        sm = cKDTree(tgt.astype(np.float64)).query(sw, k=1, distance_upper_bound=r)[0] < r
        tm = cKDTree(sw).query(tgt.astype(np.float64), k=1, distance_upper_bound=r)[0] < r
        t1 = time.perf_counter()
        R.apply({'src_xyz': src, 'tgt_xyz': tgt, 'pose': pose, 'src_overlap': sm, 'tgt_overlap': tm}, R.pair_of(d, b),
                augment_noise=cfg.get('augment_noise', 0.005), perturb_pose=cfg.get('perturb_pose', 'small'))
        t2 = time.perf_counter()
        t_mask += t1 - t0
        t_chain += t2 - t1
    return 1e3 * t_mask / n, 1e3 * t_chain / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--host-pairs', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_input_bench.txt'))
    args = ap.parse_args()
    from regtr_amd import augment, load_config, overlap
    from regtr_amd.synthetic import synth_pair
    cfg = load_config(os.path.join(ROOT, 'regtr_amd', 'conf', '3dmatch.yaml'))
    dev = torch.device('cuda', 0)
    seed = 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, 'w').close()                                     # a run replaces the file
    for name, B in (('kitchen_b2', 2), ('synthetic_b64', 64)):
        pairs = [synth_pair(i, args.points, False, return_pose=True) for i in range(B)]
        srcs = [torch.from_numpy(np.ascontiguousarray(p[0], dtype=np.float32)).to(dev) for p in pairs]
        tgts = [torch.from_numpy(np.ascontiguousarray(p[1], dtype=np.float32)).to(dev) for p in pairs]
        poses = torch.from_numpy(np.stack([np.asarray(p[2], dtype=np.float32)[:3] for p in pairs])).to(dev)
        counter = [0]

        def whole():
            counter[0] += 1
            return augment.train_batch(srcs, tgts, poses, cfg, seed, counter[0])
        sm, tm = overlap.compute_overlap_masks(srcs, tgts, poses, cfg.overlap_radius)
        clean = {'src_xyz': srcs, 'tgt_xyz': tgts, 'pose': poses, 'src_overlap': sm, 'tgt_overlap': tm}

        def masks():
            return overlap.compute_overlap_masks(srcs, tgts, poses, cfg.overlap_radius)

        def chain():
            counter[0] += 1
            return augment.augment_batch(clean, seed, counter[0], augment_noise=cfg.augment_noise, perturb_pose=cfg.perturb_pose)
        ms = {k: [] for k in ('train_batch', 'masks', 'augment')}
        for _ in range(args.rounds):                                # timed in alternation
            for k, fn in (('train_batch', whole), ('masks', masks), ('augment', chain)):
                ms[k].append(median_ms(fn, args.reps, args.warmup))
        rec = {'shape': name, 'pairs': B, 'points': int(sum(x.shape[0] for x in srcs + tgts)), 'reps': args.reps, 'rounds': args.rounds}
        for k, v in ms.items():
            rec[k + '_ms'] = round(float(np.median(v)), 3)
            rec[k + '_spread_ms'] = [round(min(v), 3), round(max(v), 3)]
        rec['pairs_per_s'] = round(B / rec['train_batch_ms'] * 1e3, 1)
        step = step_ms(B)
        if step is not None:
            rec['training_step_ms'] = step
            rec['share_of_step_percent'] = round(100.0 * rec['train_batch_ms'] / step, 2)
        hm, hc = host_pair_ms([(np.asarray(p[0], np.float32), np.asarray(p[1], np.float32), np.asarray(p[2], np.float32)) for p in pairs],
                              cfg, seed, args.host_pairs)
        rec.update(host_pairs_timed=min(args.host_pairs, B), host_masks_ms_per_pair=round(hm, 2), host_chain_ms_per_pair=round(hc, 2),
                   host_pairs_per_s_one_core=round(1e3 / (hm + hc), 1))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
