"""Times the input side of ModelNet training -- regtr_amd.augment.modelnet_train_batch: crop, Euler transform, resample, jitter, shuffle
and the crop's overlap masks, all on the device -- on resident raw clouds of 2048 points at B = 4 (conf/modelnet.yaml's batch) and
B = 256, next to the numpy restatement of the chain (tests/modelnet_augment_ref.py) on one host core, and a
training_step(train_backbone=True) + backward at B = 4, whose share the chain is.

    python tools/modelnet_train_input_bench.py            # appends nothing: rewrites profiles/modelnet_train_input_bench.txt

Device times: medians of `--reps` event-timed calls after `--warmup`, over `--rounds` rounds (median of the medians, with their spread).
Host times: wall clock of one process over `--host-clouds` clouds."""
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


def cloud(rng, n=2048):
    """Seeded points on a box and a sphere inside the unit ball."""
    a = n // 2
    dims = np.array([1.0, 0.6, 0.3])
    box = rng.uniform(-0.5, 0.5, (a, 3)) * dims
    face = rng.integers(0, 3, a)
    box[np.arange(a), face] = np.sign(box[np.arange(a), face]) * 0.5 * dims[face]
    v = rng.standard_normal((n - a, 3))
    ball = 0.35 * v / np.linalg.norm(v, axis=1, keepdims=True) + np.array([0.2, 0.1, 0.25])
    return np.concatenate([box, ball]).astype(np.float32)[rng.permutation(n)]


def host_cloud_ms(clouds, cfg, seed):
    from tests import modelnet_augment_ref as M
    t0 = time.perf_counter()
    d = M.draws(seed, 0, [len(c) for c in clouds], cfg.rot_mag, cfg.trans_mag)
    for b, c in enumerate(clouds):
        M.apply(c, M.cloud_of(d, b))
    return 1e3 * (time.perf_counter() - t0) / len(clouds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--host-clouds', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'modelnet_train_input_bench.txt'))
    args = ap.parse_args()
    from oracle import seeded_weights
    from regtr_amd import RegTR, augment, load_config
    from regtr_amd.kernel_points import K015_CENTER
    cfg = load_config(os.path.join(ROOT, 'regtr_amd', 'conf', 'modelnet.yaml'))
    seed = 20240611
    rng = np.random.default_rng(0)
    host = [cloud(rng) for _ in range(256)]
    dev = [torch.from_numpy(c).cuda() for c in host]
    model = RegTR(cfg)
    model.load_state_dict(seeded_weights.seeded_state_dict(cfg, 0, K015_CENTER))
    model = model.cuda().eval()
    counter = [0]

    def step():
        counter[0] += 1
        for p in model.parameters():
            p.grad = None
        _, losses = model.training_step(augment.modelnet_train_batch(dev[:4], cfg, seed, counter[0]), train_backbone=True)
        losses['total'].backward()

    lines = []
    host_ms = host_cloud_ms(host[:args.host_clouds], cfg, seed)
    for B in (4, 256):
        def chain():
            counter[0] += 1
            return augment.modelnet_train_batch(dev[:B], cfg, seed, counter[0])
        ms = sorted(median_ms(chain, args.reps, args.warmup) for _ in range(args.rounds))
        rec = {'clouds': B, 'points_per_cloud': 2048, 'out_rows_per_cloud': 717, 'reps': args.reps, 'rounds': args.rounds,
               'modelnet_train_batch_ms': round(ms[len(ms) // 2], 3), 'spread_ms': [round(ms[0], 3), round(ms[-1], 3)],
               'pairs_per_s': round(1e3 * B / ms[len(ms) // 2], 1), 'host_clouds_timed': args.host_clouds,
               'host_chain_ms_per_cloud': round(host_ms, 2), 'host_pairs_per_s_one_core': round(1e3 / host_ms, 1)}
        if B == 4:
            st = sorted(median_ms(step, args.reps, args.warmup) for _ in range(args.rounds))
            rec.update(training_step_with_input_ms=round(st[len(st) // 2], 3), training_step_spread_ms=[round(st[0], 3), round(st[-1], 3)],
                       share_of_step_percent=round(100 * ms[len(ms) // 2] / st[len(st) // 2], 2))
        lines.append(json.dumps(rec))
        print(lines[-1])
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
