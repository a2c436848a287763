"""Measures what encoding each cloud once is worth: the same pairs through RegTR.forward and through encode_clouds + register.
    python tools/shared_backbone_bench.py [--pairs 64] [--ratios 0.5 1 2 4] [--info test_3DMatch_info.pkl] [--points 20000]
                                          [--reps 15] [--out profiles/shared_backbone_bench.txt]
Workload: synthetic scenes (regtr_amd.synthetic.synth_fragments: rooms of 8 fragments sized like 3DMatch fragments), `--pairs` pairs per
call.  A RATIO is pairs per distinct fragment: 0.5 = every cloud appears once (nothing to share), 4 = every fragment in eight pair
slots.  --info: the ratio of that info pickle (pairs / distinct src + tgt paths) is measured as well; without it the ratios are the
stated ones -- the 3DMatch / 3DLoMatch lists are 1623 / 1781 pairs over a few hundred fragments, i.e. around 4.
Per ratio, the same pairs go
  * through forward, all `--pairs` pairs in one call (the yardstick, measured in the same run: forward is not changed by this work);
  * through ONE encode_clouds over the pairs' distinct fragments + ONE register of all pairs (a cold bank: every fragment is encoded
    in the window that first reads it; a bank that lives across windows pays encode_clouds only for fragments it has not seen).
Timed apart: encode_clouds, register, and the regtr_gather_segments launch alone (with its bytes/s: rows x (2 D + 3) floats read and
written once each) -- once over the same arrays launch after launch (they fit the 256 MB Infinity Cache: a warm figure), once ROTATING
over four copies of the bank and of the outputs (~0.9 GB, so no launch finds its rows cached: the cold figure), and next to it the
yardstick: torch's device-to-device copy_ of the same number of bytes over the same rotation.
A sample is one call (the gather and the copy: `--inner` launches) between two device events; `--reps` samples per route after three
warm-up calls, the routes taking turns; reported: the median and min .. max.  No speed-up is assumed: the result line says
whether the shared path is faster than forward beyond the two spreads, and the crossover is the lowest measured ratio at which it is."""
import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENE_FRAGMENTS = 8


def sample_ms(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(routes, reps, inner=None):
    inner = inner or {}
    for f in routes.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    samples = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            samples[k].append(sample_ms(f, inner.get(k, 1)))
    out = {}
    for k, s in samples.items():
        s = sorted(s)
        out[k] = {'median': round(s[len(s) // 2], 4), 'min': round(s[0], 4), 'max': round(s[-1], 4)}
    return out


def window(n_pairs, ratio):
    """(number of fragments, [(a, b)]): n_pairs pairs over round(n_pairs / ratio) fragments, every fragment read, partners from one scene."""
    n_frag = max(2, min(2 * n_pairs, int(round(n_pairs / ratio))))
    n_frag += n_frag % 2
    pairs = []
    for k in range(n_pairs):
        a = k % n_frag
        base = a // SCENE_FRAGMENTS * SCENE_FRAGMENTS
        size = min(SCENE_FRAGMENTS, n_frag - base)
        if ratio <= 0.5:
            a, size, base = 2 * k % n_frag, 2, 2 * k % n_frag          # every fragment once: (0, 1), (2, 3), ...
        b = base + (a - base + 1 + (k // n_frag) % max(size - 1, 1)) % size
        pairs.append((a, b))
    return n_frag, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--ratios', type=float, nargs='+', default=[0.5, 1.0, 2.0, 4.0])
    ap.add_argument('--info', type=str, default=None, help='a 3DMatch-style info pickle: its pairs / distinct fragments is measured too')
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20, help='gather launches per sample')
    ap.add_argument('--out', type=str, default=os.path.join('profiles', 'shared_backbone_bench.txt'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/shared_backbone_bench.py needs an MI355X (HIP) device')
    from regtr_amd import RegTR, load_config, ops
    from regtr_amd.cloud_bank import upload_tables
    from regtr_amd.synthetic import synth_fragments
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, 'regtr_amd', 'conf', '3dmatch.yaml'))
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = RegTR(cfg).to(dev).eval()
    ratios = [(r, 'stated') for r in opt.ratios]
    if opt.info:
        with open(opt.info, 'rb') as f:
            infos = pickle.load(f)
        ratios.append((len(infos['src']) / len(set(infos['src']) | set(infos['tgt'])), os.path.basename(opt.info)))
    need = max(window(opt.pairs, r)[0] for r, _ in ratios)
    frags = []
    for s in range(-(-need // SCENE_FRAGMENTS)):
        frags += [torch.from_numpy(f).to(dev) for f in synth_fragments(s, SCENE_FRAGMENTS, opt.points)[0]]
    lines, crossover = [], None
    for ratio, origin in sorted(ratios):
        n_frag, pairs = window(opt.pairs, ratio)
        src, tgt = [p[0] for p in pairs], [p[1] for p in pairs]
        used = sorted(set(src) | set(tgt))
        at = {f: i for i, f in enumerate(used)}
        clouds = [frags[f] for f in used]
        si, ti = [at[f] for f in src], [at[f] for f in tgt]
        bank = model.encode_clouds(clouds)
        seg, cloud_of, n_out, max_len = upload_tables(bank.lens, si + ti, dev)

        def forward():
            return model({'src_xyz': [frags[f] for f in src], 'tgt_xyz': [frags[f] for f in tgt]})

        def encode():
            return model.encode_clouds(clouds)

        def register():
            return model.register(bank, si, ti)

        def shared():
            return model.register(model.encode_clouds(clouds), si, ti)

        def gather():
            return ops.gather_segments(bank.feats, bank.seg_off, cloud_of, seg, n_out, max_len, pe=bank.pe, xyz=bank.xyz)
        D = bank.feats.shape[1]
        moved = 2 * n_out * ((2 if bank.pe is not None else 1) * D + 3) * 4
        ROT = 4
        clone = lambda t: None if t is None else t.clone()
        new = lambda t, w: None if t is None else torch.empty((n_out, w), dtype=torch.float32, device=dev)
        rot_in = [(clone(bank.feats), clone(bank.pe), clone(bank.xyz)) for _ in range(ROT)]
        rot_out = [(new(bank.feats, D), new(bank.pe, D), new(bank.xyz, 3)) for _ in range(ROT)]
        flat_in = [torch.empty(moved // 8, dtype=torch.float32, device=dev).normal_() for _ in range(ROT)]
        flat_out = [torch.empty(moved // 8, dtype=torch.float32, device=dev) for _ in range(ROT)]
        turn = [0, 0]

        def gather_cold():
            k = turn[0] = (turn[0] + 1) % ROT
            return ops.gather_segments(rot_in[k][0], bank.seg_off, cloud_of, seg, n_out, max_len, pe=rot_in[k][1], xyz=rot_in[k][2], out=rot_out[k])

        def copy_cold():
            k = turn[1] = (turn[1] + 1) % ROT
            return flat_out[k].copy_(flat_in[k])
        ms = measure({'forward': forward, 'encode_clouds': encode, 'register': register, 'encode+register': shared, 'gather_segments': gather,
                      'gather_segments_rotating': gather_cold, 'torch_copy_rotating': copy_cold},
                     opt.reps, {'gather_segments': opt.inner, 'gather_segments_rotating': opt.inner, 'torch_copy_rotating': opt.inner})
        for k in range(ROT):          # the rotating launches wrote what the plain one writes
            assert torch.equal(rot_out[k][0], gather()[0])
        fw, sh = ms['forward'], ms['encode+register']
        faster = sh['max'] < fw['min']
        slower = sh['min'] > fw['max']
        res = {'pairs': opt.pairs, 'pairs_per_fragment': round(ratio, 3), 'ratio_from': origin, 'fragments_encoded': len(used),
               'pair_slots': 2 * opt.pairs, 'points_per_fragment': int(np.mean([int(c.shape[0]) for c in clouds])), 'tokens': n_out,
               'samples': opt.reps, 'ms': ms, 'gather_bytes': moved,
               'gather_GBps': {k: round(moved / (ms['gather_segments'][j] * 1e-3) / 1e9, 1) for k, j in (('median', 'median'), ('best', 'min'), ('worst', 'max'))},
               'gather_rotating_GBps': round(moved / (ms['gather_segments_rotating']['median'] * 1e-3) / 1e9, 1),
               'torch_copy_rotating_GBps': round(moved / (ms['torch_copy_rotating']['median'] * 1e-3) / 1e9, 1),
               'forward_over_shared': round(fw['median'] / sh['median'], 3),
               'verdict': 'shared faster beyond both spreads' if faster else ('shared SLOWER beyond both spreads' if slower else 'within the spreads'),
               'f16_range_fallbacks': model.f16_range_fallbacks}
        if faster and crossover is None:
            crossover = ratio
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del bank, rot_in, rot_out, flat_in, flat_out
    tail = (f'crossover: the shared path is faster than forward beyond both spreads from {crossover:.3g} pairs per fragment on (lowest measured '
            f'ratio where it is; measured ratios: {[round(r, 3) for r, _ in sorted(ratios)]})' if crossover is not None else
            'crossover: at no measured ratio was the shared path faster than forward beyond both spreads')
    print(tail)
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        f.write('tools/shared_backbone_bench.py: one call between two device events (gather_segments: consecutive launches); median and '
                'min .. max over the samples, ms; forward = the same pairs in one RegTR.forward, measured in this run\n')
        f.write('\n'.join(lines) + '\n' + tail + '\n')


if __name__ == '__main__':
    main()
