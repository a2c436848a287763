"""Generates tests/golden/backbone_grads_crop_b2.npz by running the REAL reference KPFEncoder (models/backbone_kpconv/kpconv.py:22-88 with
the blocks of kpconv_blocks.py) forward + backward in float64 on the CPU, on the tables of the reference's own CPU Preprocessor.  Runs
where the reference tree is available, never on a GPU machine.  Re-run:  python tools/make_golden_backbone_grads.py

The batch is the two-pair crop of tests/golden/3dmatch_crop_b2.npz CUT DOWN: of each of its four clouds the N_KEEP points nearest to the
point nearest its centroid.  Why cut down: a float32 forward can take the other LeakyReLU side or pool winner on a near-tie, and a weight
gradient cannot mask one element out, so the stored run must have NO near-tie: every LeakyReLU argument at least MARGIN = 2^-19 from
zero, every pool winner leading its runner-up by at least MARGIN, every convolution input row sum (KPConv's neighbour count) at least
MARGIN from zero.  With tens of millions of activations (the full crop: 20 407 points) some always sit closer; the generator walks the
cloud sizes of N_KEEPS downward and, per size, the weight seeds of oracle/seeded_weights.py upward from SEED0, and keeps the first
(size, seed) that qualifies.  The margin is stored and asserted.

Stored (data only): the four cut clouds, the seed, the level sizes, the margin; per LeakyReLU call its bit-packed side mask
(`mask_<block>_<call>`), per max-pool its winning columns as int8 (`winner_<block>`, -1: the shadow row); per parameter max |grad|
(`m/<name>`) and 2048 sampled gradient entries (`g/<name>`, float32; all of them where the parameter has fewer) with their flat
indices (`i/<name>`, int32, drawn by tests/backbone_grads_ref.py sample_indices; 2048 and not 4096 entries: with the indices stored
the larger sample would take the file past the size limit for a committed file); every `row_step`-th row of the output; the seed of d_out (tests/backbone_grads_ref.py:
golden_d_out).    python tools/make_golden_backbone_grads.py --n-keep 700 --seed 28    skips the search and re-checks that pair.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader, seeded_weights                  # noqa: E402
from regtr_amd.kernel_points import K015_CENTER                # noqa: E402
from tests import backbone_grads_ref as BR                     # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
MARGIN = 2.0 ** -19
SEED0, N_SEEDS = 0, 65
N_KEEPS = (1500, 1000, 700, 500, 350, 250)
ROW_STEP = 5


def cut(cloud, n):
    c = cloud[np.argmin(((cloud - cloud.mean(0)) ** 2).sum(1))]
    keep = np.sort(np.argsort(((cloud - c) ** 2).sum(1), kind='stable')[:n])
    return np.ascontiguousarray(cloud[keep])


def run(ref, cfg, clouds, seed):
    model = ref_loader.build_model(cfg, 0)
    model.load_state_dict(seeded_weights.seeded_state_dict(cfg, seed, K015_CENTER), strict=True)
    with torch.no_grad():
        meta = model.preprocessor([torch.from_numpy(c) for c in clouds])
    enc = model.kpf_encoder.double()
    meta = dict(meta, points=[p.double() for p in meta['points']])
    rec = {'margin': float('inf'), 'masks': {}, 'winners': {}}
    owner = {}
    for i, blk in enumerate(enc.encoder_blocks):
        for m in blk.modules():
            if isinstance(m, torch.nn.LeakyReLU):
                owner[m] = i

    def on_lrelu(m, inp):
        z = inp[0].detach()
        rec['margin'] = min(rec['margin'], float(z.abs().min()))
        rec['masks'].setdefault(owner[m], []).append((z > 0).numpy())

    def on_conv(m, inp):
        x = inp[3].detach()
        rec['margin'] = min(rec['margin'], float(x.sum(1).abs().min()))
    hooks = [m.register_forward_pre_hook(on_lrelu) for m in owner]
    hooks += [blk.KPConv.register_forward_pre_hook(on_conv) for blk in enc.encoder_blocks]
    real_pool = ref.kpconv_blocks.max_pool
    state = {'block': None}

    def pool(x, inds):
        ns = x.shape[0]
        vals = torch.cat((x.detach(), torch.zeros_like(x[:1])), 0)[inds]         # (Nq, width, C)
        col = vals.argmax(1)
        win = torch.where(torch.gather(inds[:, :, None].expand(-1, -1, x.shape[1]), 1, col[:, None, :])[:, 0] < ns, col, -1)
        if inds.shape[1] > 1:
            shadow = inds >= ns
            dup = (shadow & (shadow.cumsum(1) > 1))[:, :, None]
            top = torch.where(dup, torch.full_like(vals, -float('inf')), vals).topk(2, dim=1).values
            rec['margin'] = min(rec['margin'], float((top[:, 0] - top[:, 1]).min()))
        rec['winners'][state['block']] = win.numpy().astype(np.int8)
        return real_pool(x, inds)
    ref.kpconv_blocks.max_pool = pool
    pre = [blk.register_forward_pre_hook(lambda m, inp, i=i: state.update(block=i)) for i, blk in enumerate(enc.encoder_blocks)]
    try:
        x = torch.ones((meta['points'][0].shape[0], 1), dtype=torch.float64)
        out, _ = enc(x, meta)
        d_out = BR.golden_d_out(tuple(out.shape))
        (out * torch.from_numpy(d_out).double()).sum().backward()
    finally:
        ref.kpconv_blocks.max_pool = real_pool
        for h in hooks + pre:
            h.remove()
    return enc, meta, out.detach(), rec


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-keep', type=int, default=None, help='only this cloud size (skip the walk down the sizes)')
    ap.add_argument('--seed', type=int, default=None, help='only this weight seed (skip the walk up the seeds)')
    args = ap.parse_args()
    ref = ref_loader.load()
    cfg = ref_loader.load_cfg('3dmatch')
    f = np.load(os.path.join(GOLD, '3dmatch_crop_b2.npz'))
    full = [f['src_0'], f['src_1'], f['tgt_0'], f['tgt_1']]                    # src clouds, then tgt clouds: RegTR's batch order
    found = None
    for n_keep in (N_KEEPS if args.n_keep is None else (args.n_keep,)):
        clouds = [cut(c, n_keep) for c in full]
        best = 0.0
        for seed in (range(SEED0, SEED0 + N_SEEDS) if args.seed is None else (args.seed,)):
            enc, meta, out, rec = run(ref, cfg, clouds, seed)
            best = max(best, rec['margin'])
            if rec['margin'] >= MARGIN:
                found = (n_keep, seed, clouds, enc, meta, out, rec)
                break
        print(f'{n_keep} points per cloud: levels {[int(p.shape[0]) for p in meta["points"]]}, best margin over the seeds tried '
              f'{best:.3e} (need {MARGIN:.3e})' + (f' -> seed {found[1]}' if found else ''))
        if found:
            break
    assert found, 'no (size, seed) qualifies'
    n_keep, seed, clouds, enc, meta, out, rec = found
    assert all(int(l) >= 2 for s in meta['stack_lengths'] for l in s)
    g = {'seed': np.int64(seed), 'n_keep': np.int64(n_keep), 'n_clouds': np.int64(len(clouds)), 'margin': np.float64(rec['margin']),
         'level_sizes': np.array([int(p.shape[0]) for p in meta['points']], dtype=np.int64), 'row_step': np.int64(ROW_STEP),
         'out': out[::ROW_STEP].numpy().astype(np.float32), 'index_seed': np.int64(BR.INDEX_SEED), 'd_out_seed': np.int64(BR.D_OUT_SEED),
         'pool_widths': np.array([int(p.shape[1]) for p in meta['pools']], dtype=np.int64)}
    for i, c in enumerate(clouds):
        g[f'cloud_{i}'] = c
    n_masks = 0
    for i, masks in rec['masks'].items():
        for j, m in enumerate(masks):
            g[f'mask_{i}_{j}'] = np.packbits(m.reshape(-1))
            n_masks += 1
    g['n_masks'] = np.int64(n_masks)
    for i, w in rec['winners'].items():
        g[f'winner_{i}'] = w
    for pi, (k, p) in enumerate((k, p) for k, p in enc.named_parameters() if p.requires_grad):
        grad = p.grad.numpy().reshape(-1)
        idx = BR.sample_indices(pi, grad.size)
        g['m/' + k] = np.float64(np.abs(grad).max())
        g['g/' + k] = grad[idx].astype(np.float32)
        g['i/' + k] = idx.astype(np.int32)
    path = os.path.join(GOLD, 'backbone_grads_crop_b2.npz')
    np.savez_compressed(path, **g)
    print(f'seed {seed}, {n_keep} points per cloud, margin {rec["margin"]:.3e}, {n_masks} masks, {len(rec["winners"])} pools, '
          f'{os.path.getsize(path) / 1024:.0f} KB')


if __name__ == '__main__':
    main()
