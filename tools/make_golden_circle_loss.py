"""Generates tests/golden/circle_loss_<case>.npz by running the REAL reference CircleLossFull (models/losses/feature_loss.py:160-243,
dist_type 'euclidean') forward + backward in float64 on the CPU.  Runs where the reference tree is available, never on a GPU machine.
Re-run:  python tools/make_golden_circle_loss.py

Inputs per case (the three of tests/golden/losses_<case>.npz, whose key points are reused, not stored again):
  * anchors: `anc_xyz_<b>` of tests/golden/loss_grads_<case>.npz (the src key points with the GT pose applied in float32, rounded per
    operation); positives: the tgt key points;
  * features of width D (256 on the kitchen pair, 64 on the other two) from torch's CPU generator seeded with `feat_seed` -- the seed
    is stored, not the matrices: unit directions scaled by s / sqrt(2) with s ~ U(0.3, 1.3), so that the feature distances (0.26 to
    1.52) lie about both margins (N(0, 0.2) features are all ~2.3 apart: no negative would carry a gradient); six anchors per pair
    are then copied onto their nearest positive with 1e-3 noise, so some positives sit below pos_margin.
The reference runs with torch.cdist patched to compute_mode='donot_use_mm_for_euclid_dist' (exact coordinate distances);
`decision_pairs` records how many (i, j) classify differently (inside r_p / outside r_n) under the stock matmul cdist, and
`decision_pairs_f32` how many do under the kernels' float32 arithmetic (0: the float64 restatement with float32 decisions reproduces
the golden to its last digits).

Stored: `loss` (float64), `pair_loss` (B,), `dA_<b>` / `dG_<b>` (float32), `n_rows` / `n_cols` (selected per pair), `d_min` / `d_max`,
`pos_active` / `neg_active` (entries with a non-zero weight), the reference module's state_dict keys (none).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
CASES = [('3dmatch_crop_b2', 64, 31), ('3dmatch_kitchen', 256, 32), ('modelnet_630', 64, 33)]


def draw_features(n_src, n_tgt, D, seed, anc_xyz, tgt_xyz):
    """(src features, tgt features) as float32 tensors: the tests draw the same from the stored seed (tests/circle_loss_ref.py)."""
    gen = torch.Generator().manual_seed(int(seed))

    def cloud(n):
        v = torch.randn((n, D), generator=gen)
        v = v / v.norm(dim=1, keepdim=True)
        s = torch.rand(n, generator=gen) * 1.0 + 0.3
        return v * (s / np.sqrt(2.0)).unsqueeze(1).float()
    src = [cloud(n) for n in n_src]
    tgt = [cloud(n) for n in n_tgt]
    for b, n in enumerate(n_src):
        idx = np.arange(0, n, max(n // 6, 1))[:6]
        cd = np.linalg.norm(anc_xyz[b][idx].astype(np.float64)[:, None] - tgt_xyz[b].astype(np.float64)[None], axis=-1)
        near = cd.argmin(1)
        noise = torch.randn((len(idx), D), generator=gen) * 1e-3
        src[b][torch.from_numpy(idx)] = tgt[b][torch.from_numpy(near)] + noise
    return src, tgt


def _dist_f32(a, p):
    d = a[:, None, :].astype(np.float32) - p[None, :, :].astype(np.float32)
    sq = d * d
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(np.float32)


def run(case, D, seed):
    ref_loader.load()                                              # the reference tree, its unused heavy imports stubbed
    from models.losses.feature_loss import CircleLossFull         # the reference's own module

    lg = np.load(os.path.join(GOLD, f'losses_{case}.npz'))
    gg = np.load(os.path.join(GOLD, f'loss_grads_{case}.npz'))
    B = int(lg['n_pairs'])
    r_p, r_n = float(lg['r_p']), float(lg['r_n'])
    tgt_kp = [lg[f'tgt_kp_{b}'] for b in range(B)]
    anc = [gg[f'anc_xyz_{b}'] for b in range(B)]
    src, tgt = draw_features([len(x) for x in anc], [len(x) for x in tgt_kp], D, seed, anc, tgt_kp)

    crit = CircleLossFull(dist_type='euclidean', r_p=r_p, r_n=r_n)
    fs = [x.double().requires_grad_() for x in src]
    ft = [x.double().requires_grad_() for x in tgt]
    ax = [torch.from_numpy(a).double() for a in anc]
    px = [torch.from_numpy(t).double() for t in tgt_kp]
    cdist = torch.cdist
    torch.cdist = lambda a, b, **kw: cdist(a, b, compute_mode='donot_use_mm_for_euclid_dist')
    try:
        loss = crit(fs, ft, ax, px)
        with torch.no_grad():
            pair_loss = [float(crit([fs[b]], [ft[b]], [ax[b]], [px[b]])) for b in range(B)]
    finally:
        torch.cdist = cdist
    loss.backward()

    n_rows, n_cols, diff_mm, diff_f32, d_min, d_max, pa, na = [], [], 0, 0, np.inf, 0.0, 0, 0
    for b in range(B):
        d_ex = cdist(ax[b], px[b], compute_mode='donot_use_mm_for_euclid_dist')
        d_mm = cdist(ax[b], px[b])
        d32 = _dist_f32(anc[b], tgt_kp[b])
        pos, neg = d_ex < r_p, d_ex > r_n
        diff_mm += int(((pos != (d_mm < r_p)) | (neg != (d_mm > r_n))).sum())
        diff_f32 += int(((pos.numpy() != (d32 < np.float32(r_p))) | (neg.numpy() != (d32 > np.float32(r_n)))).sum())
        n_rows.append(int((pos.any(1) & neg.any(1)).sum()))
        n_cols.append(int((pos.any(0) & neg.any(0)).sum()))
        fd = torch.cdist(fs[b].detach(), ft[b].detach(), compute_mode='donot_use_mm_for_euclid_dist')
        d_min, d_max = min(d_min, float(fd.min())), max(d_max, float(fd.max()))
        pa += int((pos & (fd > crit.pos_optimal)).sum())
        na += int((neg & (fd < crit.neg_optimal)).sum())

    g = {'case': np.array(case), 'n_pairs': np.int64(B), 'D': np.int64(D), 'feat_seed': np.int64(seed), 'r_p': np.float64(r_p),
         'r_n': np.float64(r_n), 'loss': np.float64(loss.item()), 'pair_loss': np.array(pair_loss, dtype=np.float64),
         'n_rows': np.array(n_rows, dtype=np.int64), 'n_cols': np.array(n_cols, dtype=np.int64),
         'decision_pairs': np.int64(diff_mm), 'decision_pairs_f32': np.int64(diff_f32), 'd_min': np.float64(d_min),
         'd_max': np.float64(d_max), 'pos_active': np.int64(pa), 'neg_active': np.int64(na),
         'sd_circle_keys': np.array(list(crit.state_dict().keys()), dtype='<U1')}
    for b in range(B):
        g[f'dA_{b}'] = fs[b].grad.float().numpy()
        g[f'dG_{b}'] = ft[b].grad.float().numpy()
    np.savez_compressed(os.path.join(GOLD, f'circle_loss_{case}.npz'), **g)
    print(case, f'D={D} loss {loss.item():.16g} rows {n_rows} cols {n_cols} d in [{d_min:.3f}, {d_max:.3f}] active pos {pa} neg {na} '
                f'decisions differing: matmul cdist {diff_mm}, float32 {diff_f32}')


def main():
    for case, D, seed in CASES:
        run(case, D, seed)


if __name__ == '__main__':
    main()
