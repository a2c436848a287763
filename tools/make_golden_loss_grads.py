"""Generates tests/golden/loss_grads_<case>.npz by running the REAL reference InfoNCELossFull (models/losses/feature_loss.py:246-314)
and CorrCriterion (models/losses/corr_loss.py:9-40) forward + backward in float64 on the CPU.  Runs where the reference tree is
available, never on a GPU machine.  Re-run:  python tools/make_golden_loss_grads.py

Inputs per case (one per tests/golden/losses_<case>.npz, whose key points, GT poses and warped points are reused, not stored again):
  * anchors: the reference's coarsest-level src key points with the GT pose applied in float32, rounded per operation (what
    ops.se3_transform / the kernels' pose-on-load compute) -- stored (`anc_xyz_<b>`), a few KB; positives: the tgt key points;
  * features: N(0, 0.2) of width D from torch's CPU generator seeded with `feat_seed` (src clouds, then tgt clouds), and
    W = N(0, 0.1) (the reference's init) drawn after them -- seeds stored, not matrices;  D = 256 on the kitchen pair (the model's
    d_embed), 64 on the other two (kept small);
  * CorrCriterion: kp_before = src key points, kp_warped_pred = the reference's own layer-5 src correspondences of the loss golden,
    overlap_weights = U(0, 1) with every third weight 0, from the same generator after W.
The reference runs with torch.cdist patched to compute_mode='donot_use_mm_for_euclid_dist' (exact distances, the kernels' decisions);
`decision_rows` records how many anchor rows decide differently (argmin, r_p mask or r_n ignore set) under the stock matmul cdist.

Stored (float32 unless noted): `loss_feat`, `loss_corr` (float64), `dA_<b>`, `dG_<b>` (feature gradients), `dW`, `dwarped_<b>`, and
the reference modules' state_dict keys / shapes (`sd_infonce_keys`, `sd_infonce_shapes`, `sd_corr_keys`).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
REF_SRC = os.path.join(ref_loader.REF_ROOT, 'src')
CASES = [('3dmatch_crop_b2', 64, 21), ('3dmatch_kitchen', 256, 22), ('modelnet_630', 64, 23)]


def transform_f32(T, x):
    """((R0 x + R1 y) + R2 z) + t per row, float32 rounded per operation."""
    T = T.astype(np.float32)
    return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], 1).astype(np.float32)


def draw_inputs(n_src, n_tgt, D, seed):
    """(src features, tgt features, W, corr weights) as float32 tensors: the tests draw the same from the stored seed."""
    gen = torch.Generator().manual_seed(int(seed))
    src = [torch.randn((n, D), generator=gen) * 0.2 for n in n_src]
    tgt = [torch.randn((n, D), generator=gen) * 0.2 for n in n_tgt]
    W = torch.randn((D, D), generator=gen) * 0.1
    w = []
    for n in n_src:
        x = torch.rand(n, generator=gen)
        x[::3] = 0.0
        w.append(x)
    return src, tgt, W, w


def _decision_rows(anc_xyz, pos_xyz, r_p, r_n):
    d_mm = torch.cdist(anc_xyz, pos_xyz)
    d_ex = torch.cdist(anc_xyz, pos_xyz, compute_mode='donot_use_mm_for_euclid_dist')
    i_mm, i_ex = d_mm.argmin(-1), d_ex.argmin(-1)
    m_mm, m_ex = d_mm.min(-1).values < r_p, d_ex.min(-1).values < r_p
    g_mm, g_ex = d_mm < r_n, d_ex < r_n
    g_mm[torch.arange(len(i_mm)), i_mm] = False
    g_ex[torch.arange(len(i_ex)), i_ex] = False
    return int(((i_mm != i_ex) | (m_mm != m_ex) | (g_mm != g_ex).any(-1)).sum())


def run(case, D, seed):
    ref_loader.load()                                              # the reference tree, its unused heavy imports stubbed
    from models.losses.corr_loss import CorrCriterion             # the reference's own modules
    from models.losses.feature_loss import InfoNCELossFull

    lg = np.load(os.path.join(GOLD, f'losses_{case}.npz'))
    B = int(lg['n_pairs'])
    r_p, r_n = float(lg['r_p']), float(lg['r_n'])
    pose = lg['pose']
    src_kp = [lg[f'src_kp_{b}'] for b in range(B)]
    tgt_kp = [lg[f'tgt_kp_{b}'] for b in range(B)]
    warped = [lg[f'src_kp_warped_{b}'] for b in range(B)]
    anc = [transform_f32(pose[b], src_kp[b]) for b in range(B)]
    src, tgt, W, w = draw_inputs([len(x) for x in src_kp], [len(x) for x in tgt_kp], D, seed)

    crit = InfoNCELossFull(D, r_p=r_p, r_n=r_n).double()
    with torch.no_grad():
        crit.W.copy_(W.double())
    fs = [x.double().requires_grad_() for x in src]
    ft = [x.double().requires_grad_() for x in tgt]
    cdist = torch.cdist
    torch.cdist = lambda a, b, **kw: cdist(a, b, compute_mode='donot_use_mm_for_euclid_dist')
    try:
        loss_feat = crit(fs, ft, [torch.from_numpy(a).double() for a in anc], [torch.from_numpy(t).double() for t in tgt_kp])
    finally:
        torch.cdist = cdist
    loss_feat.backward()

    corr = CorrCriterion(metric='mae')
    wp = [torch.from_numpy(x).double().requires_grad_() for x in warped]
    loss_corr = corr([torch.from_numpy(x).double() for x in src_kp], wp, torch.from_numpy(pose).double(), [x.double() for x in w])
    loss_corr.backward()

    g = {'case': np.array(case), 'n_pairs': np.int64(B), 'D': np.int64(D), 'feat_seed': np.int64(seed), 'r_p': np.float64(r_p),
         'r_n': np.float64(r_n), 'loss_feat': np.float64(loss_feat.item()), 'loss_corr': np.float64(loss_corr.item()),
         'dW': crit.W.grad.float().numpy()}
    for b in range(B):
        g[f'anc_xyz_{b}'] = anc[b]
        g[f'dA_{b}'] = fs[b].grad.float().numpy()
        g[f'dG_{b}'] = ft[b].grad.float().numpy()
        g[f'dwarped_{b}'] = wp[b].grad.float().numpy()
    g['decision_rows'] = np.int64(sum(_decision_rows(torch.from_numpy(anc[b]).double(), torch.from_numpy(tgt_kp[b]).double(), r_p, r_n)
                                      for b in range(B)))
    sd = InfoNCELossFull(D, r_p=r_p, r_n=r_n).state_dict()
    g['sd_infonce_keys'] = np.array(list(sd.keys()))
    g['sd_infonce_shapes'] = np.array([list(v.shape) for v in sd.values()], dtype=np.int64)
    g['sd_corr_keys'] = np.array(list(CorrCriterion(metric='mae').state_dict().keys()), dtype='<U1')
    np.savez_compressed(os.path.join(GOLD, f'loss_grads_{case}.npz'), **g)
    print(case, f'D={D} feature {loss_feat.item():.6f} corr {loss_corr.item():.6f} decision rows {int(g["decision_rows"])}')


def main():
    for case, D, seed in CASES:
        run(case, D, seed)


if __name__ == '__main__':
    main()
