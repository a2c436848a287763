"""Generates tests/golden/losses_<case>.npz by running the REAL reference RegTR.forward and RegTR.compute_loss (models/regtr.py:237-294)
on the CPU with the seeded weights of oracle.seeded_weights.  Runs where the reference tree is available, never on a GPU machine.
Re-run:  python tools/make_golden_losses.py

Cases (the input clouds are read from the forward goldens, not stored again)
  3dmatch_crop_b2 : the two ragged red-kitchen crop pairs of tests/golden/3dmatch_crop_b2.npz in ONE forward (B = 2)
  3dmatch_kitchen : the full red-kitchen pair of tests/golden/3dmatch_kitchen.npz, cloud_bin_0 -> cloud_bin_5
  modelnet_630    : demo.py example 4, tests/golden/modelnet_630.npz
GT poses: the kitchen pairs take entry 4 of datasets/3dmatch/test_3DMatch_info.pkl (cloud_bin_5 -> cloud_bin_0) inverted, since
cloud_bin_0 is the source here; the crops share it.  ModelNet takes a fixed rotation / translation.  GT masks come from the reference's
own compute_overlap on the GT-transformed source (threedmatch.py:78-84), through the open3d stand-in of oracle/make_golden_overlap.py.
feature_criterion*.W are overwritten with N(0, 0.1) (the reference's init, feature_loss.py:265-266): zero W makes every logit 0.  They
are drawn by loss_weights(shape, seed) from a seeded torch CPU generator, so the file stores the seed, not the matrices.

Stored per case (kept small: data only): pose, masks, `w_seed`, the reference's coarsest-level key points, correspondences and overlap
logits of the decoder layer the losses read (not its 256-d features: the tests take those from this project's parity-mode forward), its
losses with the stock torch.cdist (`ref_<key>`) and with torch.cdist(..., compute_mode='donot_use_mm_for_euclid_dist') patched in
(`exact_<key>`, exact distances), and `decision_rows`: the number of anchor rows whose InfoNCE decisions (argmin, r_p mask or r_n
ignore set) differ between the two cdist forms -- the size of the gap the stock values carry (0 of 206 / 410 / 531 rows here).
"""
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader, seeded_weights                 # noqa: E402
from oracle.make_golden_overlap import _open3d_stand_in      # noqa: E402
from regtr_amd.kernel_points import K015_CENTER              # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
REF_SRC = os.path.join(ref_loader.REF_ROOT, 'src')
LEVEL = 5


def _decision_rows(anc_xyz, pos_xyz, r_p, r_n):
    """Rows whose (argmin, mask, ignore row) differ between the matmul and the exact cdist forms."""
    d_mm = torch.cdist(anc_xyz, pos_xyz)
    d_ex = torch.cdist(anc_xyz, pos_xyz, compute_mode='donot_use_mm_for_euclid_dist')
    i_mm, i_ex = d_mm.argmin(-1), d_ex.argmin(-1)
    m_mm, m_ex = d_mm.min(-1).values < r_p, d_ex.min(-1).values < r_p
    g_mm, g_ex = d_mm < r_n, d_ex < r_n
    g_mm[torch.arange(len(i_mm)), i_mm] = False
    g_ex[torch.arange(len(i_ex)), i_ex] = False
    return int(((i_mm != i_ex) | (m_mm != m_ex) | (g_mm != g_ex).any(-1)).sum())


def loss_weights(shape, seed):
    """(feature_criterion.W, feature_criterion_un.W): N(0, 0.1) from torch's CPU generator seeded with `seed` (tests draw the same)."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen) * 0.1, torch.randn(shape, generator=gen) * 0.1


def run(name, cfg_name, pairs, pose, seed):
    sys.modules.update(_open3d_stand_in())
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    from utils.pointcloud import compute_overlap            # the reference's own module
    from utils.se3_numpy import se3_transform
    from utils.se3_torch import se3_transform_list

    cfg = ref_loader.load_cfg(cfg_name)
    model = ref_loader.build_model(cfg, 0)
    sd = seeded_weights.seeded_state_dict(cfg, 0, K015_CENTER)
    sd['feature_criterion.W'], sd['feature_criterion_un.W'] = loss_weights(tuple(sd['feature_criterion.W'].shape), seed)
    model.load_state_dict(sd, strict=True)
    B = len(pairs)
    masks = [compute_overlap(se3_transform(pose, s.astype(np.float64)), t, cfg.overlap_radius)[:2] for s, t in pairs]
    batch = {'src_xyz': [torch.from_numpy(s) for s, _ in pairs], 'tgt_xyz': [torch.from_numpy(t) for _, t in pairs],
             'pose': torch.from_numpy(np.stack([pose] * B).astype(np.float32)),
             'src_overlap': [torch.from_numpy(m[0]) for m in masks], 'tgt_overlap': [torch.from_numpy(m[1]) for m in masks]}
    with torch.no_grad():
        pred = model(batch)
        stock = model.compute_loss(pred, batch)
        cdist = torch.cdist
        torch.cdist = lambda a, b, **kw: cdist(a, b, compute_mode='donot_use_mm_for_euclid_dist')
        try:
            exact = model.compute_loss(pred, batch)
        finally:
            torch.cdist = cdist
    g = {'pose': np.stack([pose] * B).astype(np.float32), 'n_pairs': np.int64(B),
         'w_seed': np.int64(seed),
         'r_p': np.float64(cfg.r_p), 'r_n': np.float64(cfg.r_n)}
    for b in range(B):
        g[f'src_mask_{b}'], g[f'tgt_mask_{b}'] = masks[b][0], masks[b][1]
        for k in ('src_kp', 'tgt_kp'):
            g[f'{k}_{b}'] = pred[k][b].numpy()
        for k in ('src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
            g[f'{k}_{b}'] = pred[k][b][LEVEL].numpy()
    for k, v in stock.items():
        g[f'ref_{k}'] = np.float64(v)
    for k, v in exact.items():
        g[f'exact_{k}'] = np.float64(v)
    anc = se3_transform_list(batch['pose'], pred['src_kp'])
    g['decision_rows'] = np.int64(sum(_decision_rows(anc[b], pred['tgt_kp'][b], cfg.r_p, cfg.r_n) for b in range(B)))
    g['anchor_rows'] = np.int64(sum(int(x.shape[0]) for x in pred['src_kp']))
    np.savez_compressed(os.path.join(GOLD, f'losses_{name}.npz'), **g)
    print(name, {k: float(v) for k, v in stock.items()}, 'exact', {k: float(v) for k, v in exact.items()},
          'decision rows', int(g['decision_rows']), 'of', int(g['anchor_rows']))


def main():
    with open(os.path.join(REF_SRC, 'datasets', '3dmatch', 'test_3DMatch_info.pkl'), 'rb') as f:
        info = pickle.load(f)
    assert info['src'][4].endswith('7-scenes-redkitchen/cloud_bin_5.pth') and info['tgt'][4].endswith('cloud_bin_0.pth'), info['src'][4]
    T50 = np.eye(4)
    T50[:3, :3], T50[:3, 3] = info['rot'][4], np.asarray(info['trans'][4]).reshape(3)
    T05 = np.linalg.inv(T50)[:3]                       # cloud_bin_0 -> cloud_bin_5
    gold = lambda n: np.load(os.path.join(GOLD, f'{n}.npz'))
    b2 = gold('3dmatch_crop_b2')
    run('3dmatch_crop_b2', '3dmatch', [(b2['src_0'], b2['tgt_0']), (b2['src_1'], b2['tgt_1'])], T05, 11)
    k = gold('3dmatch_kitchen')
    run('3dmatch_kitchen', '3dmatch', [(k['src'], k['tgt'])], T05, 12)
    m = gold('modelnet_630')
    c, s_ = np.cos(0.3), np.sin(0.3)
    Tm = np.array([[c, -s_, 0, 0.05], [s_, c, 0, -0.02], [0, 0, 1, 0.01]])
    run('modelnet_630', 'modelnet', [(m['src'], m['tgt'])], Tm, 13)


if __name__ == '__main__':
    main()
