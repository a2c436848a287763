"""Generates tests/golden/head_grads_<case>.npz by running the REAL reference modules above the backbone forward + backward in float64
on the CPU: nn.Linear feat_proj (models/regtr.py:36,145), TransformerCrossEncoder (models/transformer/transformers.py:18-59),
CorrespondenceRegressor (regtr.py:399-443), nn.BCEWithLogitsLoss, InfoNCELossFull twice (models/losses/feature_loss.py:246-314),
CorrCriterion twice (models/losses/corr_loss.py:9-40) and the weighted total of regtr.py:292-293, wired as regtr.py:145-168 and :237-294
wire them, on clouds padded to (N_max, B, D) under key-padding masks.  Runs where the reference tree is available, never on a GPU
machine.  Re-run:  python tools/make_golden_head_grads.py

The cases, their seeded parameters and inputs are tests/head_grads_ref.py's (FULL_CASES / draw_full_case): the key points and GT pose of
tests/golden/losses_<case>.npz, the float32 anchors of tests/golden/loss_grads_<case>.npz, everything else from the case's seed (seeds
and shapes are stored, matrices are not).  Every loss sits on the last encoder layer; the encoder has its final norm and returns the
intermediate layers.  The reference runs with torch.cdist patched to compute_mode='donot_use_mm_for_euclid_dist' (exact distances); the
InfoNCE decisions depend on coordinates only, and `decision_rows` records how many anchor rows decide differently (argmin, r_p mask or
r_n ignore set) there than in the kernels' float32 distance arithmetic on the same float32 anchors (tests/loss_grads_ref.py: decisions).
`relu_margin` is the smallest |pre-activation| of any ReLU of the chain (tests/head_grads_ref.py: relu_margin, which says why a case
must keep it above RELU_MARGIN).

Stored (float64): `loss/<term>`; `corr`, `logit` and `d_feats_un` (every `row_step`-th token); every bias and LayerNorm gradient in full
and rows `w_rows` of every weight gradient (`g/<name>`, names as in RegTR's state_dict), both InfoNCE dW among them; the modules'
state_dict keys / shapes (`sd_keys`, `sd_shapes`).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                  # noqa: E402
from tests import head_grads_ref as HR                         # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
ROW_STEP = {'3dmatch_crop_b2': 3, '3dmatch_kitchen': 13}
W_ROWS = [0, 1, 31, 63]                                         # rows of every weight gradient that are stored (3- and 1-row weights: in full)


def _decision_rows(c):
    """Anchor rows whose decisions in float64 exact distances differ from the kernels' float32 arithmetic."""
    n = 0
    for b, (idx, mask, allowed) in enumerate(HR.decisions(c)):
        d = torch.cdist(torch.from_numpy(c['anc'][b]).double(), torch.from_numpy(c['tgt_kp'][b]).double(),
                        compute_mode='donot_use_mm_for_euclid_dist')
        i64 = d.argmin(-1)
        m64 = d.min(-1).values < c['r_p']
        a64 = ~(d < c['r_n'])
        a64[torch.arange(len(i64)), i64] = True
        n += int(((i64 != idx) | (m64 != mask) | (a64 != allowed).any(-1)).sum())
    return n


def run(name):
    ref = ref_loader.load()
    from models.losses.corr_loss import CorrCriterion             # the reference's own modules
    from models.losses.feature_loss import InfoNCELossFull
    T = ref.transformers
    c = HR.draw_full_case(name)
    D, B, L, wt = c['D'], c['B'], c['L'], c['wt']
    dbl = lambda sd: {k: v.double() for k, v in sd.items()}

    feat_proj = torch.nn.Linear(c['K'], D).double()
    feat_proj.load_state_dict(dbl(c['sd_proj']), strict=True)
    layer = T.TransformerCrossEncoderLayer(D, c['H'], c['F'], 0.0, activation='relu', normalize_before=True, sa_val_has_pos_emb=True,
                                           ca_val_has_pos_emb=True, attention_type='dot_prod')
    enc = T.TransformerCrossEncoder(layer, L, torch.nn.LayerNorm(D), return_intermediate=True).double()
    assert list(enc.state_dict()) == list(c['sd_enc']), 'the seeded state_dict does not have the reference encoder\'s keys'
    enc.load_state_dict(dbl(c['sd_enc']), strict=True)
    head = ref.regtr.CorrespondenceRegressor(D).double()
    assert list(head.state_dict()) == list(c['sd_head']), 'the seeded state_dict does not have the reference head\'s keys'
    head.load_state_dict(dbl(c['sd_head']), strict=True)
    crit, crit_un = InfoNCELossFull(D, r_p=c['r_p'], r_n=c['r_n']).double(), InfoNCELossFull(D, r_p=c['r_p'], r_n=c['r_n']).double()
    with torch.no_grad():
        crit.W.copy_(c['W'].double())
        crit_un.W.copy_(c['W_un'].double())
    corr_crit = CorrCriterion(metric='mae')
    overlap_crit = torch.nn.BCEWithLogitsLoss()

    seg = c['seg']
    lens = [int(seg[i + 1] - seg[i]) for i in range(2 * B)]
    cut = lambda t, i: t[int(seg[i]):int(seg[i + 1])]
    pad = torch.nn.utils.rnn.pad_sequence
    mask = lambda ls: torch.tensor([[j >= n for j in range(max(ls))] for n in ls])
    side = lambda t, lo: pad([cut(t, i) for i in range(lo, lo + B)])                    # (N_max, B, D)

    feats_un = c['feats_un'].double().requires_grad_()
    both = feat_proj(feats_un)                                                          # regtr.py:145
    pe = c['pe'].double() if c['pe'] is not None else None
    src_o, tgt_o = enc(side(both, 0), side(both, B), src_key_padding_mask=mask(lens[:B]), tgt_key_padding_mask=mask(lens[B:]),
                       src_pos=side(pe, 0) if pe is not None else None, tgt_pos=side(pe, B) if pe is not None else None)
    src_kp = [torch.from_numpy(x).double() for x in c['src_kp']]
    tgt_kp = [torch.from_numpy(x).double() for x in c['tgt_kp']]
    src_corr, tgt_corr, src_ov, tgt_ov = head(src_o, tgt_o, src_kp, tgt_kp)             # regtr.py:168: lists of (L, n, 3) / (L, n, 1)
    src_feat = [src_o[:, :lens[b], b] for b in range(B)]                                # (L, n, D) per pair
    tgt_feat = [tgt_o[:, :lens[B + b], b] for b in range(B)]

    i = L - 1
    gt = c['gt'].double()
    pose = torch.from_numpy(c['pose']).double()
    anc = [torch.from_numpy(a).double() for a in c['anc']]
    losses = {}
    losses['overlap'] = overlap_crit(torch.cat(src_ov + tgt_ov, dim=-2)[i, :, 0], gt)   # regtr.py:249-252
    cdist = torch.cdist
    torch.cdist = lambda a, b, **kw: cdist(a, b, compute_mode='donot_use_mm_for_euclid_dist')
    try:
        losses['feature'] = crit([s[i] for s in src_feat], [t[i] for t in tgt_feat], anc, tgt_kp)
        losses['feature_un'] = crit_un([cut(both, b) for b in range(B)], [cut(both, B + b) for b in range(B)], anc, tgt_kp)
    finally:
        torch.cdist = cdist
    gt_src, gt_tgt = [cut(gt, b) for b in range(B)], [cut(gt, B + b) for b in range(B)]
    pose44 = torch.cat([pose, torch.tensor([[[0.0, 0.0, 0.0, 1.0]]], dtype=torch.float64).expand(B, 1, 4)], 1)
    inv = torch.stack([ref.se3_torch.se3_inv(p) for p in pose44])
    losses['corr'] = (corr_crit(src_kp, [w[i] for w in src_corr], pose44, overlap_weights=gt_src) +
                      corr_crit(tgt_kp, [w[i] for w in tgt_corr], inv, overlap_weights=gt_tgt))       # regtr.py:268-281
    total = torch.sum(torch.stack([losses[k] * wt[k] for k in losses]))                  # regtr.py:292-293
    total.backward()

    step = ROW_STEP[name]
    mods = {'feat_proj': feat_proj, 'transformer_encoder': enc, 'correspondence_decoder': head, 'feature_criterion': crit,
            'feature_criterion_un': crit_un}
    corr = torch.cat([w[i] for w in src_corr] + [w[i] for w in tgt_corr]).detach()
    logit = torch.cat([o[i, :, 0] for o in src_ov] + [o[i, :, 0] for o in tgt_ov]).detach()
    g = {'case': np.array(name), 'seed': np.int64(c['seed']), 'D': np.int64(D), 'H': np.int64(c['H']), 'F': np.int64(c['F']),
         'L': np.int64(L), 'K': np.int64(c['K']), 'src_lens': np.array(c['src'], dtype=np.int64), 'tgt_lens': np.array(c['tgt'], dtype=np.int64),
         'row_step': np.int64(step), 'w_rows': np.array(W_ROWS, dtype=np.int64), 'decision_rows': np.int64(_decision_rows(c)),
         'relu_margin': np.float64(HR.relu_margin(c)),
         'corr': corr[::step].numpy(), 'logit': logit[::step].numpy(), 'd_feats_un': feats_un.grad[::step].numpy(),
         'loss/total': np.float64(total.item())}
    for k, v in losses.items():
        g['loss/' + k] = np.float64(v.item())
    keys, shapes = [], []
    for mk, m in mods.items():
        for k, v in m.state_dict().items():
            keys.append(f'{mk}.{k}')
            shapes.append(list(v.shape) + [0] * (2 - v.dim()))
        for k, p in m.named_parameters():
            g[f'g/{mk}.{k}'] = (p.grad if p.dim() == 1 or p.shape[0] <= 3 else p.grad[W_ROWS]).numpy()
    g['sd_keys'], g['sd_shapes'] = np.array(keys), np.array(shapes, dtype=np.int64)
    path = os.path.join(GOLD, f'head_grads_{name}.npz')
    np.savez_compressed(path, **g)
    print(name, ' '.join(f'{k} {v.item():.6f}' for k, v in losses.items()), f'total {total.item():.6f} decision rows '
          f'{int(g["decision_rows"])} relu margin {float(g["relu_margin"]):.2e} {os.path.getsize(path) / 1024:.0f} KB')


def main():
    for name in HR.FULL_CASES:
        run(name)


if __name__ == '__main__':
    main()
