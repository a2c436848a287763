"""Generates the goldens of the learned positional embedding (pos_emb_type: learned) by running the REAL reference on the CPU.  Runs
where the reference tree is available, never on a GPU machine.  Re-run:  python tools/make_golden_learned_posemb.py

(a) tests/golden/learned_posemb_<case>.npz, case in modelnet_demo, 3dmatch_crop_b2: the reference RegTR (models/regtr.py:22-235) with
    pos_emb_type 'learned' -- its PositionEmbeddingLearned (models/transformer/position_embedding.py:53-72) -- on the clouds of
    tests/golden/<case>.npz (read from there, not stored again).  Weights: oracle.seeded_weights.seeded_state_dict of the config plus
    tests/posemb_mlp_ref.draw_mlp(d_embed, MODEL_SEED) as pos_embed.mlp.*, inserted at the reference's key position
    (posemb_mlp_ref.learned_state_dict), asserted against the model's own keys and loaded strictly.  Stored: what oracle/make_golden.py's
    run_case / run_batch_case store of the outputs (pose, key points, correspondences, overlap logits, level sizes, the coarsest points
    and neighbour table), the reference's state_dict key list (`sd_keys`), and every `pe_step`-th row of the reference module's output on
    the key points in float64 (`pe_rows`; `mlp_seed`, `d_model`).
(b) tests/golden/head_grads_learned_3dmatch_crop_b2.npz: the reference modules above the backbone forward + backward in float64, as
    tools/make_golden_head_grads.py runs them, on posemb_mlp_ref.draw_stack_case() (452 tokens, D = 64) with pe = the reference
    PositionEmbeddingLearned(3, D) of the key points INSIDE autograd.  Stored as there: the losses, `corr` / `logit` / `d_feats_un` rows,
    every bias and LayerNorm gradient in full and rows `w_rows` of every weight gradient, the ten pos_embed.mlp.* among them.
    The case's seed is the first at or after STACK_NOMINAL_SEED whose smallest ReLU |pre-activation| -- over the MLP's four ReLUs, the
    encoder's linear1 and the head's two, in float64 -- is at least RELU_MARGIN; this tool searches it, asserts that
    posemb_mlp_ref.STACK_SEED names it, and stores the margin (`relu_margin`).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader, seeded_weights                  # noqa: E402
from regtr_amd.kernel_points import K015_CENTER                # noqa: E402
from tests import head_grads_ref as HR                         # noqa: E402
from tests import posemb_mlp_ref as PR                         # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
PE_STEP = 19
ROW_STEP = 3
W_ROWS = [0, 1, 31, 63]                                         # as tools/make_golden_head_grads.py (weights of fewer than 64 rows: in full)


def _model(cfg_name):
    cfg = ref_loader.load_cfg(cfg_name)
    cfg['pos_emb_type'] = 'learned'
    model = ref_loader.build_model(cfg, 0)
    sd = PR.learned_state_dict(seeded_weights.seeded_state_dict(cfg, 0, K015_CENTER), cfg.d_embed)
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(sd.keys()), 'state_dict names differ from the reference'
    for k in sd:
        assert tuple(ref_sd[k].shape) == tuple(sd[k].shape), k
    model.load_state_dict(sd, strict=True)
    return cfg, model


def _pe_rows(model, cfg, kp):
    """The reference module's float64 output on the key points, every PE_STEP-th row."""
    ref = ref_loader.load()
    m = ref.position_embedding.PositionEmbeddingLearned(3, cfg.d_embed).double()
    m.load_state_dict({k: v.double() for k, v in model.pos_embed.state_dict().items()}, strict=True)
    with torch.no_grad():
        return m(torch.from_numpy(kp).double())[::PE_STEP].numpy()


def run_model_cases():
    # one pair (oracle/make_golden.py: run_case)
    name = 'modelnet_demo'
    src = np.load(os.path.join(GOLD, f'{name}.npz'))
    cfg, model = _model('modelnet')
    batch = {'src_xyz': [torch.from_numpy(src['src'])], 'tgt_xyz': [torch.from_numpy(src['tgt'])]}
    with torch.no_grad():
        out = model(batch)
    meta = batch['kpconv_meta']
    g = {'pose': out['pose'].numpy(), 'sd_keys': np.array(list(model.state_dict().keys())), 'mlp_seed': np.int64(PR.MODEL_SEED),
         'd_model': np.int64(cfg.d_embed), 'pe_step': np.int64(PE_STEP)}
    for k in ('src_kp', 'tgt_kp', 'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
        g[k] = out[k][0].numpy()
    for l, (p, s) in enumerate(zip(meta['points'], meta['stack_lengths'])):
        g[f'lens_{l}'] = s.numpy().astype(np.int32)
    g['points_last'] = meta['points'][-1].numpy()
    g['neighbors_last'] = meta['neighbors'][-1].numpy().astype(np.int32)
    g['pe_rows'] = _pe_rows(model, cfg, meta['points'][-1].numpy())
    path = os.path.join(GOLD, f'learned_posemb_{name}.npz')
    np.savez_compressed(path, **g)
    print(name, 'pose[-1]\n', g['pose'][-1, 0], f'{os.path.getsize(path) / 1024:.0f} KB')

    # two ragged pairs in one forward (run_batch_case)
    name = '3dmatch_crop_b2'
    src = np.load(os.path.join(GOLD, f'{name}.npz'))
    cfg, model = _model('3dmatch')
    B = 2
    batch = {'src_xyz': [torch.from_numpy(src[f'src_{b}']) for b in range(B)], 'tgt_xyz': [torch.from_numpy(src[f'tgt_{b}']) for b in range(B)]}
    with torch.no_grad():
        out = model(batch)
    meta = batch['kpconv_meta']
    g = {'pose': out['pose'].numpy(), 'sd_keys': np.array(list(model.state_dict().keys())), 'mlp_seed': np.int64(PR.MODEL_SEED),
         'd_model': np.int64(cfg.d_embed), 'pe_step': np.int64(PE_STEP)}
    for b in range(B):
        for k in ('src_kp', 'tgt_kp', 'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
            g[f'{k}_{b}'] = out[k][b].numpy()
    for l, s in enumerate(meta['stack_lengths']):
        g[f'lens_{l}'] = s.numpy().astype(np.int32)
    g['points_last'] = meta['points'][-1].numpy()
    g['neighbors_last'] = meta['neighbors'][-1].numpy().astype(np.int32)
    g['pe_rows'] = _pe_rows(model, cfg, meta['points'][-1].numpy())
    path = os.path.join(GOLD, f'learned_posemb_{name}.npz')
    np.savez_compressed(path, **g)
    print(name, 'pose', g['pose'].shape, [s.tolist() for s in meta['stack_lengths']], f'{os.path.getsize(path) / 1024:.0f} KB')


def find_stack_seed():
    seed = PR.STACK_NOMINAL_SEED
    while True:
        c = PR.draw_stack_case(seed)
        m = PR.stack_relu_margin(c)
        print(f'stack case seed {seed}: relu margin {m:.2e} (MLP alone {PR.relu_margin(c["sd_pos"], c["xyz"].numpy()):.2e})')
        if m >= PR.RELU_MARGIN:
            return seed, c, m
        seed += 1


def run_stack_case():
    ref = ref_loader.load()
    from models.losses.corr_loss import CorrCriterion             # the reference's own modules
    from models.losses.feature_loss import InfoNCELossFull
    T = ref.transformers
    seed, c, margin = find_stack_seed()
    assert seed == PR.STACK_SEED, f'tests/posemb_mlp_ref.py: STACK_SEED must be {seed}'
    # no ReLU of the MLP takes another side in float32 than in float64 on these key points
    pe32, hs32 = PR.torch_fwd(c['sd_pos'], c['xyz'].float())
    r64 = PR.forward(c['sd_pos'], c['xyz'].numpy())
    assert all(np.array_equal(hs32[l].numpy() > 0, r64['h'][l] > 0) for l in range(4))
    D, B, L, wt = c['D'], c['B'], c['L'], c['wt']
    dbl = lambda sd: {k: v.double() for k, v in sd.items()}

    feat_proj = torch.nn.Linear(c['K'], D).double()
    feat_proj.load_state_dict(dbl(c['sd_proj']), strict=True)
    pos_embed = ref.position_embedding.PositionEmbeddingLearned(3, D).double()
    assert list(pos_embed.state_dict()) == list(c['sd_pos']), 'the seeded state_dict does not have the reference embedding\'s keys'
    pos_embed.load_state_dict(dbl(c['sd_pos']), strict=True)
    layer = T.TransformerCrossEncoderLayer(D, c['H'], c['F'], 0.0, activation='relu', normalize_before=True, sa_val_has_pos_emb=True,
                                           ca_val_has_pos_emb=True, attention_type='dot_prod')
    enc = T.TransformerCrossEncoder(layer, L, torch.nn.LayerNorm(D), return_intermediate=True).double()
    enc.load_state_dict(dbl(c['sd_enc']), strict=True)
    head = ref.regtr.CorrespondenceRegressor(D).double()
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
    pe = pos_embed(c['xyz'].double())                                                   # regtr.py:149-150, inside autograd
    src_o, tgt_o = enc(side(both, 0), side(both, B), src_key_padding_mask=mask(lens[:B]), tgt_key_padding_mask=mask(lens[B:]),
                       src_pos=side(pe, 0), tgt_pos=side(pe, B))
    src_kp = [torch.from_numpy(x).double() for x in c['src_kp']]
    tgt_kp = [torch.from_numpy(x).double() for x in c['tgt_kp']]
    src_corr, tgt_corr, src_ov, tgt_ov = head(src_o, tgt_o, src_kp, tgt_kp)             # regtr.py:168
    src_feat = [src_o[:, :lens[b], b] for b in range(B)]
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

    mods = {'feat_proj': feat_proj, 'pos_embed': pos_embed, 'transformer_encoder': enc, 'correspondence_decoder': head,
            'feature_criterion': crit, 'feature_criterion_un': crit_un}
    corr = torch.cat([w[i] for w in src_corr] + [w[i] for w in tgt_corr]).detach()
    logit = torch.cat([o[i, :, 0] for o in src_ov] + [o[i, :, 0] for o in tgt_ov]).detach()
    g = {'case': np.array(PR.STACK_CASE), 'seed': np.int64(seed), 'D': np.int64(D), 'row_step': np.int64(ROW_STEP),
         'w_rows': np.array(W_ROWS, dtype=np.int64), 'relu_margin': np.float64(margin),
         'corr': corr[::ROW_STEP].numpy(), 'logit': logit[::ROW_STEP].numpy(), 'd_feats_un': feats_un.grad[::ROW_STEP].numpy(),
         'loss/total': np.float64(total.item())}
    for k, v in losses.items():
        g['loss/' + k] = np.float64(v.item())
    sub = lambda t: t if t.dim() == 1 or t.shape[0] < 64 else t[W_ROWS]                  # (mlp.0.weight has 32 rows: in full)
    for mk, m in mods.items():
        for k, p in m.named_parameters():
            g[f'g/{mk}.{k}'] = sub(p.grad).numpy()
    # the restatement against these (float64 both): what tests/test_gpu_posemb_mlp.py's float32 fallback leans on
    f64 = PR.full(c)
    worst = max(float((sub(f64['grads'][k[2:]]) - torch.from_numpy(v)).abs().max() / max(np.abs(v).max(), 1e-300))
                for k, v in g.items() if k.startswith('g/'))
    path = os.path.join(GOLD, f'head_grads_learned_{PR.STACK_CASE}.npz')
    np.savez_compressed(path, **g)
    print(PR.STACK_CASE, ' '.join(f'{k} {v.item():.6f}' for k, v in losses.items()), f'total {total.item():.6f} relu margin {margin:.2e} '
          f'restatement vs reference (float64) worst {worst:.1e} {os.path.getsize(path) / 1024:.0f} KB')


if __name__ == '__main__':
    if 'stack' not in sys.argv[1:]:
        run_model_cases()
    if 'model' not in sys.argv[1:]:
        run_stack_case()
