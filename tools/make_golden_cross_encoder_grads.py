"""Generates tests/golden/cross_encoder_grads_<case>.npz by running the REAL reference TransformerCrossEncoder
(models/transformer/transformers.py:18-59, forward_pre :183-244) forward + backward in float64 on the CPU, on clouds padded to
(N_max, B, D) under key-padding masks, as the reference pads them.  Runs where the reference tree is available, never on a GPU machine.
Re-run:  python tools/make_golden_cross_encoder_grads.py

The cases, their seeded parameters, tokens, positional embedding and upstream gradient are tests/cross_encoder_grads_ref.py's
(CASES / draw_case): seeds and shapes are stored, matrices are not.  The loss is sum(out * d_out).

Stored (float64): `out` and `dx` (every `row_step`-th token), every bias and LayerNorm gradient in full (`g/<state_dict name>`), rows
`w_rows` of every weight gradient (`g/<name>`), `dpe` rows when the case has a positional embedding, and the reference module's
state_dict keys / shapes (`sd_keys`, `sd_shapes`).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                  # noqa: E402
from tests import cross_encoder_grads_ref as R                 # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
ROW_STEP = {'ragged': 1, 'kitchen': 13}
W_ROWS = [0, 1, 31, 63]                                         # rows of every weight gradient that are stored


def run(name):
    ref = ref_loader.load()
    T = ref.transformers
    c = R.draw_case(name)
    D, B = c['D'], len(c['src'])
    layer = T.TransformerCrossEncoderLayer(D, c['H'], c['F'], 0.0, activation='relu', normalize_before=True, sa_val_has_pos_emb=True,
                                           ca_val_has_pos_emb=True, attention_type='dot_prod')
    enc = T.TransformerCrossEncoder(layer, c['L'], torch.nn.LayerNorm(D) if c['final'] else None, return_intermediate=c['final']).double()
    sd0 = enc.state_dict()
    assert list(sd0) == list(c['sd']), 'the seeded state_dict does not have the reference module\'s keys'
    enc.load_state_dict({k: v.double() for k, v in c['sd'].items()}, strict=True)

    seg = c['seg']
    lens = [int(seg[i + 1] - seg[i]) for i in range(2 * B)]
    x = c['x'].double().requires_grad_()
    pe = c['pe'].double().requires_grad_() if c['pe'] is not None else None
    cut = lambda t, i: t[int(seg[i]):int(seg[i + 1])]
    pad = torch.nn.utils.rnn.pad_sequence
    mask = lambda ls: torch.tensor([[j >= n for j in range(max(ls))] for n in ls])
    side = lambda t, lo: pad([cut(t, i) for i in range(lo, lo + B)])                    # (N_max, B, D)
    src_o, tgt_o = enc(side(x, 0), side(x, B), src_key_padding_mask=mask(lens[:B]), tgt_key_padding_mask=mask(lens[B:]),
                       src_pos=side(pe, 0) if pe is not None else None, tgt_pos=side(pe, B) if pe is not None else None)
    # back to packed rows [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]: (L | 1, N, D)
    out = torch.cat([src_o[:, :lens[b], b] for b in range(B)] + [tgt_o[:, :lens[B + b], b] for b in range(B)], 1)
    (out * c['d_out'].double()).sum().backward()

    step = ROW_STEP[name]
    g = {'case': np.array(name), 'seed': np.int64(c['seed']), 'D': np.int64(D), 'H': np.int64(c['H']), 'F': np.int64(c['F']),
         'L': np.int64(c['L']), 'src_lens': np.array(c['src'], dtype=np.int64), 'tgt_lens': np.array(c['tgt'], dtype=np.int64),
         'row_step': np.int64(step), 'w_rows': np.array(W_ROWS, dtype=np.int64),
         'out': out.detach()[:, ::step].numpy(), 'dx': x.grad[::step].numpy(),
         'sd_keys': np.array(list(sd0.keys())), 'sd_shapes': np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd0.values()], dtype=np.int64)}
    if pe is not None:
        g['dpe'] = pe.grad[::step].numpy()
    for k, p in enc.named_parameters():
        g['g/' + k] = (p.grad if p.dim() == 1 else p.grad[W_ROWS]).numpy()
    path = os.path.join(GOLD, f'cross_encoder_grads_{name}.npz')
    np.savez_compressed(path, **g)
    print(name, tuple(out.shape), f'{os.path.getsize(path) / 1024:.0f} KB')


def main():
    for name in R.CASES:
        run(name)


if __name__ == '__main__':
    main()
