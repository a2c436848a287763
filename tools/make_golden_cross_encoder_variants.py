"""Generates tests/golden/cross_encoder_variants.npz by running the REAL reference TransformerCrossEncoder
(models/transformer/transformers.py:18-59, forward_post :121-181, forward_pre :183-244) forward in float64 on the CPU for every
configuration of tests/cross_encoder_fwd_ref.py (VARIANTS: normalize_before x sa_val_has_pos_emb x ca_val_has_pos_emb under a
positional embedding, both norm orders without one, each as return_intermediate with RegTR's final norm -- pre-norm only -- and as the
bare last layer; plus the final norm without return_intermediate), on clouds padded to (N_max, B, D) under key-padding masks, as the
reference pads them (regtr.py:147-172).  Runs where the reference tree is available, never on a GPU machine.
Re-run:  python tools/make_golden_cross_encoder_variants.py

The seeded parameters, tokens and positional embedding are tests/cross_encoder_fwd_ref.py's draw_case('golden'): the seed and the shape
are stored, matrices are not.  Stored per variant (float64): `out/<variant>` (L | 1, N, D), packed rows."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                  # noqa: E402
from tests import cross_encoder_fwd_ref as R                   # noqa: E402

PATH = os.path.join(ROOT, 'tests', 'golden', 'cross_encoder_variants.npz')


def run(ref, c, vname):
    (pre, sa, ca, with_pe), mode = R.VARIANTS[vname]
    final, ri = R.stack_form((pre, sa, ca, with_pe), mode)
    T = ref.transformers
    D, B = c['D'], len(c['src'])
    layer = T.TransformerCrossEncoderLayer(D, c['H'], c['F'], 0.0, activation='relu', normalize_before=pre, sa_val_has_pos_emb=sa,
                                           ca_val_has_pos_emb=ca, attention_type='dot_prod')
    enc = T.TransformerCrossEncoder(layer, c['L'], torch.nn.LayerNorm(D) if final else None, return_intermediate=ri).double()
    sd = {k: v.double() for k, v in c['sd'].items() if final or not k.startswith('norm.')}
    assert list(enc.state_dict()) == list(sd), 'the seeded state_dict does not have the reference module\'s keys'
    enc.load_state_dict(sd, strict=True)

    seg = c['seg']
    lens = [int(seg[i + 1] - seg[i]) for i in range(2 * B)]
    x, pe = c['x'].double(), c['pe'].double() if with_pe else None
    cut = lambda t, i: t[int(seg[i]):int(seg[i + 1])]
    pad = torch.nn.utils.rnn.pad_sequence
    mask = lambda ls: torch.tensor([[j >= n for j in range(max(ls))] for n in ls])
    side = lambda t, lo: pad([cut(t, i) for i in range(lo, lo + B)])                    # (N_max, B, D)
    with torch.no_grad():
        src_o, tgt_o = enc(side(x, 0), side(x, B), src_key_padding_mask=mask(lens[:B]), tgt_key_padding_mask=mask(lens[B:]),
                           src_pos=side(pe, 0) if with_pe else None, tgt_pos=side(pe, B) if with_pe else None)
    # back to packed rows [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]: (L | 1, N, D)
    out = torch.cat([src_o[:, :lens[b], b] for b in range(B)] + [tgt_o[:, :lens[B + b], b] for b in range(B)], 1)
    assert tuple(out.shape) == (c['L'] if ri else 1, len(x), D)
    return out.numpy()


def main():
    ref = ref_loader.load()
    c = R.draw_case('golden')
    g = {'seed': np.int64(c['seed']), 'D': np.int64(c['D']), 'H': np.int64(c['H']), 'F': np.int64(c['F']), 'L': np.int64(c['L']),
         'src_lens': np.array(c['src'], dtype=np.int64), 'tgt_lens': np.array(c['tgt'], dtype=np.int64),
         'variants': np.array(list(R.VARIANTS))}
    for vname in R.VARIANTS:
        g['out/' + vname] = run(ref, c, vname)
    np.savez_compressed(PATH, **g)
    print(len(R.VARIANTS), 'variants', f'{os.path.getsize(PATH) / 1024:.0f} KB')


if __name__ == '__main__':
    main()
