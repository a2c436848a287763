"""Times forward + backward of the differentiable correspondence head (CorrespondenceRegressor.forward_grad) and of everything above the
backbone (head_grad.stack_forward_grad: feat_proj, six cross-encoder layers, the head on the last layer) on three paths:
  * fused     the head's narrow tail through ops.head_tail_bwd (csrc/head_bwd.hip), one pass over the rows;
  * composed  the same backward from the generic ops (ops.gemm, ops.gemm_tn_any, ops.bias_relu_bwd): head_grad.use_fused_tail = False;
  * torch     stock torch modules (nn.Linear / nn.MultiheadAttention / nn.LayerNorm) on tokens padded to (N_max, B, D) under
              key-padding masks, the layout the reference runs on (the padding is done once outside the timed region).
    python tools/head_grad_bench.py [--reps 20] [--warmup 5] [--rounds 3]
Shapes (those of tools/cross_encoder_grad_bench.py): 'kitchen_b2' = 2 pairs at the kitchen golden's coarsest-level sizes (410 x 339
tokens); 'synthetic_b64' = 64 pairs of 330-460 x 330-460 tokens.  D = 256, 8 heads, F = 1024, backbone width 1024.  The paths are timed
in alternation, `rounds` times each: per path the median over the rounds of the median of CUDA events around fwd + bwd, and the
rounds' min .. max as the run-to-run spread.  Then the tail alone at the shape's row count: time and achieved bytes/s of the bytes
it must move (ops.head_tail_bwd reads h2, f and writes g2, r)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.cross_encoder_grad_bench import PaddedStack, median_ms      # noqa: E402

D, H, F, L, K = 256, 8, 1024, 6, 1024


def alternate(fns, reps, warmup, rounds):
    """{name: fn} timed in alternation -> {name: (median of the rounds' medians, min, max)} in ms."""
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(median_ms(fn, reps, warmup))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ms.items()}


def report(shape, what, res, **meta):
    row = dict(shape=shape, what=what, **meta)
    for k, (med, lo, hi) in res.items():
        row[k + '_ms'] = round(med, 3)
        row[k + '_spread_ms'] = [round(lo, 3), round(hi, 3)]
    if 'fused' in res and 'composed' in res:
        row['composed_over_fused'] = round(res['composed'][0] / res['fused'][0], 3)
    if 'fused' in res and 'torch' in res:
        row['torch_over_fused'] = round(res['torch'][0] / res['fused'][0], 2)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    from regtr_amd import head_grad, ops
    from regtr_amd.regtr import CorrespondenceRegressor
    from regtr_amd.transformer import TransformerCrossEncoder, TransformerCrossEncoderLayer
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    shapes = {'kitchen_b2': [(410, 339)] * 2,
              'synthetic_b64': [(int(rng.integers(330, 461)), int(rng.integers(330, 461))) for _ in range(64)]}

    def with_tail(fused, fn):
        def run():
            head_grad.use_fused_tail = fused
            try:
                fn()
            finally:
                head_grad.use_fused_tail = True
        return run

    for name, sizes in shapes.items():
        B = len(sizes)
        lens = [p[0] for p in sizes] + [p[1] for p in sizes]                      # [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]
        N, n_max = sum(lens), max(lens)
        off = np.concatenate([[0], np.cumsum(lens)])
        seg = torch.tensor(off, dtype=torch.int32, device=dev)
        kv_self = torch.arange(2 * B, dtype=torch.int32, device=dev)
        kv_cross = torch.cat([torch.arange(B, 2 * B), torch.arange(B)]).to(dev, torch.int32)
        gen = torch.Generator(device='cpu').manual_seed(1)
        feats = torch.randn((1, N, D), generator=gen).to(dev).requires_grad_()
        feats_un = torch.randn((N, K), generator=gen).to(dev)
        pe = torch.randn((N, D), generator=gen).to(dev)
        xyz = torch.rand((N, 3), generator=gen).to(dev)
        g_corr, g_logit = torch.randn((1, N, 3), generator=gen).to(dev), torch.randn((1, N), generator=gen).to(dev)
        g_feat = torch.randn((N, D), generator=gen).to(dev)
        head = CorrespondenceRegressor(D).to(dev)
        feat_proj = nn.Linear(K, D).to(dev)
        layer = TransformerCrossEncoderLayer(D, H, F, 0.0, 'relu', True, True, True)
        enc = TransformerCrossEncoder(layer, L, nn.LayerNorm(D), return_intermediate=True).to(dev)

        def packed_head():
            feats.grad = None
            head.zero_grad(set_to_none=True)
            corr, logit = head.forward_grad(feats)
            torch.autograd.backward([corr, logit], [g_corr, g_logit])

        def packed_stack():
            for m in (feat_proj, enc, head):
                m.zero_grad(set_to_none=True)
            _, cond, corr, logit = head_grad.stack_forward_grad(feat_proj, lambda _: pe, enc, head, feats_un, xyz, seg, kv_self, kv_cross,
                                                                n_max, [L - 1])
            torch.autograd.backward([cond[L - 1], corr, logit], [g_feat, g_corr, g_logit])

        # the padded baseline: (N_max, B, .) per side
        def pad(t, lo):
            p = torch.zeros((n_max, B, t.shape[-1]), device=dev)
            for b in range(B):
                p[:lens[lo + b], b] = t.detach()[off[lo + b]:off[lo + b + 1]]
            return p
        mask = lambda lo: torch.tensor([[j >= lens[lo + b] for j in range(n_max)] for b in range(B)], device=dev)
        src_mask, tgt_mask = mask(0), mask(B)
        t_head = nn.ModuleDict({'mlp': nn.Sequential(nn.Linear(D, D), nn.ReLU(), nn.Linear(D, D), nn.ReLU(), nn.Linear(D, 3)),
                                'conf': nn.Linear(D, 1)}).to(dev)
        t_proj, t_enc = nn.Linear(K, D).to(dev), PaddedStack(L).to(dev)
        f_pad = [pad(feats[0], lo).requires_grad_() for lo in (0, B)]
        fu_pad = [pad(feats_un, lo) for lo in (0, B)]
        pe_pad = [pad(pe, lo) for lo in (0, B)]
        gc_pad = [pad(g_corr[0], lo) for lo in (0, B)]
        gl_pad = [pad(g_logit[0, :, None], lo) for lo in (0, B)]
        gf_pad = [pad(g_feat, lo) for lo in (0, B)]

        def torch_head_on(xs):
            outs, grads = [], []
            for x, gc, gl in zip(xs, gc_pad, gl_pad):
                outs += [t_head['mlp'](x), t_head['conf'](x)]
                grads += [gc, gl]
            return outs, grads

        def torch_head():
            for x in f_pad:
                x.grad = None
            t_head.zero_grad(set_to_none=True)
            torch.autograd.backward(*torch_head_on(f_pad))

        def torch_stack():
            for m in (t_proj, t_enc, t_head):
                m.zero_grad(set_to_none=True)
            s, t = t_enc(t_proj(fu_pad[0]), t_proj(fu_pad[1]), src_mask, tgt_mask, pe_pad[0], pe_pad[1])
            outs, grads = torch_head_on([s[L - 1], t[L - 1]])
            torch.autograd.backward(outs + [s[L - 1], t[L - 1]], grads + gf_pad)

        meta = dict(pairs=B, tokens=N, D=D, reps=args.reps, rounds=args.rounds)
        report(name, 'head', alternate({'fused': with_tail(True, packed_head), 'composed': with_tail(False, packed_head),
                                        'torch': torch_head}, args.reps, args.warmup, args.rounds), **meta)
        report(name, 'stack6+head', alternate({'fused': with_tail(True, packed_stack), 'composed': with_tail(False, packed_stack),
                                               'torch': torch_stack}, args.reps, args.warmup, args.rounds), heads=H, F=F, K=K, **meta)

        # the tail alone at this row count
        h2, f = torch.randn((N, D), device=dev).relu_(), feats.detach()[0]
        w4, wc = head.coor_mlp[4].weight.detach(), head.conf_logits_decoder.weight.detach()
        dc, dl = g_corr[0].contiguous(), g_logit[0].contiguous()
        res = alternate({'fused': lambda: ops.head_tail_bwd(dc, dl, h2, f, w4, wc),
                         'composed': lambda: head_grad.tail_bwd_composed(dc, dl, h2, f, w4, wc)}, args.reps, args.warmup, args.rounds)
        report(name, 'tail alone', res, rows=N, D=D, fused_TB_per_s=round(4 * N * D * 4 / res['fused'][0] / 1e9, 3))


if __name__ == '__main__':
    main()
