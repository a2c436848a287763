"""Times forward + backward of the differentiable cross-encoder (TransformerCrossEncoderLayer / TransformerCrossEncoder.forward_grad,
regtr_amd/transformer_grad.py) against a plain-torch restatement of the same pre-norm layer on the same GPU: nn.MultiheadAttention,
nn.LayerNorm and nn.Linear on tokens padded to (N_max, B, D) under key-padding masks, the layout the reference's
transformers.py:183-244 runs on (the padding is done once outside the timed region).
    python tools/cross_encoder_grad_bench.py [--reps 30] [--warmup 5] [--packed-only]
Shapes (those of tools/mha_grad_bench.py): 'kitchen_b2' = 2 pairs at the kitchen golden's coarsest-level sizes (410 x 339 tokens);
'synthetic_b64' = 64 pairs of 330-460 x 330-460 tokens.  D = 256, 8 heads, F = 1024, positional embedding given.  Per shape: one layer
and the six-layer stack (final norm, return_intermediate), medians of CUDA events around fwd + bwd after warm-up, and the ratio.  Then
the two new kernels alone at the shape's row count: time and achieved bytes/s (the bytes the kernel must move: ops.layernorm_bwd reads
x, dy, dres and writes dx; ops.bias_relu_bwd with h reads g, h and writes dh).
--packed-only runs a few packed steps of the six-layer stack and nothing else: the command to put under `rocprofv3 --kernel-trace
--stats` for the per-kernel-family shares."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, H, F, L = 256, 8, 1024, 6


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


class PaddedLayer(nn.Module):
    """The pre-norm cross-encoder layer in stock torch modules on padded (N_max, B, D) clouds; the values carry the embedding."""

    def __init__(self):
        super().__init__()
        self.self_attn, self.multihead_attn = nn.MultiheadAttention(D, H), nn.MultiheadAttention(D, H)
        self.linear1, self.linear2 = nn.Linear(D, F), nn.Linear(F, D)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(D), nn.LayerNorm(D), nn.LayerNorm(D)

    def forward(self, src, tgt, src_mask, tgt_mask, src_pe, tgt_pe):
        s, t = self.norm1(src) + src_pe, self.norm1(tgt) + tgt_pe
        src = src + self.self_attn(s, s, s, key_padding_mask=src_mask, need_weights=False)[0]
        tgt = tgt + self.self_attn(t, t, t, key_padding_mask=tgt_mask, need_weights=False)[0]
        s, t = self.norm2(src) + src_pe, self.norm2(tgt) + tgt_pe
        src, tgt = (src + self.multihead_attn(s, t, t, key_padding_mask=tgt_mask, need_weights=False)[0],
                    tgt + self.multihead_attn(t, s, s, key_padding_mask=src_mask, need_weights=False)[0])
        src = src + self.linear2(torch.relu(self.linear1(self.norm3(src))))
        tgt = tgt + self.linear2(torch.relu(self.linear1(self.norm3(tgt))))
        return src, tgt


class PaddedStack(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.layers = nn.ModuleList([PaddedLayer() for _ in range(n)])
        self.norm = nn.LayerNorm(D)

    def forward(self, src, tgt, *a):
        outs = []
        for layer in self.layers:
            src, tgt = layer(src, tgt, *a)
            outs.append((self.norm(src), self.norm(tgt)))
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--packed-only', action='store_true')
    args = ap.parse_args()
    from regtr_amd import ops
    from regtr_amd.transformer import TransformerCrossEncoder, TransformerCrossEncoderLayer
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    shapes = {'kitchen_b2': [(410, 339)] * 2,
              'synthetic_b64': [(int(rng.integers(330, 461)), int(rng.integers(330, 461))) for _ in range(64)]}
    for name, sizes in shapes.items():
        B = len(sizes)
        lens = [p[0] for p in sizes] + [p[1] for p in sizes]                      # [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]
        N, n_max = sum(lens), max(lens)
        off = np.concatenate([[0], np.cumsum(lens)])
        seg = torch.tensor(off, dtype=torch.int32, device=dev)
        kv_self = torch.arange(2 * B, dtype=torch.int32, device=dev)
        kv_cross = torch.cat([torch.arange(B, 2 * B), torch.arange(B)]).to(dev, torch.int32)
        gen = torch.Generator(device='cpu').manual_seed(1)
        x = torch.randn((N, D), generator=gen).to(dev).requires_grad_()
        pe = torch.randn((N, D), generator=gen).to(dev)
        g = torch.randn((L, N, D), generator=gen).to(dev)
        layer = TransformerCrossEncoderLayer(D, H, F, 0.0, 'relu', True, True, True)
        enc = TransformerCrossEncoder(layer, L, nn.LayerNorm(D), return_intermediate=True).to(dev)

        def packed_layer():
            x.grad = None
            enc.zero_grad(set_to_none=True)
            enc.layers[0].forward_grad(x, pe, seg, kv_self, kv_cross, n_max).backward(g[0])

        def packed_stack():
            x.grad = None
            enc.zero_grad(set_to_none=True)
            enc.forward_grad(x, pe, seg, kv_self, kv_cross, n_max).backward(g)
        if args.packed_only:
            if name == 'synthetic_b64':
                for _ in range(4):
                    packed_stack()
                torch.cuda.synchronize()
            continue

        # the padded baseline: (N_max, B, D) per side
        def pad(t, lo):
            p = torch.zeros((n_max, B, t.shape[-1]), device=dev)
            for b in range(B):
                p[:lens[lo + b], b] = t.detach()[off[lo + b]:off[lo + b + 1]]
            return p
        src, tgt = pad(x, 0).requires_grad_(), pad(x, B).requires_grad_()
        src_pe, tgt_pe = pad(pe, 0), pad(pe, B)
        mask = lambda lo: torch.tensor([[j >= lens[lo + b] for j in range(n_max)] for b in range(B)], device=dev)
        src_mask, tgt_mask = mask(0), mask(B)
        g_src = torch.stack([pad(g[l], 0) for l in range(L)])
        g_tgt = torch.stack([pad(g[l], B) for l in range(L)])
        ref = PaddedStack(L).to(dev)

        def padded_layer():
            src.grad = tgt.grad = None
            ref.zero_grad(set_to_none=True)
            s, t = ref.layers[0](src, tgt, src_mask, tgt_mask, src_pe, tgt_pe)
            torch.autograd.backward([s, t], [g_src[0], g_tgt[0]])

        def padded_stack():
            src.grad = tgt.grad = None
            ref.zero_grad(set_to_none=True)
            s, t = ref(src, tgt, src_mask, tgt_mask, src_pe, tgt_pe)
            torch.autograd.backward([s, t], [g_src, g_tgt])
        for what, pk, pd in (('layer', packed_layer, padded_layer), ('stack6', packed_stack, padded_stack)):
            ms_p = median_ms(pk, args.reps, args.warmup)
            ms_t = median_ms(pd, args.reps, args.warmup)
            print(json.dumps({'shape': name, 'what': what, 'pairs': B, 'tokens': N, 'D': D, 'heads': H, 'F': F,
                              'packed_fwd_bwd_ms': round(ms_p, 3), 'torch_padded_fwd_bwd_ms': round(ms_t, 3),
                              'torch_over_packed': round(ms_t / ms_p, 2), 'reps': args.reps}), flush=True)

        # the two new kernels alone at this row count
        xd, dy, dres, gamma = x.detach(), g[0], g[1], torch.ones(D, device=dev)
        ms = median_ms(lambda: ops.layernorm_bwd(xd, gamma, dy, dres=dres), args.reps, args.warmup)
        print(json.dumps({'shape': name, 'kernel': 'layernorm_bwd', 'rows': N, 'D': D, 'ms': round(ms, 4),
                          'TB_per_s': round(4 * N * D * 4 / ms / 1e9, 3)}), flush=True)
        gh, hh = torch.randn((N, F), device=dev), torch.randn((N, F), device=dev).relu_()
        ms = median_ms(lambda: ops.bias_relu_bwd(gh, hh), args.reps, args.warmup)
        print(json.dumps({'shape': name, 'kernel': 'bias_relu_bwd (with h)', 'rows': N, 'N': F, 'ms': round(ms, 4),
                          'TB_per_s': round(3 * N * F * 4 / ms / 1e9, 3)}), flush=True)
        ms = median_ms(lambda: ops.bias_relu_bwd(gh), args.reps, args.warmup)
        print(json.dumps({'shape': name, 'kernel': 'bias_relu_bwd (bias only)', 'rows': N, 'N': F, 'ms': round(ms, 4),
                          'TB_per_s': round(N * F * 4 / ms / 1e9, 3)}), flush=True)


if __name__ == '__main__':
    main()
