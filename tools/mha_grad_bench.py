"""Times forward + backward of the differentiable packed attention (regtr_amd/attention.py: packed_mha, forward ops.mha, backward
regtr_mha_bwd) against torch's own nn.MultiheadAttention on the same GPU with the same tokens padded to (N_max, B, E) under a
key_padding_mask (the layout the reference's transformers.py:197-226 runs on).
    python tools/mha_grad_bench.py [--reps 50] [--warmup 10]
Shapes (those of tools/loss_grad_bench.py): 'kitchen_b2' = 2 pairs at the kitchen golden's coarsest-level sizes (410 x 339 tokens);
'synthetic_b64' = 64 pairs of 330-460 x 330-460 tokens; 8 heads, E = 256; each for self (kv_of = identity) and cross (pair swap)
attention.  Three medians per line (CUDA events around fwd + bwd, after warm-up, one process): the packed CORE alone (packed_mha on
ready projections), the packed MODULE (PackedMultiheadAttention: torch linears + the core) and the padded torch module with the same
weights; the padding itself is done once outside the timed region."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    args = ap.parse_args()
    from regtr_amd.attention import PackedMultiheadAttention, packed_mha
    dev = torch.device('cuda:0')
    E, H = 256, 8
    rng = np.random.default_rng(0)
    shapes = {'kitchen_b2': [(410, 339)] * 2,
              'synthetic_b64': [(int(rng.integers(330, 461)), int(rng.integers(330, 461))) for _ in range(64)]}
    for name, sizes in shapes.items():
        lens = [n for pair in sizes for n in pair]
        C, N, n_max = len(lens), sum(lens), max(lens)
        off = np.concatenate([[0], np.cumsum(lens)])
        seg = torch.tensor(off, dtype=torch.int32, device=dev)
        gen = torch.Generator(device='cpu').manual_seed(1)
        x = torch.randn((N, E), generator=gen).to(dev).requires_grad_()
        g = torch.randn((N, E), generator=gen).to(dev)
        ref = torch.nn.MultiheadAttention(E, H).to(dev)
        mod = PackedMultiheadAttention(E, H).to(dev)
        mod.load_state_dict(ref.state_dict())
        for mode in ('self', 'cross'):
            kv = list(range(C)) if mode == 'self' else [c ^ 1 for c in range(C)]
            kvt = torch.tensor(kv, dtype=torch.int32, device=dev)
            # padded (N_max, C, E) tensors for the baseline: queries of cloud c, keys / values of cloud kv[c]
            xq = torch.zeros((n_max, C, E), device=dev)
            xk = torch.zeros((n_max, C, E), device=dev)
            mask = torch.ones((C, n_max), dtype=torch.bool, device=dev)
            for c in range(C):
                xq[:lens[c], c] = x.detach()[off[c]:off[c + 1]]
                xk[:lens[kv[c]], c] = x.detach()[off[kv[c]]:off[kv[c] + 1]]
                mask[c, :lens[kv[c]]] = False
            xq.requires_grad_()
            xk.requires_grad_()
            gp = torch.zeros((n_max, C, E), device=dev)
            for c in range(C):
                gp[:lens[c], c] = g[off[c]:off[c + 1]]
            qkv = torch.randn((N, 3 * E), generator=gen).to(dev).requires_grad_()

            def core():
                qkv.grad = None
                packed_mha(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], seg, kvt, n_max, H).backward(g)

            def packed():
                x.grad = None
                mod.zero_grad(set_to_none=True)
                mod(x, x, x, seg, kvt, n_max).backward(g)

            def padded():
                xq.grad = None
                xk.grad = None
                ref.zero_grad(set_to_none=True)
                ref(xq, xk, xk, key_padding_mask=mask, need_weights=False)[0].backward(gp)
            ms_c = median_ms(core, args.reps, args.warmup)
            ms_p = median_ms(packed, args.reps, args.warmup)
            ms_t = median_ms(padded, args.reps, args.warmup)
            print(json.dumps({'shape': name, 'mode': mode, 'pairs': len(sizes), 'tokens': N, 'heads': H, 'E': E,
                              'packed_core_fwd_bwd_ms': round(ms_c, 3), 'packed_module_fwd_bwd_ms': round(ms_p, 3),
                              'torch_padded_module_fwd_bwd_ms': round(ms_t, 3), 'speedup_module': round(ms_t / ms_p, 2),
                              'reps': args.reps}), flush=True)


if __name__ == '__main__':
    main()
