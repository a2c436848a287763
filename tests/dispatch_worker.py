"""GEMM / attention checks against float64 shared by tests/test_gpu_dispatch.py and its child processes.

As a script it is the child: `REGTR_DEV=1 REGTR_VARIANT=dispatch [REGTR_X3_*=..] python tests/dispatch_worker.py gemm|mha OUT` loads
libregtr_hip.dispatch.so (regtr_amd/build.py: build_dispatch), whose tile planner reads the forced-route switches once per process,
runs the cases and writes JSON verdicts (gemm) or the attention outputs (mha, a torch file) to OUT for the parent to assert on."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SENTINEL = 1234.5          # the finite value around the output view; the view itself starts as NaN
SLOPE, EPS = 0.1, 1e-5


def ragged_lens(M):
    """Clouds of M rows with an empty and two one-row clouds among them, so that statistics tiles straddle tiny clouds."""
    if M < 3:
        return [M, 0]
    return [1, 0, M // 2 - 1, 1, M - M // 2 - 1]


def seg_tensor(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return torch.tensor(off, dtype=torch.int32, device='cuda')


def stats64(y, lens):
    """Per-cloud (mean, rstd) in float64 of y's rows (InstanceNorm, biased variance); an empty cloud gives (0, 0) as the kernels do."""
    out, o = torch.zeros((len(lens), y.shape[1], 2), dtype=torch.float64, device=y.device), 0
    for c, n in enumerate(lens):
        if n:
            blk = y[o:o + n].double()
            out[c, :, 0] = blk.mean(0)
            out[c, :, 1] = 1.0 / torch.sqrt(blk.var(0, unbiased=False) + EPS)
        o += n
    return out


def check_gemm(M, N, K, planes=3, a_stats=False, want_stats=False, ldc_pad=4, seed=0, lens=None, forced=False):
    """ops.gemm on the split kernel (planes 1-3; 4 = the f16 pair) with the full epilogue -- bias, row_div, ReLU, residual -- into a NaN-filled
    strided view of C inside a buffer of finite sentinels, against float64.  Returns a JSON-able verdict (err is relative to max |ref|)."""
    from regtr_amd import _lib, ops
    g = torch.Generator().manual_seed(seed * 7919 + M * 31 + N * 7 + K)
    lens = ragged_lens(M) if lens is None else lens
    assert sum(lens) == M
    seg = seg_tensor(lens)
    a = (torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g)) + 0.3).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    bias, res = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
    div = torch.randint(1, 40, (M,), generator=g).float().cuda()
    st_a = stats64(a, lens).float().contiguous() if a_stats else None      # the (mean, rstd) table of A, from float64
    a64 = a.double()
    if a_stats:                                   # A' = LeakyReLU(InstanceNorm(A)) with the float32 statistics the kernel reads
        rows = torch.repeat_interleave(torch.arange(len(lens), device='cuda'), torch.tensor(lens, device='cuda'))
        sa = st_a.double()[rows]
        a64 = torch.nn.functional.leaky_relu((a64 - sa[..., 0]) * sa[..., 1], SLOPE)
    ref = torch.relu(a64 @ w.double().t() / div.double()[:, None] + bias.double()) + res.double()
    ldc = N + ldc_pad
    buf = torch.full((M + 2, ldc), SENTINEL, dtype=torch.float32, device='cuda')
    out = buf[1:M + 1, :N]
    out.fill_(float('nan'))
    sw = ops.SplitWeight(w, 'nk')
    ws = (seg, max(lens)) if want_stats else None
    kw = dict(bias=bias, row_div=div, residual=res, relu=True, a_stats=st_a, a_seg_off=seg if a_stats else None, want_stats=ws)
    keep = ops.force_x3_gemm
    ops.force_x3_gemm = True
    try:
        if planes == 4:
            assert sw.f16_ok and ops.f16_pair_ok(M, N, K, want_stats or a_stats), 'the f16 pair format does not serve this launch'
            with ops.f16_pair(True):
                r = ops.gemm(a, sw, out=out, **kw)
        else:
            r = ops.gemm(a, sw, out=out, planes=planes, **kw)
    finally:
        ops.force_x3_gemm = keep
    torch.cuda.synchronize()
    outside = buf.clone()
    outside[1:M + 1, :N] = SENTINEL
    v = {'M': M, 'N': N, 'K': K, 'planes': planes, 'a_stats': bool(a_stats), 'want_stats': bool(want_stats), 'ldc': ldc,
         'finite': bool(torch.isfinite(out).all()), 'outside_untouched': bool((outside == SENTINEL).all())}
    scale = max(ref.abs().max().item(), 1e-30)
    v['err'] = ((out.double() - ref).abs().max() / scale).item() if v['finite'] else float('inf')
    if planes == 3:                               # float32-grade: the exact-f32 kernel's bound, and at most twice that kernel's error
        out32 = ops.gemm(a, w.t().contiguous(), **dict(kw, want_stats=None))
        err32 = ((out32.double() - ref).abs().max() / scale).item()
        tol = (2e-6 * K ** 0.5 * 4 + 1e-6) * max(1.0, scale / 10) / scale
        # (the accumulation error grows with the square root of the k-chunk each float32 sum runs over: a forced plan that keeps K in
        #  one chunk where the exact-f32 kernel splits it -- K = 1000 in one chunk against seven -- is held to twice that ratio instead)
        L = _lib.lib()
        s32, s3 = (max(1, L.regtr_gemm_f32_ws_bytes(M, N, K) // (4 * M * N)), max(1, L.regtr_gemm_x3_ws_bytes(M, N, K) // (4 * M * N)))
        v['err_f32'], v['splits'] = err32, [s3, s32]
        ratio = max(1.0, s32 / s3) ** 0.5 if forced else 1.0
        v['ok'] = v['err'] < tol and v['err'] < 2 * ratio * err32 + 1e-7 * max(1.0, scale / 10) / scale
    else:
        v['ok'] = v['err'] < {4: 3e-6, 2: 2e-4, 1: 2e-2}[planes]
    if want_stats:
        st, rst = r[1], stats64(out, lens)
        m_err = (st[..., 0].double() - rst[..., 0]).abs().max().item()
        v['stats_ok'] = bool(m_err <= 1e-6 * max(1.0, rst[..., 0].abs().max().item())
                             and ((st[..., 1].double() - rst[..., 1]).abs() <= 2e-6 * rst[..., 1].abs() + 1e-30).all())
    v['pass'] = bool(v['ok'] and v['finite'] and v['outside_untouched'] and v.get('stats_ok', True))
    return v


def forced_cases():
    """The small ragged shapes every forced-route child runs: M around the 64 / 128-row tile edges, K a multiple of 32 (row-strip and
    three-deep kernels), K = 100 (not a multiple of 32: tiled kernel only) and K = 1000 (split-K with a short last chunk); every plane count,
    with and without the folded InstanceNorm operand and the statistics epilogue, C's leading dimension alternately unaligned."""
    cases = []
    for i, M in enumerate((1, 63, 65, 127, 129)):
        for N, K in ((128, 64), (256, 100), (128, 1000)):
            pad = 3 if i % 2 else 4
            cases += [(M, N, K, p, False, False, pad) for p in (1, 2)]
            cases += [(M, N, K, p, fold, st, pad) for p in (3, 4) for fold in (False, True) for st in (False, True)]
    return cases


def mha_ref(q, k, v, lens, kv, heads):
    """softmax(q k^T / sqrt(d)) v per cloud and head in float64 on the device (clouds padded in chunks); an empty partner gives zeros."""
    E = q.shape[1]
    d = E // heads
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    out = torch.zeros(q.shape, dtype=torch.float64, device=q.device)
    L = max(lens)
    chunk = max(1, (1 << 27) // max(1, heads * L * L))
    for c0 in range(0, len(lens), chunk):
        cs = [c for c in range(c0, min(len(lens), c0 + chunk)) if lens[c] and lens[kv[c]]]
        if not cs:
            continue
        Q = torch.zeros((len(cs), L, E), dtype=torch.float64, device=q.device)
        Kp, Vp = torch.zeros_like(Q), torch.zeros_like(Q)
        mask = torch.ones((len(cs), 1, 1, L), dtype=torch.bool, device=q.device)
        for i, c in enumerate(cs):
            p = kv[c]
            Q[i, :lens[c]] = q[off[c]:off[c + 1]].double()
            Kp[i, :lens[p]] = k[off[p]:off[p + 1]].double()
            Vp[i, :lens[p]] = v[off[p]:off[p + 1]].double()
            mask[i, 0, 0, :lens[p]] = False
        Qh, Kh, Vh = (t.view(len(cs), L, heads, d).transpose(1, 2) for t in (Q, Kp, Vp))
        s = (Qh @ Kh.transpose(2, 3)) / math.sqrt(d)
        o = (torch.softmax(s.masked_fill(mask, -math.inf), -1) @ Vh).transpose(1, 2).reshape(len(cs), L, E)
        for i, c in enumerate(cs):
            out[off[c]:off[c + 1]] = o[i, :lens[c]]
    return out


def mha_inputs(lens, seed, heads=8, peak=0.0):
    """Packed q, k, v (N, 32 heads) of ragged clouds and the partner maps: self-attention and (without a peak) the two halves swapped.
    peak > 0: every query's 32-channel head vectors have norm sqrt(32) and k = q * peak / sqrt(32), so each query meets its own key at a
    score of `peak` after the 1 / sqrt(32) scaling and every other key some 20 below -- a softmax that does not subtract the row maximum
    overflows float32 (e^89) there, while the exact result stays a well-separated one-hot mix."""
    g = torch.Generator().manual_seed(seed)
    E = 32 * heads
    qkv = torch.randn(sum(lens), 3 * E, generator=g) * 1.5
    if peak:
        q = qkv[:, :E].view(-1, heads, 32)
        q = q / q.norm(dim=-1, keepdim=True) * math.sqrt(32)
        qkv[:, :E] = q.reshape(-1, E)
        qkv[:, E:2 * E] = qkv[:, :E] * (peak / math.sqrt(32))
        return qkv, [list(range(len(lens)))]
    B = len(lens) // 2
    return qkv, [list(range(len(lens))), list(range(B, 2 * B)) + list(range(B)) + list(range(2 * B, len(lens)))]


def run_mha(lens, precision, qkv, kv, heads=8):
    from regtr_amd import ops
    E = 32 * heads
    q = qkv.cuda()
    return ops.mha(q[:, :E], q[:, E:2 * E], q[:, 2 * E:], seg_tensor(lens), torch.tensor(kv, dtype=torch.int32, device='cuda'), max(lens),
                   heads, precision)


def main():
    mode, out_path = sys.argv[1], sys.argv[2]
    torch.cuda.set_device(0)
    if mode == 'gemm':
        from regtr_amd import _lib
        L = _lib.lib()
        verdicts = []
        for M, N, K, p, fold, st, pad in forced_cases():
            try:
                v = check_gemm(M, N, K, p, fold, st, pad, forced=True)
            except Exception as e:          # noqa: BLE001 -- reported per case to the parent
                v = {'M': M, 'N': N, 'K': K, 'planes': p, 'a_stats': fold, 'want_stats': st, 'ldc': N + pad, 'pass': False, 'error': repr(e)}
            v['plan'] = [L.regtr_gemm_x3_tile_rows(M, N, K), L.regtr_gemm_x3_ws_bytes(M, N, K)]    # the planner as this process sees it
            verdicts.append(v)
        with open(out_path, 'w') as f:
            json.dump(verdicts, f)
    elif mode == 'mha':
        lens = json.loads(sys.argv[3])
        qkv, kvs = mha_inputs(lens, seed=sum(lens))
        outs = {f'{p}/{i}': run_mha(lens, p, qkv, kv).cpu() for p in (0, 1, 3) for i, kv in enumerate(kvs)}
        torch.save(outs, out_path)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
