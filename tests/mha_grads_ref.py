"""Float64 restatement of the packed multi-head attention core and its backward (regtr_mha_fwd / regtr_mha_bwd; the arithmetic of
nn.MultiheadAttention between its projections, transformers.py:197-226) for tests/test_gpu_mha_grads.py and
tests/test_mha_grads_host.py, with per-element error bounds of the float32 evaluation csrc/attention_bwd.hip performs, and the same
module (projections included) on packed tokens.

Per (cloud c, head): query i of cloud c, key j of cloud kv_of[c], s_ij = q_i.k_j / sqrt(32), P = softmax_j(s), dP_ij = dO_i.v_j,
delta_i = sum_j P_ij dP_ij, dS_ij = P_ij (dP_ij - delta_i), dV_j = sum_i P_ij dO_i, dQ_i = scale sum_j dS_ij k_j, dK_j = scale sum_i
dS_ij q_i (summed over every query cloud attending the key cloud)."""
import numpy as np

U = 2.0 ** -24
LN2 = np.log(2.0)
LOG2E = 1.0 / LN2
HD = 32
TILE = 32               # rows per streamed tile of the kernels

# ---- the bound's constants, from the operation counts of csrc/attention_bwd.hip as written (first order in U; MFMA products are
# exact, every float32 sum of n terms costs n U of the sum of magnitudes)
# scores in the log2 domain, t = (q * fl(scale * log2e)) . k: the constant (scale, log2e and their product rounded: 3 U), the scaled q
# (1 U), a 32-term MFMA sum
C_T = HD + 4
C_DP = HD               # dP = dO . v: a 32-term MFMA sum
E_EXP = 4 * U           # v_exp_f32: 1 ulp = 2 U documented; 2 ulp taken
# sweep 1 per streamed tile: alpha = exp2(m_old - m_new) (E_EXP) and one fma of the running sum (U): 5 U per tile; the tile's own sum: 16
# in-register additions + the half-wave exchange (17 U); one element's exponential (E_EXP).  With T tiles: (21 + 6 T) U, see _c_l.
E_LOG = 4 * U           # log2f of the row sum: relative, 2 ulp taken
# float32's normal range ends at 2^-126 and the GPU flushes what lies below (v_exp_f32 results, VALU and MFMA operands and products): a
# saturated row's far probabilities, their dS and the products with them carry an ABSOLUTE error of up to TINY each
TINY = 2.0 ** -126


def _c_l(n_keys):
    T = -(-n_keys // TILE)
    return E_EXP + 17 * U + (E_EXP + 2 * U) * T


def core(q, k, v, d_out, seg_off, kv_of, n_heads, bounds=False):
    """q, k, v, d_out (N, 32 n_heads) float arrays, seg_off (C + 1,), kv_of (C,).  Float64 -> dict with 'o', 'dq', 'dk', 'dv' (N, E); rows
    outside every cloud are 0.  bounds=True adds 'b_dq', 'b_dk', 'b_dv': per-element bounds on |float32 kernel - float64| derived
    below.  The bound follows the kernel: P is evaluated as exp2(t - L) from the log2-domain logsumexp L of an online sweep, delta from
    the same sweep's running sum of p dP; the argument of every exponential is rounded (|t - L| U), the exponential itself has a unit
    error, and the errors of L and delta propagate into every dS of the row."""
    q, k, v, g = (np.asarray(x, dtype=np.float64) for x in (q, k, v, d_out))
    N, E = q.shape
    assert E == HD * n_heads
    scale = 1.0 / np.sqrt(HD)
    out = {n: np.zeros((N, E)) for n in ('o', 'dq', 'dk', 'dv')}
    if bounds:
        out.update({n: np.zeros((N, E)) for n in ('b_dq', 'b_dk', 'b_dv')})
    C = len(kv_of)
    # rows a key cloud accumulates over (padded to whole tiles per query cloud): the length of its dK / dV sums
    n_acc = np.zeros(C)
    for c in range(C):
        nq = seg_off[c + 1] - seg_off[c]
        if nq > 0:
            n_acc[kv_of[c]] += nq + TILE
    for c in range(C):
        qs = slice(seg_off[c], seg_off[c + 1])
        kc = kv_of[c]
        ks = slice(seg_off[kc], seg_off[kc + 1])
        nq, nk = qs.stop - qs.start, ks.stop - ks.start
        if nq == 0 or nk == 0:
            continue
        for h in range(n_heads):
            cs = slice(h * HD, (h + 1) * HD)
            Q, K, V, G = q[qs, cs], k[ks, cs], v[ks, cs], g[qs, cs]
            s = scale * (Q @ K.T)
            m = s.max(1, keepdims=True)
            e = np.exp(s - m)
            l = e.sum(1, keepdims=True)
            P = e / l
            dP = G @ V.T
            delta = (P * dP).sum(1, keepdims=True)
            dS = P * (dP - delta)
            out['o'][qs, cs] = P @ V
            out['dq'][qs, cs] = scale * (dS @ K)
            out['dk'][ks, cs] += scale * (dS.T @ Q)
            out['dv'][ks, cs] += P.T @ G
            if not bounds:
                continue
            aQ, aK, aV, aG = np.abs(Q), np.abs(K), np.abs(V), np.abs(G)
            t = s * LOG2E                                   # log2 domain
            M = m * LOG2E
            L = M + np.log2(l)
            e_t = C_T * U * scale * LOG2E * (aQ @ aK.T)     # |t^ - t|
            e_dp = C_DP * U * (aG @ aV.T)                   # |dP^ - dP|
            # sweep 1.  Element j enters the running sum through exp2(fl(t_j - m_tile)) and a chain of alphas whose exponents sum to
            # (m_final - m_tile): argument roundings of at most (M - t_j) U in all, each exponential and fma as counted in _c_l.  All
            # terms are positive, so the relative error of the row sum is the P-weighted mean of the elements':
            c_l = _c_l(nk)
            arg1 = LN2 * (e_t + U * (M - t))
            eps_l = (P * arg1).sum(1, keepdims=True) + c_l
            # L^ = fl(m + log2f(l^)): d log2 l = (dl / l) / ln 2, log2f's own error, the final addition
            e_L = eps_l * LOG2E + E_LOG * np.abs(np.log2(l)) + U * np.abs(L)
            # delta^ = D^ / l^, D^ = sum_j p~_j dP^_j (one more fma per element: U), the division U
            e_delta = (P * np.abs(dP) * (arg1 + c_l + eps_l + 2 * U)).sum(1, keepdims=True) + (P * e_dp).sum(1, keepdims=True)
            # sweep 2 and the key pass: P^ = exp2(fl(t^ - L^)), relative error rho; dS^ = fl(P^ fl(dP^ - delta^))
            rho = LN2 * (e_t + e_L + U * np.abs(t - L)) + E_EXP
            e_ds = P * ((rho + 2 * U) * np.abs(dP - delta) + e_dp + e_delta) + TINY * (np.abs(dP - delta) + 1)      # P^ and dS^ flushed
            aS = np.abs(dS)
            # dQ: an MFMA sum over the key tiles (nk rounded up to whole tiles), then * fl(scale): 2 U
            out['b_dq'][qs, cs] = scale * (e_ds @ aK + (nk + TILE + 2) * U * (aS @ aK) + nk * TINY)
            # dK / dV: MFMA sums over every query tile of every attending cloud (n_acc rows), dK then * fl(scale)
            out['b_dk'][ks, cs] += scale * (e_ds.T @ aQ + (n_acc[kc] + 2) * U * (aS.T @ aQ) + nq * TINY)
            out['b_dv'][ks, cs] += (P * rho + TINY).T @ aG + n_acc[kc] * U * (P.T @ aG) + nq * TINY
    return out


def module(query, key, value, w_in, b_in, w_out, b_out, d_y, seg_off, kv_of, n_heads):
    """nn.MultiheadAttention on packed tokens in float64 with manual backward: query / key / value (N, E), d_y (N, E) the upstream
    gradient of the output.  -> dict: 'y', 'd_query', 'd_key', 'd_value', 'd_in_proj_weight', 'd_in_proj_bias', 'd_out_proj_weight',
    'd_out_proj_bias'."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    query, key, value, w_in, b_in, w_out, b_out, d_y = map(f, (query, key, value, w_in, b_in, w_out, b_out, d_y))
    E = query.shape[1]
    wq, wk, wv = w_in[:E], w_in[E:2 * E], w_in[2 * E:]
    q = query @ wq.T + b_in[:E]
    k = key @ wk.T + b_in[E:2 * E]
    v = value @ wv.T + b_in[2 * E:]
    o = core(q, k, v, np.zeros_like(q), seg_off, kv_of, n_heads)['o']
    y = o @ w_out.T + b_out
    d_o = d_y @ w_out
    r = core(q, k, v, d_o, seg_off, kv_of, n_heads)
    return {'y': y, 'd_query': r['dq'] @ wq, 'd_key': r['dk'] @ wk, 'd_value': r['dv'] @ wv,
            'd_in_proj_weight': np.concatenate([r['dq'].T @ query, r['dk'].T @ key, r['dv'].T @ value]),
            'd_in_proj_bias': np.concatenate([r['dq'].sum(0), r['dk'].sum(0), r['dv'].sum(0)]),
            'd_out_proj_weight': d_y.T @ o, 'd_out_proj_bias': d_y.sum(0)}


def torch_module(query, key, value, w_in, b_in, w_out, b_out, d_y, seg_off, kv_of, n_heads):
    """The same quantities from float64 torch.nn.MultiheadAttention on the CPU -- the class transformers.py:197-226 calls -- with the
    clouds padded to (N_max, C, E) under a key_padding_mask.  Every cloud must be non-empty (a fully masked row is NaN in torch)."""
    import torch
    t = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))
    E = np.asarray(query).shape[1]
    C = len(kv_of)
    lens = [int(seg_off[c + 1] - seg_off[c]) for c in range(C)]
    n_max = max(lens)
    mha = torch.nn.MultiheadAttention(E, n_heads).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(t(w_in)); mha.in_proj_bias.copy_(t(b_in))
        mha.out_proj.weight.copy_(t(w_out)); mha.out_proj.bias.copy_(t(b_out))
    xq, xk, xv = t(query).requires_grad_(), t(key).requires_grad_(), t(value).requires_grad_()
    pad = lambda x, c: torch.cat([x[seg_off[c]:seg_off[c + 1]], x.new_zeros(n_max - lens[c], E)])
    Q = torch.stack([pad(xq, c) for c in range(C)], 1)
    K = torch.stack([pad(xk, kv_of[c]) for c in range(C)], 1)
    V = torch.stack([pad(xv, kv_of[c]) for c in range(C)], 1)
    mask = torch.tensor([[j >= lens[kv_of[c]] for j in range(n_max)] for c in range(C)])
    Y, _ = mha(Q, K, V, key_padding_mask=mask, need_weights=False)
    y = torch.cat([Y[:lens[c], c] for c in range(C)])
    n_live = y.shape[0]
    y.backward(t(d_y)[:n_live])
    z = lambda x: x.grad.numpy() if x.grad is not None else np.zeros(x.shape)
    return {'y': y.detach().numpy(), 'd_query': z(xq), 'd_key': z(xk), 'd_value': z(xv),
            'd_in_proj_weight': mha.in_proj_weight.grad.numpy(), 'd_in_proj_bias': mha.in_proj_bias.grad.numpy(),
            'd_out_proj_weight': mha.out_proj.weight.grad.numpy(), 'd_out_proj_bias': mha.out_proj.bias.grad.numpy()}


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
