// Backward of the multi-head attention core of attention.hip (regtr_mha_fwd) on the same PACKED, ragged layout: cloud c's
// queries attend the keys / values of cloud kv_of[c], head dimension 32, exact-f32 MFMA (v_mfma_f32_32x32x2_f32), float32
// softmax statistics with the hardware exp2 on log2(e)-scaled scores.  For query i of cloud c and key j of cloud kv_of[c]:
//   s_ij = scale q_i.k_j   P = softmax_j(s)   dP_ij = dO_i.v_j   delta_i = sum_j P_ij dP_ij   dS_ij = P_ij (dP_ij - delta_i)
//   dV_j = sum_i P_ij dO_i      dQ_i = scale sum_j dS_ij k_j      dK_j = scale sum_i dS_ij q_i
// The backward is a function of (q, k, v, dO) and the layout only: it recomputes S and the row statistics (flash style) and never
// reads the forward's output, so it is the same whichever forward precision produced O.  Owner computes, two launches:
//   k_mha_bwd_q   one wave owns a 32-QUERY tile of one (cloud, head) and sweeps the key cloud twice.  Sweep 1: running
//                 (max m, sum l, D = sum_j e^(s - m) dP_ij), all rescaled online -> lse_i = m + log2 l (log2 domain) and
//                 delta_i = D / l, written to the workspace [head][row].  delta comes from this online accumulation of its own
//                 -- not from rowsum(dO o O'), which would need the O' accumulator and a second product per tile for one number.
//                 Sweep 2: P = exp2(s - lse), dS, dQ^T += K^T dS^T.
//   k_mha_bwd_kv  one wave owns a 32-KEY tile of one (cloud, head) and walks the query clouds c' = 0 .. n_clouds - 1 in ascending
//                 order, taking those with kv_of[c'] == its cloud (a workgroup-uniform scalar test; any kv_of is legal, and several
//                 query clouds on one key cloud accumulate in that fixed order): dV^T += dO^T P, dK^T += Q^T dS.  A cloud nobody
//                 attends gets zero rows, written.
// Every output row has one owner: no atomics, bit-reproducible.  Rows outside every cloud are not written.
//
// Lanes.  As in k_mha_fwd the score tile is computed TRANSPOSED to the owner: the streamed tile (32 rows from LDS) is the A operand,
// the owned rows (registers, B operand: lane (l31, hi) holds X[row l31][2 s + hi], s < 16) are the columns.  Each lane then holds the
// scores of ONE owned row against the 16 streamed rows acc_row(r, hi); the other half-wave holds the complementary 16, so row
// statistics need 15 in-register ops and one exchange with lane ^ 32.  dS^T (and P^T) go straight back in as the B operand of the
// accumulating products: contraction step s of half-wave hi uses streamed row acc_row(s, hi) on both operands.  Accumulator register
// r of the outputs is head channel acc_row(r, hi) of the owned row l31: four float4 stores per lane.
// LDS: two 32 x 32 float tiles with row stride 33 (both fragment read patterns conflict free); the next tile's global loads are
// issued before the MFMAs of the current one (register staging).  Loads come from CLAMPED rows with no predicate; dead rows are
// neutralised arithmetically (scale 0, score -inf, lse +inf).
#include "common.h"
#include "mfma_operands.h"

namespace {

constexpr int HD = 32;       // head dimension handled by these kernels
constexpr int TQ = 32, TK = 32;
constexpr int LDS_STRIDE = HD + 1;
constexpr float LOG2E = 1.44269504088896340736f;

struct MhaBwdArgs {
    const float* q; const float* k; const float* v; const float* d_out;   // row-major, leading dims ldq / ldk / ldv / ld_do
    float* dq; float* dk; float* dv;
    const int* seg_off; const int* kv_of;
    float* lse; float* delta;       // workspace, [n_heads][n_total] each: log2-domain logsumexp and delta of every (head, query row)
    int ldq, ldk, ldv, ld_do, ld_dq, ld_dk, ld_dv, n_clouds, n_total;
    float scale;
};

// accumulator register r of half-wave `hi` holds matrix row  (r & 3) + 8 * (r >> 2) + 4 * hi
__device__ __forceinline__ int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// rows t0 .. t0 + 31 of the cloud starting at `base` (clamped to its last row) of two matrices: a row is one 128-B line, 8 lanes per row
__device__ __forceinline__ void fetch_tiles(float4 (&a)[4], float4 (&b)[4], const float* A, int lda, const float* B, int ldb, int base,
                                            int t0, int last, int hoff, int lane)
{
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int row = min(t0 + it * 8 + (lane >> 3), last), c4 = (lane & 7) * 4;
        a[it] = *(const float4*)(A + (size_t)(base + row) * lda + hoff + c4);
        b[it] = *(const float4*)(B + (size_t)(base + row) * ldb + hoff + c4);
    }
}
__device__ __forceinline__ void store_tiles(float* As, float* Bs, const float4 (&a)[4], const float4 (&b)[4], int lane)
{
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int row = it * 8 + (lane >> 3), c4 = (lane & 7) * 4;
        float* ad = &As[row * LDS_STRIDE + c4];
        ad[0] = a[it].x; ad[1] = a[it].y; ad[2] = a[it].z; ad[3] = a[it].w;
        float* bd = &Bs[row * LDS_STRIDE + c4];
        bd[0] = b[it].x; bd[1] = b[it].y; bd[2] = b[it].z; bd[3] = b[it].w;
    }
}
// the owned row's B operand: X[row][2 s + hi] * scl, s < 16
__device__ __forceinline__ void load_owned(float (&x)[16], const float* p, float scl)
{
#pragma unroll
    for (int s = 0; s < 16; s++) x[s] = p[2 * s] * scl;
}
// T^T = A B^T for the streamed tile As (A operand) and the owned rows (B operand)
__device__ __forceinline__ floatx16 tile_product(const float* As, const float (&b)[16], int l31, int hi)
{
    floatx16 c;
#pragma unroll
    for (int r = 0; r < 16; r++) c[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; s++) c = __builtin_amdgcn_mfma_f32_32x32x2f32(As[l31 * LDS_STRIDE + 2 * s + hi], b[s], c, 0, 0, 0);
    return c;
}
// acc^T += As^T x^T : contraction step s uses streamed row acc_row(s, hi) on both operands
__device__ __forceinline__ floatx16 tile_accumulate(const float* As, const floatx16& x, floatx16 acc, int l31, int hi)
{
#pragma unroll
    for (int s = 0; s < 16; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[acc_row(s, hi) * LDS_STRIDE + l31], x[s], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ void store_owned(float* dst, const floatx16& o, float scl, int hi)
{
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) {
        const int d = 8 * r4 + 4 * hi;   // acc_row(4 * r4 + j, hi) = j + 8 * r4 + 4 * hi
        *(float4*)(dst + d) = make_float4(o[4 * r4] * scl, o[4 * r4 + 1] * scl, o[4 * r4 + 2] * scl, o[4 * r4 + 3] * scl);
    }
}

// (waves_per_eu: with a register budget hipcc keeps the MFMA accumulators in VGPRs instead of AGPRs, see k_mha_fwd_bf16)
__global__ void __launch_bounds__(RG_WAVE) __attribute__((amdgpu_waves_per_eu(2))) k_mha_bwd_q(MhaBwdArgs g)
{
    __shared__ float Ks[TK * LDS_STRIDE];
    __shared__ float Vs[TK * LDS_STRIDE];
    const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
    const int cloud = blockIdx.z, head = blockIdx.y;
    const int q_begin = g.seg_off[cloud], q_end = g.seg_off[cloud + 1];
    const int q0 = q_begin + blockIdx.x * TQ;
    if (q0 >= q_end) return;                                        // (workgroup-uniform)
    const int kc = g.kv_of[cloud];
    const int k_begin = g.seg_off[kc], nk = g.seg_off[kc + 1] - k_begin;
    const int hoff = head * HD;
    const int qrow = q0 + l31;
    const bool live = qrow < q_end;

    // owned rows: q * scale * log2(e) and dO (clamped row, scale 0 for a dead lane: branch free)
    float qreg[16], greg[16];
    load_owned(qreg, g.q + (size_t)(live ? qrow : q_begin) * g.ldq + hoff + hi, live ? g.scale * LOG2E : 0.f);
    load_owned(greg, g.d_out + (size_t)(live ? qrow : q_begin) * g.ld_do + hoff + hi, live ? 1.f : 0.f);

    const int nk1 = nk > 0 ? nk - 1 : 0;
    const int kb = nk > 0 ? k_begin : q_begin;         // an empty key cloud: the loops below do not run
    float4 kreg[4], vreg[4];
    // one streamed tile: LDS <- registers, request the next one, S^T and dP^T of the tile (keys past nk: score -inf)
    auto tile = [&](int kt, floatx16& sc, floatx16& dp) {
        __syncthreads();                                 // the previous tile is consumed
        store_tiles(Ks, Vs, kreg, vreg, lane);
        __syncthreads();
        fetch_tiles(kreg, vreg, g.k, g.ldk, g.v, g.ldv, kb, kt + TK, nk1, hoff, lane);      // unconditional: rows are clamped
        sc = tile_product(Ks, qreg, l31, hi);
        dp = tile_product(Vs, greg, l31, hi);
        if (kt + TK > nk) {                              // (workgroup-uniform: only the last tile has keys past the end)
#pragma unroll
            for (int r = 0; r < 16; r++)
                if (kt + acc_row(r, hi) >= nk) sc[r] = -INFINITY;
        }
    };

    // sweep 1: lse_i and delta_i
    float m_run = -INFINITY, l_run = 0.f, d_run = 0.f;
    fetch_tiles(kreg, vreg, g.k, g.ldk, g.v, g.ldv, kb, 0, nk1, hoff, lane);
    for (int kt = 0; kt < nk; kt += TK) {
        floatx16 sc, dp;
        tile(kt, sc, dp);
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; r++) mx = fmaxf(mx, sc[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, RG_WAVE));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float psum = 0.f, dsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float p = __builtin_amdgcn_exp2f(sc[r] - m_new);
            psum += p;
            dsum = fmaf(p, dp[r], dsum);
        }
        psum += __shfl_xor(psum, 32, RG_WAVE);
        dsum += __shfl_xor(dsum, 32, RG_WAVE);
        l_run = fmaf(l_run, alpha, psum);
        d_run = fmaf(d_run, alpha, dsum);
        m_run = m_new;
    }
    const float lse = l_run > 0.f ? m_run + log2f(l_run) : 0.f;     // (an empty key set: nothing uses it)
    const float delta = l_run > 0.f ? d_run / l_run : 0.f;
    if (live && hi == 0 && qrow < g.n_total) {
        g.lse[(size_t)head * g.n_total + qrow] = lse;
        g.delta[(size_t)head * g.n_total + qrow] = delta;
    }

    // sweep 2: dQ^T += K^T dS^T
    floatx16 dq;
#pragma unroll
    for (int r = 0; r < 16; r++) dq[r] = 0.f;
    fetch_tiles(kreg, vreg, g.k, g.ldk, g.v, g.ldv, kb, 0, nk1, hoff, lane);
    for (int kt = 0; kt < nk; kt += TK) {
        floatx16 sc, dp;
        tile(kt, sc, dp);
#pragma unroll
        for (int r = 0; r < 16; r++) sc[r] = __builtin_amdgcn_exp2f(sc[r] - lse) * (dp[r] - delta);       // masked keys: 0 * finite
        dq = tile_accumulate(Ks, sc, dq, l31, hi);
    }
    if (live) store_owned(g.dq + (size_t)qrow * g.ld_dq + hoff, dq, g.scale, hi);     // an empty key cloud -> zeros
}

__global__ void __launch_bounds__(RG_WAVE) __attribute__((amdgpu_waves_per_eu(2))) k_mha_bwd_kv(MhaBwdArgs g)
{
    __shared__ float Qs[TQ * LDS_STRIDE];
    __shared__ float Gs[TQ * LDS_STRIDE];
    __shared__ float lse_s[TQ];
    __shared__ float del_s[TQ];
    const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;
    const int cloud = blockIdx.z, head = blockIdx.y;
    const int k_begin = g.seg_off[cloud], k_end = g.seg_off[cloud + 1];
    const int k0 = k_begin + blockIdx.x * TK;
    if (k0 >= k_end) return;                                        // (workgroup-uniform)
    const int hoff = head * HD;
    const int krow = k0 + l31;
    const bool live = krow < k_end;

    // owned rows: k * scale * log2(e) and v (a dead lane: scale 0; what its column accumulates is never stored)
    float kreg[16], vreg[16];
    load_owned(kreg, g.k + (size_t)(live ? krow : k_begin) * g.ldk + hoff + hi, live ? g.scale * LOG2E : 0.f);
    load_owned(vreg, g.v + (size_t)(live ? krow : k_begin) * g.ldv + hoff + hi, live ? 1.f : 0.f);

    floatx16 dk, dv;
#pragma unroll
    for (int r = 0; r < 16; r++) { dk[r] = 0.f; dv[r] = 0.f; }

    for (int qc = 0; qc < g.n_clouds; qc++) {                       // ascending: the accumulation order of shared key clouds
        if (g.kv_of[qc] != cloud) continue;                         // (workgroup-uniform, scalar)
        const int q_begin = g.seg_off[qc], nq = g.seg_off[qc + 1] - q_begin;
        if (nq <= 0) continue;
        const float* lse_h = g.lse + (size_t)head * g.n_total;
        const float* del_h = g.delta + (size_t)head * g.n_total;
        float4 qreg[4], greg[4];
        float lreg, dreg;
        auto fetch = [&](int qt) {
            fetch_tiles(qreg, greg, g.q, g.ldq, g.d_out, g.ld_do, q_begin, qt, nq - 1, hoff, lane);
            const int row = min(q_begin + min(qt + l31, nq - 1), g.n_total - 1);
            lreg = lse_h[row];
            dreg = del_h[row];
        };
        fetch(0);
        for (int qt = 0; qt < nq; qt += TQ) {
            __syncthreads();                             // the previous tile is consumed
            store_tiles(Qs, Gs, qreg, greg, lane);
            if (hi == 0) {
                const bool qlive = qt + l31 < nq;        // a query row past the end: lse = +inf makes its probabilities exactly 0
                lse_s[l31] = qlive ? lreg : INFINITY;
                del_s[l31] = qlive ? dreg : 0.f;
            }
            __syncthreads();
            fetch(qt + TQ);                              // unconditional: rows are clamped
            // S and dP of the tile: rows = queries acc_row(r, hi), column = this lane's key
            floatx16 sc = tile_product(Qs, kreg, l31, hi);
            floatx16 dp = tile_product(Gs, vreg, l31, hi);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = acc_row(r, hi);
                const float p = __builtin_amdgcn_exp2f(sc[r] - lse_s[row]);
                sc[r] = p;
                dp[r] = p * (dp[r] - del_s[row]);
            }
            dv = tile_accumulate(Gs, sc, dv, l31, hi);   // dV^T += dO^T P
            dk = tile_accumulate(Qs, dp, dk, l31, hi);   // dK^T += Q^T dS
        }
    }
    if (live) {
        store_owned(g.dk + (size_t)krow * g.ld_dk + hoff, dk, g.scale, hi);
        store_owned(g.dv + (size_t)krow * g.ld_dv + hoff, dv, 1.f, hi);
    }
}

}  // namespace

extern "C" {

size_t regtr_mha_bwd_ws_bytes(int n_total, int n_heads)
{
    if (n_total <= 0 || n_heads <= 0) return 0;
    return 2 * rg_align_up((size_t)n_total * n_heads * sizeof(float), 256);     // lse | delta
}

int regtr_mha_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* d_out, int ld_do,
                  float* dq, int ld_dq, float* dk, int ld_dk, float* dv, int ld_dv, const int* seg_off, const int* kv_of,
                  int n_clouds, int n_total, int max_len, int n_heads, int head_dim, float scale, void* ws, size_t ws_bytes,
                  void* stream)
{
    if (n_clouds < 1 || n_total < 0 || max_len < 0 || n_heads < 1 || head_dim != HD) return RG_ERR_ARG;
    const int lds[7] = {ldq, ldk, ldv, ld_do, ld_dq, ld_dk, ld_dv};
    for (int i = 0; i < 7; i++)
        if (lds[i] % 4 || lds[i] < n_heads * HD) return RG_ERR_ARG;
    if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)d_out | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) % 16) return RG_ERR_ARG;
    if (max_len == 0 || n_total == 0) return RG_OK;
    if (!q || !k || !v || !d_out || !dq || !dk || !dv || !seg_off || !kv_of || !ws) return RG_ERR_ARG;
    if (ws_bytes < regtr_mha_bwd_ws_bytes(n_total, n_heads)) return RG_ERR_WORKSPACE;
    RgCarver carve(ws, ws_bytes);
    float* lse = carve.take<float>((size_t)n_total * n_heads);
    float* delta = carve.take<float>((size_t)n_total * n_heads);
    MhaBwdArgs g{q, k, v, d_out, dq, dk, dv, seg_off, kv_of, lse, delta, ldq, ldk, ldv, ld_do, ld_dq, ld_dk, ld_dv, n_clouds, n_total, scale};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(rg_cdiv(max_len, TQ), n_heads, n_clouds);
    k_mha_bwd_q<<<grid, RG_WAVE, 0, st>>>(g);
    RG_RETURN_IF_LAUNCH_FAILED();
    k_mha_bwd_kv<<<grid, RG_WAVE, 0, st>>>(g);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
