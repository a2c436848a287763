// CircleLossFull (models/losses/feature_loss.py:160-243, dist_type 'euclidean') over packed, ragged pairs for gfx950: forward and backward
// without the reference's (N, M, D) cdist tensor, its eight (N, M) temporaries or its four logsumexp passes.
//
// Per pair, anchors a_i (coordinates optionally through the pair's pose) and positives b_j:
//   d_ij  = sqrt(sum_c (a_ic - b_jc)^2 + 1e-12)      the explicit difference, accumulated c ascending by fmaf -- not a Gram expansion
//   pos   = coord_dist_rn(i, j) < r_p,  neg = coord_dist_rn(i, j) > r_n      (loss_common.h: InfoNCE's arithmetic)
//   tp_ij = s (d - pos_margin) max(d - pos_optimal, 0) on pos, else 0;   tn_ij = s (neg_margin - d) max(neg_optimal - d, 0) on neg, else 0
//   every entry of a row enters both of its log-sum-exps: a masked one with exp(0) = 1, as the reference's -1e5 mask times a zero
//   weight leaves it.
//
// Shape: one template for all four passes.  A workgroup of 128 threads owns CL_TR = 32 rows of one pair (anchors or positives) and
// streams the pair's other side in tiles of CL_TC = 64 columns; the feature dimension goes through LDS in chunks of CL_KC = 64
// (rows padded by 4 floats: the 16 rows of one ds_read_b128 hit 16 distinct bank quads).  Thread (ty, tx) holds the 4 x 4 distances of
// rows ty + 8 r and columns tx + 16 k: per chunk step 8 ds_read_b128 feed 128 VALU instructions.  Both sides are chunked, so LDS is
// 26 KB (forward) / 35 KB (backward) whatever D: four or more workgroups per CU.  A 64-pair batch of ~400-point clouds is 13 x 64 = 832
// workgroups per pass on 256 CUs.  Every d_ij is accumulated in the same order in all four passes: they see the same bits.
//
//   k_circle_fwd<ANC_ROWS>   online (max, sum) log-sum-exp state per owned row for tp and tn, merged over the 16 column lanes by xor
//                            shuffles; writes the two LSEs and the selection flag (a pos and a neg in the row) per row.
//   k_circle_reduce          one workgroup per pair: softplus(LSEp + LSEn) / s over the selected rows and columns, float64 sums in a
//                            fixed order -> pair_out.  No workspace, no atomics.
//   k_circle_bwd<ANC_ROWS>   recomputes d_ij and the masks, forms c_ij = g_ij / d_ij from the saved statistics of row i AND column j,
//                            stages the 32 x 64 coefficient tile in LDS and accumulates sum_j c_ij F_j on vector FMAs (D / 4 accumulators
//                            per thread), F streamed in the same 64-wide chunks; out_i = (sum_j c_ij) own_i - sum_j c_ij F_j.  One owner
//                            per output row, no atomics, bit-reproducible.
//
// Compiled with -ffp-contract=off (regtr_amd/build.py) like losses.hip; the fused steps are explicit fmaf calls.
#include <math.h>

#include "common.h"
#include "loss_common.h"

namespace {

constexpr int CL_TR = 32;          // owned rows per workgroup
constexpr int CL_TC = 64;          // streamed columns per tile
constexpr int CL_KC = 64;          // features per LDS chunk
constexpr int CL_LD = CL_KC + 4;   // padded LDS row
constexpr int CL_THREADS = 128;    // 8 (ty) x 16 (tx)
constexpr float CL_EPS = 1e-12f;   // feature_loss.py's cdist: sqrt(sum + 1e-12)

struct CirArgs {
    const float* anc; int lda;
    const float* pos; int ldp;
    const float* anc_xyz; const float* pos_xyz;
    const int* anc_off; const int* pos_off;
    int n_pairs, n_anc, n_pos;
    float r_p, r_n, scale, pos_margin, pos_optimal, neg_margin, neg_optimal;
    const float* pose;
    float* anc_lse; float* anc_sel;      // [n_anc, 2] (LSE of tp, LSE of tn), [n_anc]
    float* pos_lse; float* pos_sel;      // the same per positive column
    // backward only
    const float* pair_out; const float* grad; float mean_div;
    float* d_anc; int ld_danc; float* d_pos; int ld_dpos;
};

// The squared feature distances of the calling thread's 4 x 4 elements: rows r_base + ty + 8 r of rf, columns ct + tx + 16 k of cf.
// Rows / columns outside [.., r1) / [.., c1) are staged as zeros (their results are never used).  Every thread of the workgroup calls it.
template <int D>
__device__ __forceinline__ void d2_tile(const float* __restrict__ rf, int ldr, int r_base, int r1, const float* __restrict__ cf, int ldc,
                                        int ct, int c1, float* r_s, float* c_s, float d2[4][4])
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int k = 0; k < 4; k++) d2[r][k] = 0.f;
    for (int kc = 0; kc < D; kc += CL_KC) {
        __syncthreads();                                             // the previous chunk is consumed
        for (int idx = tid; idx < CL_TR * (CL_KC / 4); idx += CL_THREADS) {
            const int jj = idx >> 4, c4 = idx & 15;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r_base + jj < r1) v = *reinterpret_cast<const float4*>(rf + (size_t)(r_base + jj) * ldr + kc + 4 * c4);
            *reinterpret_cast<float4*>(r_s + jj * CL_LD + 4 * c4) = v;
        }
        for (int idx = tid; idx < CL_TC * (CL_KC / 4); idx += CL_THREADS) {
            const int jj = idx >> 4, c4 = idx & 15;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ct + jj < c1) v = *reinterpret_cast<const float4*>(cf + (size_t)(ct + jj) * ldc + kc + 4 * c4);
            *reinterpret_cast<float4*>(c_s + jj * CL_LD + 4 * c4) = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < CL_KC / 4; q++) {
            float4 rv[4], cv[4];
#pragma unroll
            for (int r = 0; r < 4; r++) rv[r] = *reinterpret_cast<const float4*>(r_s + (ty + 8 * r) * CL_LD + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; k++) cv[k] = *reinterpret_cast<const float4*>(c_s + (tx + 16 * k) * CL_LD + 4 * q);
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float e0 = rv[r].x - cv[k].x, e1 = rv[r].y - cv[k].y, e2 = rv[r].z - cv[k].z, e3 = rv[r].w - cv[k].w;
                    d2[r][k] = fmaf(e3, e3, fmaf(e2, e2, fmaf(e1, e1, fmaf(e0, e0, d2[r][k]))));
                }
        }
    }
}

__device__ __forceinline__ void lse_push(float& m, float& s, float t)
{
    if (t > m) { s = s * expf(m - t) + 1.f; m = t; }                 // (m = -inf, s = 0 at the start: 0 * 0 + 1)
    else s += expf(t - m);
}

// the two terms of element (i, j): tp / tn and the detached weights wp / wn (0 where the entry is masked)
__device__ __forceinline__ void circle_terms(const CirArgs& g, float d, bool p, bool n, float& tp, float& tn, float& wp, float& wn)
{
    wp = p ? fmaxf(d - g.pos_optimal, 0.f) : 0.f;
    wn = n ? fmaxf(g.neg_optimal - d, 0.f) : 0.f;
    tp = g.scale * (d - g.pos_margin) * wp;
    tn = g.scale * (g.neg_margin - d) * wn;
}

__device__ __forceinline__ void load_xyz(const CirArgs& g, int b, bool is_anchor, int i, float out[3])
{
    const float* xyz = (is_anchor ? g.anc_xyz : g.pos_xyz) + 3 * (size_t)i;
    if (is_anchor && g.pose) {
        transform_rn(g.pose + 12 * (size_t)b, xyz[0], xyz[1], xyz[2], out);
    } else {
        out[0] = xyz[0]; out[1] = xyz[1]; out[2] = xyz[2];
    }
}

template <int D, bool ANC_ROWS>
__global__ __launch_bounds__(CL_THREADS) void k_circle_fwd(CirArgs g)
{
    __shared__ __attribute__((aligned(16))) float r_s[CL_TR * CL_LD];
    __shared__ __attribute__((aligned(16))) float c_s[CL_TC * CL_LD];
    __shared__ float cxyz_s[CL_TC * 3];

    const int tile = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int a0, a1, p0, p1;
    if (!pair_ok(g.anc_off, b, g.n_anc, a0, a1) || !pair_ok(g.pos_off, b, g.n_pos, p0, p1)) return;      // k_circle_reduce reports NaN
    const int r0 = ANC_ROWS ? a0 : p0, r1 = ANC_ROWS ? a1 : p1;      // owned rows
    const int c0 = ANC_ROWS ? p0 : a0, c1 = ANC_ROWS ? p1 : a1;      // streamed columns
    const int r_base = r0 + tile * CL_TR;
    if (r_base >= r1) return;                                        // (uniform over the workgroup: before any barrier)
    const float* rf = ANC_ROWS ? g.anc : g.pos;
    const int ldr = ANC_ROWS ? g.lda : g.ldp;
    const float* cf = ANC_ROWS ? g.pos : g.anc;
    const int ldc = ANC_ROWS ? g.ldp : g.lda;

    float rx[4][3], mp[4], sp[4], mn[4], sn[4];
    int anyp[4], anyn[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = r_base + ty + 8 * r;
        load_xyz(g, b, ANC_ROWS, row < r1 ? row : r0, rx[r]);
        mp[r] = mn[r] = -INFINITY;
        sp[r] = sn[r] = 0.f;
        anyp[r] = anyn[r] = 0;
    }

    for (int ct = c0; ct < c1; ct += CL_TC) {
        __syncthreads();                                             // the previous tile's coordinates are consumed
        if (tid < CL_TC) {
            float x3[3] = {0.f, 0.f, 0.f};
            if (ct + tid < c1) load_xyz(g, b, !ANC_ROWS, ct + tid, x3);
            cxyz_s[3 * tid] = x3[0]; cxyz_s[3 * tid + 1] = x3[1]; cxyz_s[3 * tid + 2] = x3[2];
        }
        float d2[4][4];
        d2_tile<D>(rf, ldr, r_base, r1, cf, ldc, ct, c1, r_s, c_s, d2);      // (its barriers publish cxyz_s)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int cc = tx + 16 * k;
            if (ct + cc >= c1) continue;
            const float cx = cxyz_s[3 * cc], cy = cxyz_s[3 * cc + 1], cz = cxyz_s[3 * cc + 2];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float d = __fsqrt_rn(__fadd_rn(d2[r][k], CL_EPS));
                const float cd = ANC_ROWS ? coord_dist_rn(rx[r][0], rx[r][1], rx[r][2], cx, cy, cz)
                                          : coord_dist_rn(cx, cy, cz, rx[r][0], rx[r][1], rx[r][2]);
                const bool p = cd < g.r_p, n = cd > g.r_n;
                float tp, tn, wp, wn;
                circle_terms(g, d, p, n, tp, tn, wp, wn);
                anyp[r] |= p;
                anyn[r] |= n;
                lse_push(mp[r], sp[r], tp);
                lse_push(mn[r], sn[r], tn);
            }
        }
    }

    // ---- merge the 16 column lanes of each row (xor within tx: a commutative merge, every lane ends with the same state)
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            lse_merge(mp[r], sp[r], __shfl_xor(mp[r], o, RG_WAVE), __shfl_xor(sp[r], o, RG_WAVE));
            lse_merge(mn[r], sn[r], __shfl_xor(mn[r], o, RG_WAVE), __shfl_xor(sn[r], o, RG_WAVE));
            anyp[r] |= __shfl_xor(anyp[r], o, RG_WAVE);
            anyn[r] |= __shfl_xor(anyn[r], o, RG_WAVE);
        }
    }
    if (tx == 0) {
        float* lse = ANC_ROWS ? g.anc_lse : g.pos_lse;
        float* sel = ANC_ROWS ? g.anc_sel : g.pos_sel;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = r_base + ty + 8 * r;
            if (row >= r1) continue;
            lse[2 * (size_t)row] = __fadd_rn(mp[r], logf(sp[r]));
            lse[2 * (size_t)row + 1] = __fadd_rn(mn[r], logf(sn[r]));
            sel[row] = (anyp[r] && anyn[r]) ? 1.f : 0.f;
        }
    }
}

__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_f(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

constexpr int CR_THREADS = 256;

// pair_out[b] = (sum of selected row_i, number of selected rows, sum of selected col_j, number of selected columns)
__global__ __launch_bounds__(CR_THREADS) void k_circle_reduce(CirArgs g, int max_anc, int max_pos, float* __restrict__ out)
{
    __shared__ double sh[CR_THREADS / RG_WAVE];
    const int b = blockIdx.x;
    int lo[2], hi[2];
    const bool ok = pair_ok(g.anc_off, b, g.n_anc, lo[0], hi[0]) && pair_ok(g.pos_off, b, g.n_pos, lo[1], hi[1]) &&
                    hi[0] - lo[0] <= max_anc && hi[1] - lo[1] <= max_pos;
    if (!ok) {                                                       // (uniform)
        if (threadIdx.x < 4) out[4 * b + threadIdx.x] = (threadIdx.x & 1) ? 0.f : NAN;
        return;
    }
    for (int side = 0; side < 2; side++) {
        const float* lse = side ? g.pos_lse : g.anc_lse;
        const float* sel = side ? g.pos_sel : g.anc_sel;
        double sum = 0.0, cnt = 0.0;
        for (int i = lo[side] + threadIdx.x; i < hi[side]; i += CR_THREADS) {
            if (sel[i] != 0.f) {
                sum += (double)__fdiv_rn(softplus_f(__fadd_rn(lse[2 * (size_t)i], lse[2 * (size_t)i + 1])), g.scale);
                cnt += 1.0;
            }
        }
        sum = rg_block_sum<CR_THREADS>(sum, sh);
        cnt = rg_block_sum<CR_THREADS>(cnt, sh);
        if (threadIdx.x == 0) { out[4 * b + 2 * side] = (float)sum; out[4 * b + 2 * side + 1] = (float)cnt; }
    }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// loss = (1 / mean_div) sum_b ((1 / nr_b) sum_sel row_i + (1 / nc_b) sum_sel col_j) / 2 with row_i = softplus(LSEp_i + LSEn_i) / s.  The
// weights max(.) are detached, so d tp / d d = s wp and d tn / d d = -s wn, and the s cancels against softplus(.) / s:
//   g_ij = k_i (exp(tp - LSEp_i) wp - exp(tn - LSEn_i) wn) + k_j (exp(tp - LSEp_j) wp - exp(tn - LSEn_j) wn),
//   k_i = (g / mean_div / 2 / nr_b) sigmoid(LSEp_i + LSEn_i) on selected rows, 0 elsewhere; k_j the same with nc_b on selected columns.
// A pair with nr_b = 0 or nc_b = 0 (a NaN loss) gets zero rows.
template <int D, bool ANC_ROWS>
__global__ __launch_bounds__(CL_THREADS) void k_circle_bwd(CirArgs g)
{
    constexpr int NK = D / CL_KC;
    __shared__ __attribute__((aligned(16))) float r_s[CL_TR * CL_LD];
    __shared__ __attribute__((aligned(16))) float c_s[CL_TC * CL_LD];
    __shared__ __attribute__((aligned(16))) float w_s[CL_TR * CL_LD];      // c_ij of the tile, [row][column]
    __shared__ float cxyz_s[CL_TC * 3];
    __shared__ float cst_s[CL_TC * 3];                                      // per column: LSEp, LSEn, k_j

    const int tile = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int a0, a1, p0, p1;
    if (!pair_ok(g.anc_off, b, g.n_anc, a0, a1) || !pair_ok(g.pos_off, b, g.n_pos, p0, p1)) return;
    const int r0 = ANC_ROWS ? a0 : p0, r1 = ANC_ROWS ? a1 : p1;
    const int c0 = ANC_ROWS ? p0 : a0, c1 = ANC_ROWS ? p1 : a1;
    const int r_base = r0 + tile * CL_TR;
    if (r_base >= r1) return;                                        // (uniform: before any barrier)
    const float* rf = ANC_ROWS ? g.anc : g.pos;
    const int ldr = ANC_ROWS ? g.lda : g.ldp;
    const float* cf = ANC_ROWS ? g.pos : g.anc;
    const int ldc = ANC_ROWS ? g.ldp : g.lda;
    float* out = ANC_ROWS ? g.d_anc : g.d_pos;
    const int ldo = ANC_ROWS ? g.ld_danc : g.ld_dpos;

    const float nr = g.pair_out[4 * b + 1], nc = g.pair_out[4 * b + 3];
    if (!(nr > 0.f && nc > 0.f) || c0 == c1) {                       // a NaN pair: zero rows (uniform)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = r_base + ty + 8 * r;
            if (row >= r1) continue;
#pragma unroll
            for (int kc = 0; kc < NK; kc++)
                *reinterpret_cast<float4*>(out + (size_t)row * ldo + kc * CL_KC + 4 * tx) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    const float gh = __fmul_rn(__fdiv_rn(g.grad[0], g.mean_div), 0.5f);
    const float k_own = __fdiv_rn(gh, ANC_ROWS ? nr : nc), k_col = __fdiv_rn(gh, ANC_ROWS ? nc : nr);
    const float* own_lse = ANC_ROWS ? g.anc_lse : g.pos_lse;
    const float* own_sel = ANC_ROWS ? g.anc_sel : g.pos_sel;
    const float* col_lse = ANC_ROWS ? g.pos_lse : g.anc_lse;
    const float* col_sel = ANC_ROWS ? g.pos_sel : g.anc_sel;

    float rx[4][3], olp[4], oln[4], ok_[4], osum[4];
    bool rok[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = r_base + ty + 8 * r;
        rok[r] = row < r1;
        const int rr = rok[r] ? row : r0;
        load_xyz(g, b, ANC_ROWS, rr, rx[r]);
        olp[r] = own_lse[2 * (size_t)rr];
        oln[r] = own_lse[2 * (size_t)rr + 1];
        ok_[r] = (rok[r] && own_sel[rr] != 0.f) ? __fmul_rn(k_own, sigmoid_f(__fadd_rn(olp[r], oln[r]))) : 0.f;
        osum[r] = 0.f;
    }
    float4 acc[NK][4];
#pragma unroll
    for (int kc = 0; kc < NK; kc++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[kc][r] = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int ct = c0; ct < c1; ct += CL_TC) {
        __syncthreads();                                             // the previous tile's coordinates, statistics and c_ij are consumed
        if (tid < CL_TC) {
            const int c = ct + tid;
            float x3[3] = {0.f, 0.f, 0.f}, lp = 0.f, ln = 0.f, kj = 0.f;
            if (c < c1) {
                load_xyz(g, b, !ANC_ROWS, c, x3);
                lp = col_lse[2 * (size_t)c];
                ln = col_lse[2 * (size_t)c + 1];
                if (col_sel[c] != 0.f) kj = __fmul_rn(k_col, sigmoid_f(__fadd_rn(lp, ln)));
            }
            cxyz_s[3 * tid] = x3[0]; cxyz_s[3 * tid + 1] = x3[1]; cxyz_s[3 * tid + 2] = x3[2];
            cst_s[3 * tid] = lp; cst_s[3 * tid + 1] = ln; cst_s[3 * tid + 2] = kj;
        }
        float d2[4][4];
        d2_tile<D>(rf, ldr, r_base, r1, cf, ldc, ct, c1, r_s, c_s, d2);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int cc = tx + 16 * k;
            const bool cok = ct + cc < c1;
            const float cx = cxyz_s[3 * cc], cy = cxyz_s[3 * cc + 1], cz = cxyz_s[3 * cc + 2];
            const float clp = cst_s[3 * cc], cln = cst_s[3 * cc + 1], kj = cst_s[3 * cc + 2];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float c = 0.f;
                if (cok && rok[r]) {
                    const float d = __fsqrt_rn(__fadd_rn(d2[r][k], CL_EPS));
                    const float cd = ANC_ROWS ? coord_dist_rn(rx[r][0], rx[r][1], rx[r][2], cx, cy, cz)
                                              : coord_dist_rn(cx, cy, cz, rx[r][0], rx[r][1], rx[r][2]);
                    const bool p = cd < g.r_p, n = cd > g.r_n;
                    float tp, tn, wp, wn;
                    circle_terms(g, d, p, n, tp, tn, wp, wn);
                    float gi = 0.f, gj = 0.f;                        // the row-statistics path of the ANCHOR, of the POSITIVE
                    const float ki = ok_[r];
                    if (wp != 0.f) { gi = __fmul_rn(expf(tp - olp[r]), wp); gj = __fmul_rn(expf(tp - clp), wp); }
                    if (wn != 0.f) { gi = __fsub_rn(gi, __fmul_rn(expf(tn - oln[r]), wn)); gj = __fsub_rn(gj, __fmul_rn(expf(tn - cln), wn)); }
                    // (own + column: the two passes add the same two products, in either order the same bits)
                    c = __fdiv_rn(__fadd_rn(__fmul_rn(ki, gi), __fmul_rn(kj, gj)), d);
                }
                w_s[(ty + 8 * r) * CL_LD + cc] = c;
                osum[r] += c;
            }
        }
        // ---- acc (32 rows x D) += c (32 x 64) x F (64 x D), F in chunks of 64 features: thread (ty, tx) owns rows ty + 8 r, features 4 tx .. + 3
#pragma unroll
        for (int kc = 0; kc < NK; kc++) {
            __syncthreads();                                         // c_s is free (d2_tile's / the previous chunk's reads); w_s is published
            for (int idx = tid; idx < CL_TC * (CL_KC / 4); idx += CL_THREADS) {
                const int jj = idx >> 4, c4 = idx & 15;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ct + jj < c1) v = *reinterpret_cast<const float4*>(cf + (size_t)(ct + jj) * ldc + kc * CL_KC + 4 * c4);
                *reinterpret_cast<float4*>(c_s + jj * CL_LD + 4 * c4) = v;
            }
            __syncthreads();
#pragma unroll 2
            for (int j4 = 0; j4 < CL_TC / 4; j4++) {
                float4 w4[4];
#pragma unroll
                for (int r = 0; r < 4; r++) w4[r] = *reinterpret_cast<const float4*>(w_s + (ty + 8 * r) * CL_LD + 4 * j4);
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const float4 f = *reinterpret_cast<const float4*>(c_s + (4 * j4 + jj) * CL_LD + 4 * tx);
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float w = jj == 0 ? w4[r].x : (jj == 1 ? w4[r].y : (jj == 2 ? w4[r].z : w4[r].w));
                        acc[kc][r].x = fmaf(w, f.x, acc[kc][r].x);
                        acc[kc][r].y = fmaf(w, f.y, acc[kc][r].y);
                        acc[kc][r].z = fmaf(w, f.z, acc[kc][r].z);
                        acc[kc][r].w = fmaf(w, f.w, acc[kc][r].w);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) osum[r] += __shfl_xor(osum[r], o, RG_WAVE);
        const int row = r_base + ty + 8 * r;
        if (row >= r1) continue;
#pragma unroll
        for (int kc = 0; kc < NK; kc++) {
            const float4 f = *reinterpret_cast<const float4*>(rf + (size_t)row * ldr + kc * CL_KC + 4 * tx);
            float4 o4;
            o4.x = __fsub_rn(__fmul_rn(osum[r], f.x), acc[kc][r].x);
            o4.y = __fsub_rn(__fmul_rn(osum[r], f.y), acc[kc][r].y);
            o4.z = __fsub_rn(__fmul_rn(osum[r], f.z), acc[kc][r].z);
            o4.w = __fsub_rn(__fmul_rn(osum[r], f.w), acc[kc][r].w);
            *reinterpret_cast<float4*>(out + (size_t)row * ldo + kc * CL_KC + 4 * tx) = o4;
        }
    }
}

int circle_tiles(int max_rows) { return max_rows > 0 ? rg_cdiv(max_rows, CL_TR) : 1; }

template <int D>
int launch_circle_fwd(const CirArgs& g, int tiles_anc, int tiles_pos, hipStream_t s)
{
    k_circle_fwd<D, true><<<dim3(tiles_anc, g.n_pairs), CL_THREADS, 0, s>>>(g);
    if (hipGetLastError() != hipSuccess) return RG_ERR_LAUNCH;
    k_circle_fwd<D, false><<<dim3(tiles_pos, g.n_pairs), CL_THREADS, 0, s>>>(g);
    return hipGetLastError() == hipSuccess ? RG_OK : RG_ERR_LAUNCH;
}

template <int D>
int launch_circle_bwd(const CirArgs& g, int tiles_anc, int tiles_pos, hipStream_t s)
{
    k_circle_bwd<D, true><<<dim3(tiles_anc, g.n_pairs), CL_THREADS, 0, s>>>(g);
    if (hipGetLastError() != hipSuccess) return RG_ERR_LAUNCH;
    k_circle_bwd<D, false><<<dim3(tiles_pos, g.n_pairs), CL_THREADS, 0, s>>>(g);
    return hipGetLastError() == hipSuccess ? RG_OK : RG_ERR_LAUNCH;
}

// what both entry points refuse
bool circle_args_bad(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                     const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int max_pos, int D)
{
    if (D <= 0 || D % 64 != 0 || D > 512) return true;
    if (n_pairs < 0 || n_anc < 0 || n_pos < 0 || max_anc < 0 || max_pos < 0) return true;
    if (n_anc > 0 && (!anc || !anc_xyz)) return true;
    if (n_pos > 0 && (!pos || !pos_xyz)) return true;
    if (n_pairs > 0 && (!anc_seg_off || !pos_seg_off)) return true;
    if (ld_anc < D || ld_pos < D || ld_anc % 4 != 0 || ld_pos % 4 != 0) return true;
    return ((uintptr_t)anc | (uintptr_t)pos) % 16 != 0;
}

}  // namespace

extern "C" {

int regtr_circle_rows(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                      const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int max_pos, int D,
                      float r_p, float r_n, float log_scale, float pos_margin, float pos_optimal, float neg_margin, float neg_optimal,
                      const float* anc_pose, float* pair_out, float* anc_lse, float* anc_sel, float* pos_lse, float* pos_sel,
                      void* stream)
{
    if (circle_args_bad(anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos, max_anc, max_pos, D))
        return RG_ERR_ARG;
    if (n_anc > 0 && (!anc_lse || !anc_sel)) return RG_ERR_ARG;
    if (n_pos > 0 && (!pos_lse || !pos_sel)) return RG_ERR_ARG;
    if (n_pairs > 0 && !pair_out) return RG_ERR_ARG;
    if (!(log_scale > 0.f)) return RG_ERR_ARG;
    if (n_pairs == 0) return RG_OK;
    CirArgs g{anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos,
              r_p, r_n, log_scale, pos_margin, pos_optimal, neg_margin, neg_optimal, anc_pose, anc_lse, anc_sel, pos_lse, pos_sel,
              nullptr, nullptr, 1.f, nullptr, 0, nullptr, 0};
    const hipStream_t s = (hipStream_t)stream;
    const int ta = circle_tiles(max_anc), tp = circle_tiles(max_pos);
    int rc = RG_ERR_ARG;
    switch (D) {
    case 64: rc = launch_circle_fwd<64>(g, ta, tp, s); break;
    case 128: rc = launch_circle_fwd<128>(g, ta, tp, s); break;
    case 192: rc = launch_circle_fwd<192>(g, ta, tp, s); break;
    case 256: rc = launch_circle_fwd<256>(g, ta, tp, s); break;
    case 320: rc = launch_circle_fwd<320>(g, ta, tp, s); break;
    case 384: rc = launch_circle_fwd<384>(g, ta, tp, s); break;
    case 448: rc = launch_circle_fwd<448>(g, ta, tp, s); break;
    case 512: rc = launch_circle_fwd<512>(g, ta, tp, s); break;
    }
    if (rc != RG_OK) return rc;
    k_circle_reduce<<<n_pairs, CR_THREADS, 0, s>>>(g, max_anc, max_pos, pair_out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_circle_bwd(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                     const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int max_pos, int D,
                     float r_p, float r_n, float log_scale, float pos_margin, float pos_optimal, float neg_margin, float neg_optimal,
                     const float* anc_pose, const float* anc_lse, const float* anc_sel, const float* pos_lse, const float* pos_sel,
                     const float* pair_out, const float* grad, float mean_div, float* d_anc, int ld_danc, float* d_pos, int ld_dpos,
                     void* stream)
{
    if (circle_args_bad(anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos, max_anc, max_pos, D))
        return RG_ERR_ARG;
    if (n_anc > 0 && (!anc_lse || !anc_sel || !d_anc)) return RG_ERR_ARG;
    if (n_pos > 0 && (!pos_lse || !pos_sel || !d_pos)) return RG_ERR_ARG;
    if (n_pairs > 0 && (!pair_out || !grad)) return RG_ERR_ARG;
    if (ld_danc < D || ld_dpos < D || ld_danc % 4 != 0 || ld_dpos % 4 != 0) return RG_ERR_ARG;
    if (((uintptr_t)d_anc | (uintptr_t)d_pos) % 16 != 0) return RG_ERR_ARG;
    if (!(mean_div > 0.f) || !(log_scale > 0.f)) return RG_ERR_ARG;
    if (n_pairs == 0) return RG_OK;
    CirArgs g{anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos,
              r_p, r_n, log_scale, pos_margin, pos_optimal, neg_margin, neg_optimal, anc_pose,
              const_cast<float*>(anc_lse), const_cast<float*>(anc_sel), const_cast<float*>(pos_lse), const_cast<float*>(pos_sel),
              pair_out, grad, mean_div, d_anc, ld_danc, d_pos, ld_dpos};
    const hipStream_t s = (hipStream_t)stream;
    const int ta = circle_tiles(max_anc), tp = circle_tiles(max_pos);
    switch (D) {
    case 64: return launch_circle_bwd<64>(g, ta, tp, s);
    case 128: return launch_circle_bwd<128>(g, ta, tp, s);
    case 192: return launch_circle_bwd<192>(g, ta, tp, s);
    case 256: return launch_circle_bwd<256>(g, ta, tp, s);
    case 320: return launch_circle_bwd<320>(g, ta, tp, s);
    case 384: return launch_circle_bwd<384>(g, ta, tp, s);
    case 448: return launch_circle_bwd<448>(g, ta, tp, s);
    case 512: return launch_circle_bwd<512>(g, ta, tp, s);
    }
    return RG_ERR_ARG;
}

}  // extern "C"
