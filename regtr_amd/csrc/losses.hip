// Losses of RegTR.compute_loss (models/regtr.py:237-294) for gfx950, and the backward of the training-loss drop-ins
// (regtr_amd/losses.py: InfoNCELossFull, CorrCriterion).
//
// regtr_infonce -- InfoNCELossFull.compute_infonce (models/losses/feature_loss.py:281-314) over packed, ragged pairs.  The reference
// materialises an [N_anc x N_pos] logit matrix and a cdist per pair; here it is one attention-shaped pass over the pair's targets:
//   * one workgroup = 2 waves = 32 anchor rows of one pair (TR); wave w owns rows 16 w .. 16 w + 15 and keeps its A fragment of
//     v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation) in registers: lane l holds A[row l & 15][k = (l >> 4) DQ + s],
//     s < DQ = D / 4 -- the K order is permuted so that every operand load is a float4;
//   * the targets stream through LDS in tiles of TJ rows (32, or 16 at D = 512: 33 KB either way, rows padded by 4 floats so the
//     16 rows of one ds_read_b128 hit 16 distinct bank quads), both waves reading the same tile;
//   * per 16 x 16 logit block each lane owns rows 4 (l >> 4) + r, column l & 15 (the C/D map) and folds them into per-row running
//     state: (max, sum) of exp over the targets with d >= r_n, and the current argmin (distance, index, logit).  The argmin's logit
//     is added to the sum at the end only if d* < r_n -- otherwise it is already in it.  Ties of d keep the lowest j (a lane sees its
//     columns in increasing order; the cross-lane merge is lexicographic on (d, j)), which torch's topk leaves unspecified.
//   Occupancy: a 64-pair 3DMatch forward has ~394 src tokens per pair -> 13 tiles x 64 pairs = 832 workgroups of 2 waves on 1024
//   SIMDs; 33 KB of LDS allows 4 workgroups per CU, so the whole problem is resident in one wave of the grid.  64-row tiles would
//   leave ~450 workgroups for 256 CUs.
//   Determinism: every workgroup writes its (sum, count) partial to its own workspace slot; a second launch sums the slots of a pair
//   in tile order.  No float atomics.
//
// regtr_se3_transform -- x' = R x + t per point of packed clouds, rounded per operation (the GT-pose transform of the overlap masks).
//
// regtr_loss_terms -- the O(N) terms: BCE-with-logits sums against the GT overlap pyramid (regtr.py:250-257) and the weighted L1
// correspondence sums of CorrCriterion (corr_loss.py:18-40) in both directions, one workgroup per pair, float64 sums, fixed-order
// reductions.
//
// Compiled with -ffp-contract=off (regtr_amd/build.py): the distances and pose transforms are rounded per operation as restated.
#include <math.h>

#include "common.h"
#include "loss_common.h"      // lse_merge, transform_rn, coord_dist_rn, pair_ok: shared with circle_loss.hip

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int IN_TR = 32;          // anchor rows per workgroup
constexpr int IN_THREADS = 128;    // 2 waves x 16 rows

struct InfArgs {
    const float* anc; int lda;
    const float* pos; int ldp;
    const float* anc_xyz; const float* pos_xyz;
    const int* anc_off; const int* pos_off;
    int n_pairs, n_anc, n_pos, n_tiles;
    float r_p, r_n;
    const float* pose;
    float* row_loss; float* row_mask;
    double* part;                  // [n_pairs][n_tiles][2]
    float* row_lse; int* row_idx;  // optional: the decisions the backward reuses (regtr_infonce_rows)
};

// running state of one anchor row over a set of targets
struct RowState {
    float m, s;                    // max and sum of exp(l - m) over the targets with d >= r_n (or NaN distance)
    float dmin, lstar;             // current argmin distance and its logit
    int jmin;                      // its target index (-1: none seen)
};

__device__ __forceinline__ void row_merge(RowState& a, const RowState& b)
{
    lse_merge(a.m, a.s, b.m, b.s);
    // lexicographic (d, j): lowest j among equal distances; an empty side (jmin -1) never wins
    const bool take = b.jmin >= 0 && (a.jmin < 0 || b.dmin < a.dmin || (b.dmin == a.dmin && b.jmin < a.jmin));
    if (take) { a.dmin = b.dmin; a.lstar = b.lstar; a.jmin = b.jmin; }
}

__device__ __forceinline__ RowState row_shfl_xor(const RowState& a, int o)
{
    RowState b;
    b.m = __shfl_xor(a.m, o, RG_WAVE);
    b.s = __shfl_xor(a.s, o, RG_WAVE);
    b.dmin = __shfl_xor(a.dmin, o, RG_WAVE);
    b.lstar = __shfl_xor(a.lstar, o, RG_WAVE);
    b.jmin = __shfl_xor(a.jmin, o, RG_WAVE);
    return b;
}

template <int D>
__global__ __launch_bounds__(IN_THREADS) void k_infonce(InfArgs g)
{
    constexpr int DQ = D / 4;                  // k values per lane group
    constexpr int TJ = D <= 256 ? 32 : 16;     // targets per LDS tile
    constexpr int NB = TJ / 16;                // 16-column logit blocks per tile
    constexpr int LDP = D + 4;                 // padded LDS row
    __shared__ __attribute__((aligned(16))) float p_s[TJ * LDP];
    __shared__ float pxyz_s[TJ * 3];
    __shared__ float rl_s[IN_TR];
    __shared__ int rm_s[IN_TR];

    const int tile = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, grp = lane >> 4;
    double* part = g.part + ((size_t)b * g.n_tiles + tile) * 2;

    int a0, a1, p0, p1;
    if (!pair_ok(g.anc_off, b, g.n_anc, a0, a1) || !pair_ok(g.pos_off, b, g.n_pos, p0, p1)) {
        if (tid == 0) { part[0] = NAN; part[1] = 0.0; }          // the reducer reports the pair as NaN
        return;
    }
    const int r_base = a0 + tile * IN_TR;
    if (r_base >= a1) {                                          // (uniform over the workgroup: before any barrier)
        if (tid == 0) { part[0] = 0.0; part[1] = 0.0; }
        return;
    }

    // ---- A fragment: row r_base + 16 wave + col, k = grp DQ + s
    float a[DQ];
    {
        const int row = r_base + 16 * wave + col;
        const bool ok = row < a1;
        const float4* src = reinterpret_cast<const float4*>(g.anc + (size_t)(ok ? row : a0) * g.lda + grp * DQ);
#pragma unroll
        for (int t = 0; t < DQ / 4; t++) {
            const float4 v = ok ? src[t] : make_float4(0.f, 0.f, 0.f, 0.f);
            a[4 * t] = v.x; a[4 * t + 1] = v.y; a[4 * t + 2] = v.z; a[4 * t + 3] = v.w;
        }
    }
    // ---- coordinates of the 4 rows this lane owns in the C/D map: 16 wave + 4 grp + r
    float ax[4][3];
    RowState st[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = r_base + 16 * wave + 4 * grp + r;
        const int rr = row < a1 ? row : a0;
        const float x = g.anc_xyz[3 * (size_t)rr], y = g.anc_xyz[3 * (size_t)rr + 1], z = g.anc_xyz[3 * (size_t)rr + 2];
        if (g.pose) {
            transform_rn(g.pose + 12 * (size_t)b, x, y, z, ax[r]);
        } else {
            ax[r][0] = x; ax[r][1] = y; ax[r][2] = z;
        }
        st[r].m = -INFINITY; st[r].s = 0.f; st[r].dmin = INFINITY; st[r].lstar = 0.f; st[r].jmin = -1;
    }

    const float r_p = g.r_p, r_n = g.r_n;
    for (int jt = p0; jt < p1; jt += TJ) {
        __syncthreads();                                         // the previous tile is consumed
        for (int idx = tid; idx < TJ * (D / 4); idx += IN_THREADS) {
            const int jj = idx / (D / 4), c4 = idx - jj * (D / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (jt + jj < p1) v = reinterpret_cast<const float4*>(g.pos + (size_t)(jt + jj) * g.ldp)[c4];
            *reinterpret_cast<float4*>(p_s + jj * LDP + 4 * c4) = v;
        }
        if (tid < TJ * 3) pxyz_s[tid] = (jt + tid / 3 < p1) ? g.pos_xyz[3 * (size_t)jt + tid] : 0.f;
        __syncthreads();

        floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
        if constexpr (NB == 2) {               // two independent chains: one per 16-column block
            const float* pr0 = p_s + col * LDP + grp * DQ;
            const float* pr1 = pr0 + 16 * LDP;
#pragma unroll
            for (int t = 0; t < DQ / 4; t++) {
                const float4 b0 = *reinterpret_cast<const float4*>(pr0 + 4 * t);
                const float4 b1 = *reinterpret_cast<const float4*>(pr1 + 4 * t);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t], b0.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t], b1.x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 1], b0.y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 1], b1.y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 2], b0.z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 2], b1.z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 3], b0.w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 3], b1.w, acc[1], 0, 0, 0);
            }
        } else {                               // one block: the K range split over two chains, summed once
            const float* pr0 = p_s + col * LDP + grp * DQ;
#pragma unroll
            for (int t = 0; t < DQ / 4; t++) {
                const float4 b0 = *reinterpret_cast<const float4*>(pr0 + 4 * t);
                floatx4& c = acc[t & 1];
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t], b0.x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 1], b0.y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 2], b0.z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 3], b0.w, c, 0, 0, 0);
            }
            acc[0] = acc[0] + acc[1];
        }

#pragma unroll
        for (int c = 0; c < NB; c++) {
            const int jj = 16 * c + col, j = jt + jj;
            if (j >= p1) continue;
            const float px = pxyz_s[3 * jj], py = pxyz_s[3 * jj + 1], pz = pxyz_s[3 * jj + 2];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float l = acc[c][r];
                const float d = coord_dist_rn(ax[r][0], ax[r][1], ax[r][2], px, py, pz);
                if (d < st[r].dmin) { st[r].dmin = d; st[r].lstar = l; st[r].jmin = j; }   // strict: the lowest j keeps a tie
                if (!(d < r_n)) {
                    if (l > st[r].m) { st[r].s = st[r].s * expf(st[r].m - l) + 1.f; st[r].m = l; }
                    else st[r].s += expf(l - st[r].m);
                }
            }
        }
    }

    // ---- merge the 16 column lanes of each row (xor within the lane group: commutative merge, every lane gets the same state)
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const RowState other = row_shfl_xor(st[r], o);
            row_merge(st[r], other);
        }
    }
    if (col == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int lr = 16 * wave + 4 * grp + r, row = r_base + lr;
            float loss = NAN;
            int mask = 0;
            float lse = NAN;
            if (st[r].jmin >= 0) {
                float m = st[r].m, s = st[r].s;
                if (st[r].dmin < r_n) lse_merge(m, s, st[r].lstar, 1.f);
                lse = __fadd_rn(m, logf(s));
                loss = __fsub_rn(lse, st[r].lstar);
                mask = st[r].dmin < r_p;
            }
            const bool valid = row < a1;
            rl_s[lr] = loss;
            rm_s[lr] = valid ? mask : 0;
            if (valid) {
                if (g.row_loss) g.row_loss[row] = loss;
                if (g.row_mask) g.row_mask[row] = (float)mask;
                if (g.row_lse) g.row_lse[row] = lse;
                if (g.row_idx) g.row_idx[row] = st[r].jmin;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0, cnt = 0.0;
        for (int i = 0; i < IN_TR; i++)
            if (rm_s[i]) { sum += (double)rl_s[i]; cnt += 1.0; }
        part[0] = sum;
        part[1] = cnt;
    }
}

__global__ void k_infonce_reduce(const double* __restrict__ part, const int* __restrict__ anc_off, const int* __restrict__ pos_off,
                                 int n_pairs, int n_anc, int n_pos, int n_tiles, float* __restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_pairs) return;
    int a0, a1, p0, p1;
    double sum = 0.0, cnt = 0.0;
    if (!pair_ok(anc_off, b, n_anc, a0, a1) || !pair_ok(pos_off, b, n_pos, p0, p1) || a1 - a0 > n_tiles * IN_TR) {
        sum = NAN;
    } else {
        for (int t = 0; t < n_tiles; t++) {
            sum += part[((size_t)b * n_tiles + t) * 2];
            cnt += part[((size_t)b * n_tiles + t) * 2 + 1];
        }
    }
    out[2 * b] = (float)sum;
    out[2 * b + 1] = (float)cnt;
}

template <int D>
int launch_infonce(const InfArgs& g, hipStream_t s)
{
    k_infonce<D><<<dim3(g.n_tiles, g.n_pairs), IN_THREADS, 0, s>>>(g);
    return hipGetLastError() == hipSuccess ? RG_OK : RG_ERR_LAUNCH;
}

// ---------------------------------------------------------------------------------------------------------------- O(N) terms
constexpr int LT_THREADS = 256;

__global__ __launch_bounds__(LT_THREADS) void k_loss_terms(const float* __restrict__ logit, const float* __restrict__ gt,
                                                           const float* __restrict__ kp, const float* __restrict__ warped,
                                                           const int* __restrict__ seg_off, int n_pairs, int n_total,
                                                           const float* __restrict__ pose, int pose_stride, float* __restrict__ out)
{
    __shared__ double sh[LT_THREADS / RG_WAVE];
    const int b = blockIdx.x;
    int s0, s1, t0, t1;
    if (!pair_ok(seg_off, b, n_total, s0, s1) || !pair_ok(seg_off, n_pairs + b, n_total, t0, t1)) {
        if (threadIdx.x == 0)
            for (int k = 0; k < 5; k++) out[5 * b + k] = NAN;
        return;
    }
    // T (src -> tgt) and T^-1 = [R^T | -R^T t], rounded per operation
    const float* P = pose + (size_t)b * pose_stride;
    float T[12], Ti[12];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) T[4 * r + c] = P[4 * r + c];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Ti[4 * r + c] = T[4 * c + r];
        Ti[4 * r + 3] = -__fadd_rn(__fadd_rn(__fmul_rn(T[r], T[3]), __fmul_rn(T[4 + r], T[7])), __fmul_rn(T[8 + r], T[11]));
    }

    double bce = 0.0, err[2] = {0.0, 0.0}, wsum[2] = {0.0, 0.0};
    for (int side = 0; side < 2; side++) {
        const int lo = side ? t0 : s0, hi = side ? t1 : s1;
        const float* M = side ? Ti : T;
        for (int i = lo + threadIdx.x; i < hi; i += LT_THREADS) {
            const double x = logit[i], y = gt[i];
            bce += fmax(x, 0.0) - x * y + log1p(exp(-fabs(x)));
            float w3[3];
            transform_rn(M, kp[3 * (size_t)i], kp[3 * (size_t)i + 1], kp[3 * (size_t)i + 2], w3);
            const float e = __fadd_rn(__fadd_rn(fabsf(__fsub_rn(warped[3 * (size_t)i], w3[0])), fabsf(__fsub_rn(warped[3 * (size_t)i + 1], w3[1]))),
                                      fabsf(__fsub_rn(warped[3 * (size_t)i + 2], w3[2])));
            const float w = gt[i];
            err[side] += (double)__fmul_rn(w, e);
            wsum[side] += (double)w;
        }
    }
    const double v0 = rg_block_sum<LT_THREADS>(bce, sh), v1 = rg_block_sum<LT_THREADS>(err[0], sh), v2 = rg_block_sum<LT_THREADS>(wsum[0], sh);
    const double v3 = rg_block_sum<LT_THREADS>(err[1], sh), v4 = rg_block_sum<LT_THREADS>(wsum[1], sh);
    if (threadIdx.x == 0) {
        out[5 * b] = (float)v0; out[5 * b + 1] = (float)v1; out[5 * b + 2] = (float)v2;
        out[5 * b + 3] = (float)v3; out[5 * b + 4] = (float)v4;
    }
}

__global__ void k_se3_transform(const float* __restrict__ xyz, const int* __restrict__ seg_off, int n_clouds, int n,
                                const float* __restrict__ pose, int pose_stride, float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_clouds;                 // the cloud c with seg_off[c] <= i < seg_off[c + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= i) lo = mid; else hi = mid;
    }
    float T[12], o[3];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = pose[(size_t)lo * pose_stride + e];
    transform_rn(T, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], o);
    out[3 * (size_t)i] = o[0]; out[3 * (size_t)i + 1] = o[1]; out[3 * (size_t)i + 2] = o[2];
}

// ---------------------------------------------------------------------------------------------------------------- backward
// regtr_infonce_bwd: the forward's decisions (LSE_i, j*_i, mask_i saved by regtr_infonce_rows) and the upstream scale per pair
// s_b = (g / mean_div) / count_b (read on the device) give dl_ij = s_b p_ij - s_b [j = j*_i], p_ij = exp(l_ij - LSE_i) over the
// allowed set {d_ij >= r_n} u {j*_i}, 0 elsewhere and on unmasked rows.  Attention-backward shaped, two launches of one template:
//   ANC_ROWS: a workgroup owns 32 anchor rows of a pair and sweeps the pair's positives -> dA_i = sum_j dl_ij P'_j;
//   else:     a workgroup owns 32 positive rows of a pair and sweeps the pair's anchors -> dP'_j = sum_i dl_ij A_i.
// Every output row has exactly one owner: no cross-workgroup sum, no atomics, bit-reproducible.  Per streamed tile of 16 columns the
// logits are recomputed by the forward's MFMA chain (same K order), dl goes through LDS from the C/D map into the A-operand map,
// and a second v_mfma_f32_16x16x4_f32 chain accumulates dl (16 x 16) x F (16 x D) into D / 16 accumulators per lane.
constexpr int BW_TC = 16;          // streamed columns per tile

struct InfBwdArgs {
    const float* anc; int lda;
    const float* pos; int ldp;
    const float* anc_xyz; const float* pos_xyz;
    const int* anc_off; const int* pos_off;
    int n_pairs, n_anc, n_pos, n_tiles;
    float r_n;
    const float* pose;
    const float* row_lse; const int* row_idx; const float* row_mask;
    const float* pair_out; const float* grad; float mean_div;
    float* out; int ldo;
};

template <int D, bool ANC_ROWS>
__global__ __launch_bounds__(IN_THREADS) void k_infonce_bwd(InfBwdArgs g)
{
    constexpr int DQ = D / 4;
    constexpr int LDP = D + 4;
    constexpr int NO = D / 16;                 // 16-column output blocks
    __shared__ __attribute__((aligned(16))) float f_s[BW_TC * LDP];
    __shared__ float cxyz_s[BW_TC * 3];
    __shared__ float clse_s[BW_TC];
    __shared__ int cidx_s[BW_TC];
    __shared__ int cmsk_s[BW_TC];
    __shared__ float dl_s[2][16][17];

    const int tile = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, grp = lane >> 4;

    int a0, a1, p0, p1;
    if (!pair_ok(g.anc_off, b, g.n_anc, a0, a1) || !pair_ok(g.pos_off, b, g.n_pos, p0, p1)) return;
    const int r0 = ANC_ROWS ? a0 : p0, r1 = ANC_ROWS ? a1 : p1;      // owned rows
    const int c0 = ANC_ROWS ? p0 : a0, c1 = ANC_ROWS ? p1 : a1;      // streamed columns
    const int r_base = r0 + tile * IN_TR;
    if (r_base >= r1) return;                                        // (uniform: before any barrier)
    const float* rf = ANC_ROWS ? g.anc : g.pos;
    const int ldr = ANC_ROWS ? g.lda : g.ldp;
    const float* cf = ANC_ROWS ? g.pos : g.anc;
    const int ldc = ANC_ROWS ? g.ldp : g.lda;
    const float* pose = g.pose ? g.pose + 12 * (size_t)b : nullptr;
    const float s = __fdiv_rn(__fdiv_rn(g.grad[0], g.mean_div), g.pair_out[2 * b + 1]);   // used on masked rows only (count >= 1)

    // ---- row fragment (the forward's A operand layout)
    float a[DQ];
    {
        const int row = r_base + 16 * wave + col;
        const bool ok = row < r1;
        const float4* src = reinterpret_cast<const float4*>(rf + (size_t)(ok ? row : r0) * ldr + grp * DQ);
#pragma unroll
        for (int t = 0; t < DQ / 4; t++) {
            const float4 v = ok ? src[t] : make_float4(0.f, 0.f, 0.f, 0.f);
            a[4 * t] = v.x; a[4 * t + 1] = v.y; a[4 * t + 2] = v.z; a[4 * t + 3] = v.w;
        }
    }
    // ---- the 4 C/D-map rows of this lane: coordinates (anchors with the pose applied), and the anchor rows' decisions
    float rx[4][3], rlse[4];
    int ridx[4];
    bool rok[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = r_base + 16 * wave + 4 * grp + r;
        rok[r] = row < r1;
        const int rr = rok[r] ? row : r0;
        const float* xyz = (ANC_ROWS ? g.anc_xyz : g.pos_xyz) + 3 * (size_t)rr;
        if (ANC_ROWS && pose) {
            transform_rn(pose, xyz[0], xyz[1], xyz[2], rx[r]);
        } else {
            rx[r][0] = xyz[0]; rx[r][1] = xyz[1]; rx[r][2] = xyz[2];
        }
        rlse[r] = 0.f; ridx[r] = -1;
        if (ANC_ROWS) {
            rlse[r] = g.row_lse[rr];
            ridx[r] = g.row_idx[rr];
            rok[r] = rok[r] && g.row_mask[rr] != 0.f;
        }
    }

    floatx4 o[NO];
#pragma unroll
    for (int n = 0; n < NO; n++) o[n] = floatx4{0.f, 0.f, 0.f, 0.f};

    const float r_n = g.r_n;
    for (int ct = c0; ct < c1; ct += BW_TC) {
        __syncthreads();                                             // the previous tile is consumed
        for (int idx = tid; idx < BW_TC * (D / 4); idx += IN_THREADS) {
            const int jj = idx / (D / 4), c4 = idx - jj * (D / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ct + jj < c1) v = reinterpret_cast<const float4*>(cf + (size_t)(ct + jj) * ldc)[c4];
            *reinterpret_cast<float4*>(f_s + jj * LDP + 4 * c4) = v;
        }
        if (tid < BW_TC) {
            const int c = ct + tid;
            float x = 0.f, y = 0.f, z = 0.f, lse = 0.f;
            int ci = -1, cm = 0;
            if (c < c1) {
                const float* xyz = (ANC_ROWS ? g.pos_xyz : g.anc_xyz) + 3 * (size_t)c;
                x = xyz[0]; y = xyz[1]; z = xyz[2];
                if (!ANC_ROWS) {
                    if (pose) {
                        float t3[3];
                        transform_rn(pose, x, y, z, t3);
                        x = t3[0]; y = t3[1]; z = t3[2];
                    }
                    lse = g.row_lse[c];
                    ci = g.row_idx[c];
                    cm = g.row_mask[c] != 0.f;
                }
            }
            cxyz_s[3 * tid] = x; cxyz_s[3 * tid + 1] = y; cxyz_s[3 * tid + 2] = z;
            clse_s[tid] = lse; cidx_s[tid] = ci; cmsk_s[tid] = cm;
        }
        __syncthreads();

        // logits of this wave's 16 rows x the 16 columns: the forward's chain (one sequential chain up to D = 256, two summed above)
        floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
        {
            const float* pr = f_s + col * LDP + grp * DQ;
#pragma unroll
            for (int t = 0; t < DQ / 4; t++) {
                const float4 bv = *reinterpret_cast<const float4*>(pr + 4 * t);
                floatx4& c = acc[D <= 256 ? 0 : (t & 1)];
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t], bv.x, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 1], bv.y, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 2], bv.z, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * t + 3], bv.w, c, 0, 0, 0);
            }
            if (D > 256) acc[0] = acc[0] + acc[1];
        }
        // dl in the C/D map -> LDS
        {
            const int c = ct + col;
            const float cx = cxyz_s[3 * col], cy = cxyz_s[3 * col + 1], cz = cxyz_s[3 * col + 2];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = r_base + 16 * wave + 4 * grp + r;
                const bool on = c < c1 && (ANC_ROWS ? rok[r] : (rok[r] && cmsk_s[col]));
                float v = 0.f;
                if (on) {
                    // d_ij with the anchor first, as the forward computes it
                    const float* ap = ANC_ROWS ? rx[r] : &cxyz_s[3 * col];
                    const float px = ANC_ROWS ? cx : rx[r][0], py = ANC_ROWS ? cy : rx[r][1], pz = ANC_ROWS ? cz : rx[r][2];
                    const float d = coord_dist_rn(ap[0], ap[1], ap[2], px, py, pz);
                    const int j = ANC_ROWS ? c : row;
                    const int jstar = ANC_ROWS ? ridx[r] : cidx_s[col];
                    const float lse = ANC_ROWS ? rlse[r] : clse_s[col];
                    const bool positive = j == jstar;
                    if (positive || !(d < r_n)) v = __fmul_rn(s, expf(__fsub_rn(acc[0][r], lse)));
                    if (positive) v = __fsub_rn(v, s);
                }
                dl_s[wave][4 * grp + r][col] = v;
            }
        }
        __syncthreads();
        // out (16 rows x D) += dl (16 x 16, A operand: lane -> dl[l & 15][k = 4 kb + (l >> 4)]) x F (16 x D)
#pragma unroll
        for (int kb = 0; kb < 4; kb++) {
            const float av = dl_s[wave][col][4 * kb + grp];
            const float* fr = f_s + (4 * kb + grp) * LDP + col;
#pragma unroll
            for (int n = 0; n < NO; n++) o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, fr[16 * n], o[n], 0, 0, 0);
        }
    }

#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = r_base + 16 * wave + 4 * grp + r;
        if (row >= r1) continue;
        float* dst = g.out + (size_t)row * g.ldo + col;
#pragma unroll
        for (int n = 0; n < NO; n++) dst[16 * n] = o[n][r];
    }
}

template <int D>
int launch_infonce_bwd(InfBwdArgs ga, InfBwdArgs gp, int tiles_anc, int tiles_pos, hipStream_t s)
{
    k_infonce_bwd<D, true><<<dim3(tiles_anc, ga.n_pairs), IN_THREADS, 0, s>>>(ga);
    if (hipGetLastError() != hipSuccess) return RG_ERR_LAUNCH;
    k_infonce_bwd<D, false><<<dim3(tiles_pos, gp.n_pairs), IN_THREADS, 0, s>>>(gp);
    return hipGetLastError() == hipSuccess ? RG_OK : RG_ERR_LAUNCH;
}

// regtr_gemm_tn: C = A^T B over a tall K (rows of A [M, N1] and B [M, N2]), exact-f32 MFMA.  Split-K: workgroup (tm, tn, z) sums
// rows [z chunk, (z + 1) chunk) of one 64 x 64 tile into its own partial slot; a second launch sums the slots in z order (float64)
// and optionally folds the result into InfoNCELossFull's dW (dW_ij = C_ij + C_ji above the diagonal, 2 C_ii on it, 0 below).  The
// split depends on (M, N1, N2) only: bit-reproducible.
constexpr int TN_TILE = 64, TN_THREADS = 256;

__global__ __launch_bounds__(TN_THREADS) void k_gemm_tn_part(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                             int M, int N1, int N2, int chunk, float* __restrict__ part)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, grp = lane >> 4;
    const int m0 = TN_TILE * blockIdx.x + 16 * wave, n0 = TN_TILE * blockIdx.y;
    const int k0 = blockIdx.z * chunk, k1 = min(M, k0 + chunk);
    floatx4 acc[4] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 4
    for (int k = k0; k < k1; k += 4) {
        const int kk = k + grp;
        const bool ok = kk < k1;
        const float av = ok ? A[(size_t)kk * lda + m0 + col] : 0.f;
        const float* br = B + (size_t)(ok ? kk : k0) * ldb + n0 + col;
#pragma unroll
        for (int n = 0; n < 4; n++) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, ok ? br[16 * n] : 0.f, acc[n], 0, 0, 0);
    }
    float* dst = part + (size_t)blockIdx.z * N1 * N2;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int n = 0; n < 4; n++) dst[(size_t)(m0 + 4 * grp + r) * N2 + n0 + 16 * n + col] = acc[n][r];
}

__global__ void k_gemm_tn_reduce(const float* __restrict__ part, int splits, int N1, int N2, int fold, float* __restrict__ out, int ldo)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N1 * N2) return;
    const int i = idx / N2, j = idx - i * N2;
    const size_t plane = (size_t)N1 * N2;
    double v = 0.0;
    if (!fold || i <= j)
        for (int z = 0; z < splits; z++) v += part[z * plane + (size_t)i * N2 + j];
    if (fold) {
        if (i > j) {
            v = 0.0;
        } else if (i == j) {
            v = 2.0 * v;
        } else {
            double t = 0.0;
            for (int z = 0; z < splits; z++) t += part[z * plane + (size_t)j * N2 + i];
            v = (double)((float)v + (float)t);
        }
    }
    out[(size_t)i * ldo + j] = (float)v;
}

int gemm_tn_splits(int M, int N1, int N2, int& chunk)
{
    const int tiles = (N1 / TN_TILE) * (N2 / TN_TILE);
    const int target = tiles > 0 ? rg_cdiv(2048, tiles) : 1;
    chunk = rg_cdiv(rg_cdiv(M > 0 ? M : 1, target), 4) * 4;
    if (chunk < 64) chunk = 64;
    return M > 0 ? rg_cdiv(M, chunk) : 1;
}

// regtr_corr_l1_bwd: d warped_ik = ((g / den) w_i) sgn(e_ik), e = warped - T kp rounded as regtr_loss_terms rounds it.
__global__ void k_corr_l1_bwd(const float* __restrict__ kp, const float* __restrict__ warped, const float* __restrict__ w,
                              const int* __restrict__ seg_off, int n_clouds, int n, const float* __restrict__ pose, int pose_stride,
                              const float* __restrict__ grad, const float* __restrict__ den, float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int lo = 0, hi = n_clouds;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= i) lo = mid; else hi = mid;
    }
    float T[12], t3[3];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = pose[(size_t)lo * pose_stride + e];
    transform_rn(T, kp[3 * (size_t)i], kp[3 * (size_t)i + 1], kp[3 * (size_t)i + 2], t3);
    const float sw = __fmul_rn(__fdiv_rn(grad[0], den[0]), w[i]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float e = __fsub_rn(warped[3 * (size_t)i + k], t3[k]);
        const float sg = e > 0.f ? 1.f : (e < 0.f ? -1.f : (e == 0.f ? 0.f : NAN));
        out[3 * (size_t)i + k] = __fmul_rn(sw, sg);
    }
}

int infonce_tiles(int max_anc) { return max_anc > 0 ? rg_cdiv(max_anc, IN_TR) : 1; }

}  // namespace

extern "C" {

size_t regtr_infonce_ws_bytes(int n_pairs, int max_anc)
{
    if (n_pairs < 0 || max_anc < 0) return 0;
    return (size_t)n_pairs * infonce_tiles(max_anc) * 2 * sizeof(double);
}

static int infonce_impl(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                        const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int D,
                        float r_p, float r_n, const float* anc_pose, float* pair_out, float* row_loss, float* row_mask, float* row_lse,
                        int* row_idx, void* ws, size_t ws_bytes, void* stream)
{
    if (D <= 0 || D % 64 != 0 || D > 512) return RG_ERR_ARG;
    if (n_pairs < 0 || n_anc < 0 || n_pos < 0 || max_anc < 0) return RG_ERR_ARG;
    if (n_anc > 0 && (!anc || !anc_xyz)) return RG_ERR_ARG;
    if (n_pos > 0 && (!pos || !pos_xyz)) return RG_ERR_ARG;
    if (n_pairs > 0 && (!anc_seg_off || !pos_seg_off || !pair_out || !ws)) return RG_ERR_ARG;
    if (ld_anc < D || ld_pos < D || ld_anc % 4 != 0 || ld_pos % 4 != 0) return RG_ERR_ARG;
    if (((uintptr_t)anc | (uintptr_t)pos) % 16 != 0) return RG_ERR_ARG;
    if (n_pairs == 0) return RG_OK;
    if (ws_bytes < regtr_infonce_ws_bytes(n_pairs, max_anc)) return RG_ERR_WORKSPACE;
    InfArgs g{anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos, infonce_tiles(max_anc),
              r_p, r_n, anc_pose, row_loss, row_mask, (double*)ws, row_lse, row_idx};
    const hipStream_t s = (hipStream_t)stream;
    int rc = RG_ERR_ARG;
    switch (D) {
    case 64: rc = launch_infonce<64>(g, s); break;
    case 128: rc = launch_infonce<128>(g, s); break;
    case 192: rc = launch_infonce<192>(g, s); break;
    case 256: rc = launch_infonce<256>(g, s); break;
    case 320: rc = launch_infonce<320>(g, s); break;
    case 384: rc = launch_infonce<384>(g, s); break;
    case 448: rc = launch_infonce<448>(g, s); break;
    case 512: rc = launch_infonce<512>(g, s); break;
    }
    if (rc != RG_OK) return rc;
    k_infonce_reduce<<<rg_cdiv(n_pairs, 256), 256, 0, s>>>((const double*)ws, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos,
                                                          g.n_tiles, pair_out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_infonce(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                  const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int D,
                  float r_p, float r_n, const float* anc_pose, float* pair_out, float* row_loss, float* row_mask, void* ws,
                  size_t ws_bytes, void* stream)
{
    return infonce_impl(anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos, max_anc, D, r_p,
                        r_n, anc_pose, pair_out, row_loss, row_mask, nullptr, nullptr, ws, ws_bytes, stream);
}

int regtr_infonce_rows(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                       const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int D,
                       float r_p, float r_n, const float* anc_pose, float* pair_out, float* row_loss, float* row_mask, float* row_lse,
                       int* row_idx, void* ws, size_t ws_bytes, void* stream)
{
    if (n_anc > 0 && (!row_mask || !row_lse || !row_idx)) return RG_ERR_ARG;
    return infonce_impl(anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos, max_anc, D, r_p,
                        r_n, anc_pose, pair_out, row_loss, row_mask, row_lse, row_idx, ws, ws_bytes, stream);
}

int regtr_infonce_bwd(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                      const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int max_pos,
                      int D, float r_n, const float* anc_pose, const float* row_lse, const int* row_idx, const float* row_mask,
                      const float* pair_out, const float* grad, float mean_div, float* d_anc, int ld_danc, float* d_pos, int ld_dpos,
                      void* stream)
{
    if (D <= 0 || D % 64 != 0 || D > 512) return RG_ERR_ARG;
    if (n_pairs < 0 || n_anc < 0 || n_pos < 0 || max_anc < 0 || max_pos < 0) return RG_ERR_ARG;
    if (n_anc > 0 && (!anc || !anc_xyz || !row_lse || !row_idx || !row_mask || !d_anc)) return RG_ERR_ARG;
    if (n_pos > 0 && (!pos || !pos_xyz || !d_pos)) return RG_ERR_ARG;
    if (n_pairs > 0 && (!anc_seg_off || !pos_seg_off || !pair_out || !grad)) return RG_ERR_ARG;
    if (ld_anc < D || ld_pos < D || ld_anc % 4 != 0 || ld_pos % 4 != 0 || ld_danc < D || ld_dpos < D) return RG_ERR_ARG;
    if (((uintptr_t)anc | (uintptr_t)pos) % 16 != 0 || !(mean_div > 0.f)) return RG_ERR_ARG;
    if (n_pairs == 0) return RG_OK;
    InfBwdArgs ga{anc, ld_anc, pos, ld_pos, anc_xyz, pos_xyz, anc_seg_off, pos_seg_off, n_pairs, n_anc, n_pos, infonce_tiles(max_anc),
                  r_n, anc_pose, row_lse, row_idx, row_mask, pair_out, grad, mean_div, d_anc, ld_danc};
    InfBwdArgs gp = ga;
    gp.n_tiles = infonce_tiles(max_pos);
    gp.out = d_pos;
    gp.ldo = ld_dpos;
    const hipStream_t s = (hipStream_t)stream;
    switch (D) {
    case 64: return launch_infonce_bwd<64>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    case 128: return launch_infonce_bwd<128>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    case 192: return launch_infonce_bwd<192>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    case 256: return launch_infonce_bwd<256>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    case 320: return launch_infonce_bwd<320>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    case 384: return launch_infonce_bwd<384>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    case 448: return launch_infonce_bwd<448>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    case 512: return launch_infonce_bwd<512>(ga, gp, ga.n_tiles, gp.n_tiles, s);
    }
    return RG_ERR_ARG;
}

size_t regtr_gemm_tn_ws_bytes(int M, int N1, int N2)
{
    if (M < 0 || N1 <= 0 || N2 <= 0 || N1 % TN_TILE != 0 || N2 % TN_TILE != 0) return 0;
    int chunk;
    return (size_t)gemm_tn_splits(M, N1, N2, chunk) * N1 * N2 * sizeof(float);
}

int regtr_gemm_tn(const float* a, int lda, const float* b, int ldb, int M, int N1, int N2, int fold, float* out, int ldo, void* ws,
                  size_t ws_bytes, void* stream)
{
    if (M < 0 || N1 <= 0 || N2 <= 0 || N1 % TN_TILE != 0 || N2 % TN_TILE != 0) return RG_ERR_ARG;
    if (lda < N1 || ldb < N2 || ldo < N2 || (fold && N1 != N2)) return RG_ERR_ARG;
    if (!out || !ws || (M > 0 && (!a || !b))) return RG_ERR_ARG;
    if (ws_bytes < regtr_gemm_tn_ws_bytes(M, N1, N2)) return RG_ERR_WORKSPACE;
    int chunk;
    const int splits = gemm_tn_splits(M, N1, N2, chunk);
    const hipStream_t s = (hipStream_t)stream;
    k_gemm_tn_part<<<dim3(N1 / TN_TILE, N2 / TN_TILE, splits), TN_THREADS, 0, s>>>(a, lda, b, ldb, M, N1, N2, chunk, (float*)ws);
    RG_RETURN_IF_LAUNCH_FAILED();
    k_gemm_tn_reduce<<<rg_cdiv((long long)N1 * N2, 256), 256, 0, s>>>((const float*)ws, splits, N1, N2, fold, out, ldo);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_corr_l1_bwd(const float* kp, const float* warped, const float* w, const int* seg_off, int n_clouds, int n, const float* pose,
                      int pose_stride, const float* grad, const float* den, float* d_warped, void* stream)
{
    if (n_clouds < 0 || n < 0 || (pose_stride != 12 && pose_stride != 16)) return RG_ERR_ARG;
    if (n > 0 && (!kp || !warped || !w || !seg_off || !pose || !grad || !den || !d_warped || n_clouds < 1)) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    k_corr_l1_bwd<<<rg_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(kp, warped, w, seg_off, n_clouds, n, pose, pose_stride, grad, den,
                                                                    d_warped);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_loss_terms(const float* logit, const float* gt_overlap, const float* kp, const float* warped, const int* seg_off,
                     int n_pairs, int n_total, const float* pose, int pose_stride, float* out, void* stream)
{
    if (n_pairs < 0 || n_total < 0) return RG_ERR_ARG;
    if (pose_stride != 12 && pose_stride != 16) return RG_ERR_ARG;
    if (n_total > 0 && (!logit || !gt_overlap || !kp || !warped)) return RG_ERR_ARG;
    if (n_pairs > 0 && (!seg_off || !pose || !out)) return RG_ERR_ARG;
    if (n_pairs == 0) return RG_OK;
    k_loss_terms<<<n_pairs, LT_THREADS, 0, (hipStream_t)stream>>>(logit, gt_overlap, kp, warped, seg_off, n_pairs, n_total, pose,
                                                                  pose_stride, out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_se3_transform(const float* xyz, const int* seg_off, int n_clouds, int n, const float* pose, int pose_stride, float* out,
                        void* stream)
{
    if (n_clouds < 0 || n < 0 || (pose_stride != 12 && pose_stride != 16)) return RG_ERR_ARG;
    if (n > 0 && (!xyz || !seg_off || !pose || !out || n_clouds < 1)) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    k_se3_transform<<<rg_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(xyz, seg_off, n_clouds, n, pose, pose_stride, out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
