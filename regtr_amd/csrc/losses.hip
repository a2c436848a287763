// Validation / test losses of RegTR.compute_loss (models/regtr.py:237-294) for gfx950, inference only.
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
};

// running state of one anchor row over a set of targets
struct RowState {
    float m, s;                    // max and sum of exp(l - m) over the targets with d >= r_n (or NaN distance)
    float dmin, lstar;             // current argmin distance and its logit
    int jmin;                      // its target index (-1: none seen)
};

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2)
{
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) { s = s + s2; m = M; return; }          // both empty (s = s2 = 0)
    s = s * expf(m - M) + s2 * expf(m2 - M);
    m = M;
}

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

__device__ __forceinline__ void transform_rn(const float* T, float x, float y, float z, float out[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
        out[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4 * r], x), __fmul_rn(T[4 * r + 1], y)), __fmul_rn(T[4 * r + 2], z)), T[4 * r + 3]);
}

__device__ __forceinline__ bool pair_ok(const int* off, int b, int n, int& lo, int& hi)
{
    lo = off[b];
    hi = off[b + 1];
    return 0 <= lo && lo <= hi && hi <= n;
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
                const float dx = __fsub_rn(ax[r][0], px), dy = __fsub_rn(ax[r][1], py), dz = __fsub_rn(ax[r][2], pz);
                const float d = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
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
            if (st[r].jmin >= 0) {
                float m = st[r].m, s = st[r].s;
                if (st[r].dmin < r_n) lse_merge(m, s, st[r].lstar, 1.f);
                loss = __fsub_rn(__fadd_rn(m, logf(s)), st[r].lstar);
                mask = st[r].dmin < r_p;
            }
            const bool valid = row < a1;
            rl_s[lr] = loss;
            rm_s[lr] = valid ? mask : 0;
            if (valid) {
                if (g.row_loss) g.row_loss[row] = loss;
                if (g.row_mask) g.row_mask[row] = (float)mask;
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

__device__ __forceinline__ double block_sum_d(double v, double* sh)
{
    v = rg_wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if (rg_lane() == 0) sh[wave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < LT_THREADS / RG_WAVE; w++) t += sh[w];
    return t;
}

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
    const double v0 = block_sum_d(bce, sh), v1 = block_sum_d(err[0], sh), v2 = block_sum_d(wsum[0], sh);
    const double v3 = block_sum_d(err[1], sh), v4 = block_sum_d(wsum[1], sh);
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

int infonce_tiles(int max_anc) { return max_anc > 0 ? rg_cdiv(max_anc, IN_TR) : 1; }

}  // namespace

extern "C" {

size_t regtr_infonce_ws_bytes(int n_pairs, int max_anc)
{
    if (n_pairs < 0 || max_anc < 0) return 0;
    return (size_t)n_pairs * infonce_tiles(max_anc) * 2 * sizeof(double);
}

int regtr_infonce(const float* anc, int ld_anc, const float* pos, int ld_pos, const float* anc_xyz, const float* pos_xyz,
                  const int* anc_seg_off, const int* pos_seg_off, int n_pairs, int n_anc, int n_pos, int max_anc, int D,
                  float r_p, float r_n, const float* anc_pose, float* pair_out, float* row_loss, float* row_mask, void* ws,
                  size_t ws_bytes, void* stream)
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
              r_p, r_n, anc_pose, row_loss, row_mask, (double*)ws};
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
