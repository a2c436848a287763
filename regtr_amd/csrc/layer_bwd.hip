// Backward pieces of the cross-encoder layer that are not contractions (gfx950; both HBM-bound streams, float4 accesses):
//   * regtr_layernorm_bwd   backward of regtr_layernorm (norm.hip, k_layernorm): dx (+ the residual branch's gradient), dgamma, dbeta
//   * regtr_bias_relu_bwd   column sums of a gradient, optionally through a ReLU mask: the bias gradients of the layer's Linears and
//                           the ReLU backward of the feed-forward block in the same pass
// (nn.LayerNorm / nn.Linear / F.relu backward under models/transformer/transformers.py:194-238 of the reference.)
// Deterministic: one owner per output element; the column sums are per-workgroup partials over FIXED row chunks (a function of the
// row count only), summed in a fixed order by a second launch.  No atomics.
#include "common.h"

namespace {

constexpr int LN_MAX_D = 1024;      // a lane keeps its dgamma / dbeta accumulators in registers: four float4 column groups per lane

// Rows per workgroup of both first passes: 32 until that would make more than ~1024 chunks, then n / 1024 rounded up to a multiple of
// four (a workgroup's four waves / row lanes share a chunk).  Host-side, a function of n only.
inline int bwd_chunk_rows(int n)
{
    const int r = 4 * rg_cdiv(n > 0 ? n : 1, 4096);
    return r > 32 ? r : 32;
}

// One wave per row, a workgroup's four waves interleaved over its chunk of rows.  Per row: mean and rstd recomputed with k_layernorm's
// own statements (so xh is the value the forward used), then with g = dy * gamma
//     dx = rstd * (g - mean(g) - xh * mean(g * xh)) [+ dres]
// and the lane's columns of dy * xh and dy added into its accumulators (row order).  The four waves' accumulators are added in wave
// order through LDS: partial[chunk][0][c] = sum dy * xh, partial[chunk][1][c] = sum dy over the chunk's rows.
template <int NG>
__global__ void __launch_bounds__(256) k_layernorm_bwd(const float* __restrict__ x, int n, int D, const float* __restrict__ gamma, float eps,
                                                       const float* __restrict__ dy, const float* __restrict__ dres, float* __restrict__ dx,
                                                       int rows, float* __restrict__ partial)
{
    __shared__ float4 sh[3 * 2 * NG * RG_WAVE];
    const int wave = threadIdx.x >> 6, lane = rg_lane();
    const int r0 = blockIdx.x * rows, r1 = min(n, r0 + rows);
    float4 ag[NG], ab[NG];
#pragma unroll
    for (int k = 0; k < NG; k++) ag[k] = ab[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int row = r0 + wave; row < r1; row += 4) {
        const float* xr = x + (size_t)row * D;
        const float* gr = dy + (size_t)row * D;
        float s = 0.f;
        for (int c = lane * 4; c < D; c += RG_WAVE * 4) {
            const float4 v = *(const float4*)(xr + c);
            s += (v.x + v.y) + (v.z + v.w);
        }
        const float mean = rg_wave_sum(s) / (float)D;
        float ss = 0.f;
        for (int c = lane * 4; c < D; c += RG_WAVE * 4) {
            const float4 v = *(const float4*)(xr + c);
            const float a = v.x - mean, b = v.y - mean, cc = v.z - mean, d = v.w - mean;
            ss += (a * a + b * b) + (cc * cc + d * d);
        }
        const float rstd = 1.0f / sqrtf(rg_wave_sum(ss) / (float)D + eps);
        float4 xh[NG], g[NG];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NG; k++) {
            const int c = lane * 4 + k * RG_WAVE * 4;
            xh[k] = g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < D) {
                const float4 v = *(const float4*)(xr + c), u = *(const float4*)(gr + c), gm = *(const float4*)(gamma + c);
                xh[k] = make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd);
                g[k] = make_float4(u.x * gm.x, u.y * gm.y, u.z * gm.z, u.w * gm.w);
                s1 += (g[k].x + g[k].y) + (g[k].z + g[k].w);
                s2 += (g[k].x * xh[k].x + g[k].y * xh[k].y) + (g[k].z * xh[k].z + g[k].w * xh[k].w);
                ag[k].x += u.x * xh[k].x; ag[k].y += u.y * xh[k].y; ag[k].z += u.z * xh[k].z; ag[k].w += u.w * xh[k].w;
                ab[k].x += u.x; ab[k].y += u.y; ab[k].z += u.z; ab[k].w += u.w;
            }
        }
        const float c1 = rg_wave_sum(s1) / (float)D, c2 = rg_wave_sum(s2) / (float)D;
#pragma unroll
        for (int k = 0; k < NG; k++) {
            const int c = lane * 4 + k * RG_WAVE * 4;
            if (c < D) {
                float4 o = make_float4(rstd * (g[k].x - c1 - xh[k].x * c2), rstd * (g[k].y - c1 - xh[k].y * c2),
                                       rstd * (g[k].z - c1 - xh[k].z * c2), rstd * (g[k].w - c1 - xh[k].w * c2));
                if (dres) {
                    const float4 r = *(const float4*)(dres + (size_t)row * D + c);
                    o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
                }
                *(float4*)(dx + (size_t)row * D + c) = o;
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < NG; k++) {
            sh[((wave - 1) * 2 * NG + 2 * k) * RG_WAVE + lane] = ag[k];
            sh[((wave - 1) * 2 * NG + 2 * k + 1) * RG_WAVE + lane] = ab[k];
        }
    }
    __syncthreads();
    if (wave == 0) {
        float* pg = partial + (size_t)blockIdx.x * 2 * D;
#pragma unroll
        for (int k = 0; k < NG; k++) {
            const int c = lane * 4 + k * RG_WAVE * 4;
            for (int w = 0; w < 3; w++) {
                const float4 a = sh[(w * 2 * NG + 2 * k) * RG_WAVE + lane], b = sh[(w * 2 * NG + 2 * k + 1) * RG_WAVE + lane];
                ag[k].x += a.x; ag[k].y += a.y; ag[k].z += a.z; ag[k].w += a.w;
                ab[k].x += b.x; ab[k].y += b.y; ab[k].z += b.z; ab[k].w += b.w;
            }
            if (c < D) {
                *(float4*)(pg + c) = ag[k];
                *(float4*)(pg + D + c) = ab[k];
            }
        }
    }
}

// Thread (tx = t % CW, ty = t / CW) owns float4 column group blockIdx.x * CW + tx for rows ty, ty + TR, ... of chunk blockIdx.y
// (TR = 256 / CW), added in row order; the TR row lanes are added in lane order through LDS: partial[chunk][c].  With h:
// dh = h > 0 ? g : 0 is what is summed, and stored when dh is given (dh may be g itself: every element is read, then written, by its
// one owner -- hence no __restrict__ on the two).
template <int CW>
__global__ void __launch_bounds__(256) k_bias_relu_bwd(const float* g, int ldg, const float* __restrict__ h, int ldh, float* dh, int ld_dh,
                                                       int n, int N, int rows, float* __restrict__ partial)
{
    constexpr int TR = 256 / CW;
    __shared__ float4 sh[256];
    const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
    const int c = 4 * (blockIdx.x * CW + tx);
    const int r0 = blockIdx.y * rows, r1 = min(n, r0 + rows);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < N) {
        auto one = [&](int r, float4 v, const float4& m) {
            if (h) {
                v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f; v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
                if (dh) *(float4*)(dh + (size_t)r * ld_dh + c) = v;
            }
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        };
        // full groups of four rows with the loads unconditional and in flight together, then the tail row by row: the same rows in
        // the same order as one loop (norm.hip, k_instnorm_partial)
        int r = r0 + ty;
        for (; r + 3 * TR < r1; r += 4 * TR) {
            float4 v[4], m[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = *(const float4*)(g + (size_t)(r + u * TR) * ldg + c);
            if (h) {
#pragma unroll
                for (int u = 0; u < 4; u++) m[u] = *(const float4*)(h + (size_t)(r + u * TR) * ldh + c);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) one(r + u * TR, v[u], m[u]);
        }
        for (; r < r1; r += TR) {
            const float4 v = *(const float4*)(g + (size_t)r * ldg + c);
            float4 m = v;
            if (h) m = *(const float4*)(h + (size_t)r * ldh + c);
            one(r, v, m);
        }
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (ty == 0 && c < N) {
        for (int y = 1; y < TR; y++) {
            const float4 a = sh[y * CW + tx];
            acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
        }
        *(float4*)(partial + (size_t)blockIdx.y * N + c) = acc;
    }
}

// out[c] = sum over the chunks of partial[chunk][c], c < ncols: one wave per column, the chunks dealt to the lanes in order and added
// in float64 by a fixed shuffle tree.  Columns [0, split) go to out_a, the rest to out_b (dgamma | dbeta).
__global__ void __launch_bounds__(256) k_colsum_final(const float* __restrict__ partial, int nchunk, int ncols, float* __restrict__ out_a,
                                                      int split, float* __restrict__ out_b)
{
    const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= ncols) return;
    const int lane = rg_lane();
    double s = 0;
    for (int k = lane; k < nchunk; k += RG_WAVE) s += (double)partial[(size_t)k * ncols + c];
    s = rg_wave_sum(s);
    if (lane == 0) {
        if (c < split) out_a[c] = (float)s; else out_b[c - split] = (float)s;
    }
}

inline bool misaligned(const void* p) { return ((uintptr_t)p % 16) != 0; }

}  // namespace

extern "C" {

size_t regtr_layernorm_bwd_ws_bytes(int n, int D)
{
    if (n <= 0 || D < 4 || D % 4 || D > LN_MAX_D) return 0;
    return (size_t)rg_cdiv(n, bwd_chunk_rows(n)) * 2 * D * sizeof(float);
}

int regtr_layernorm_bwd(const float* x, int n, int D, const float* gamma, float eps, const float* dy, const float* dres, float* dx,
                        float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream)
{
    if (n < 0 || D < 4 || D % 4 || D > LN_MAX_D) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    if (!x || !gamma || !dy || !dx || !dgamma || !dbeta || !ws) return RG_ERR_ARG;
    if (misaligned(x) || misaligned(gamma) || misaligned(dy) || misaligned(dres) || misaligned(dx) || misaligned(ws)) return RG_ERR_ARG;
    if (ws_bytes < regtr_layernorm_bwd_ws_bytes(n, D)) return RG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int rows = bwd_chunk_rows(n), nchunk = rg_cdiv(n, rows);
    float* partial = (float*)ws;
    if (D <= 256) k_layernorm_bwd<1><<<nchunk, 256, 0, st>>>(x, n, D, gamma, eps, dy, dres, dx, rows, partial);
    else if (D <= 512) k_layernorm_bwd<2><<<nchunk, 256, 0, st>>>(x, n, D, gamma, eps, dy, dres, dx, rows, partial);
    else k_layernorm_bwd<4><<<nchunk, 256, 0, st>>>(x, n, D, gamma, eps, dy, dres, dx, rows, partial);
    k_colsum_final<<<rg_cdiv(2 * D, 4), 256, 0, st>>>(partial, nchunk, 2 * D, dgamma, D, dbeta);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

size_t regtr_bias_relu_bwd_ws_bytes(int n, int N)
{
    if (n <= 0 || N < 4 || N % 4) return 0;
    return (size_t)rg_cdiv(n, bwd_chunk_rows(n)) * N * sizeof(float);
}

int regtr_bias_relu_bwd(const float* g, int ldg, const float* h, int ldh, float* dh, int ld_dh, float* db, int n, int N, void* ws,
                        size_t ws_bytes, void* stream)
{
    if (n < 0 || N < 4 || N % 4 || ldg < N || ldg % 4) return RG_ERR_ARG;
    if (h && (ldh < N || ldh % 4)) return RG_ERR_ARG;
    if (dh && (!h || ld_dh < N || ld_dh % 4)) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    if (!g || !db || !ws || misaligned(g) || misaligned(h) || misaligned(dh) || misaligned(ws)) return RG_ERR_ARG;
    if (ws_bytes < regtr_bias_relu_bwd_ws_bytes(n, N)) return RG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int rows = bwd_chunk_rows(n), nchunk = rg_cdiv(n, rows), N4 = N / 4;
    float* partial = (float*)ws;
    if (N4 >= 64) k_bias_relu_bwd<64><<<dim3(rg_cdiv(N4, 64), nchunk), 256, 0, st>>>(g, ldg, h, ldh, dh, ld_dh, n, N, rows, partial);
    else if (N4 >= 32) k_bias_relu_bwd<32><<<dim3(rg_cdiv(N4, 32), nchunk), 256, 0, st>>>(g, ldg, h, ldh, dh, ld_dh, n, N, rows, partial);
    else k_bias_relu_bwd<16><<<dim3(rg_cdiv(N4, 16), nchunk), 256, 0, st>>>(g, ldg, h, ldh, dh, ld_dh, n, N, rows, partial);
    k_colsum_final<<<rg_cdiv(N, 4), 256, 0, st>>>(partial, nchunk, N, db, N, nullptr);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
