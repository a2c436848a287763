// Backward pieces of the correspondence head and of the overlap loss (gfx950; HBM-bound streams, float4 accesses):
//   * regtr_head_tail_bwd    CorrespondenceRegressor's two narrow outputs, corr = h2 W4^T + b4 (3 wide) and logit = f wc^T + bc (1 wide),
//                            backward in ONE pass over the rows: the gradient in front of coor_mlp[2]'s ReLU, the logit branch's share of
//                            df, and all six parameter / bias sums
//   * regtr_bce_logits_bwd   nn.BCEWithLogitsLoss (mean) backward, elementwise
// (models/regtr.py:399-443 and :250-257 of the reference.)
// Deterministic like layer_bwd.hip: one owner per output element; the sums are per-workgroup partials over FIXED row chunks (a function
// of the row count only), each thread adding its rows in row order, added in a fixed order in float64 by a second launch.  No atomics.
#include "common.h"

namespace {

// Rows per workgroup of the first pass: layer_bwd.hip's rule (32 until that would make more than ~1024 chunks).  Host-side, of m only.
inline int tail_chunk_rows(int m)
{
    const int r = 4 * rg_cdiv(m > 0 ? m : 1, 4096);
    return r > 32 ? r : 32;
}

// Columns of one chunk's partial row: dW4 (3 D) | dwc (D) | db2 (D) | db4 (3) | dbc (1)
inline int tail_partial_cols(int D) { return 5 * D + 4; }

__device__ __forceinline__ void add4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ __forceinline__ void fma4(float4& a, float s, const float4& b) { a.x += s * b.x; a.y += s * b.y; a.z += s * b.z; a.w += s * b.w; }

// k_bias_relu_bwd's mapping: thread (tx = t % CW, ty = t / CW) owns float4 column group blockIdx.x * CW + tx for rows ty, ty + TR, ...
// of chunk blockIdx.y (TR = 256 / CW), in row order.  Per row and column c, with dc = dcorr[row] (0 without dcorr) and dl = dlogit[row]
// (0 without dlogit):
//     g2 = h2 > 0 ? (dc0 W4[0][c] + dc1 W4[1][c]) + dc2 W4[2][c] : +0        r = dl wc[c]
//     dW4[k][c] += dc_k h2        dwc[c] += dl f        db2[c] += g2
// and the column-free sums db4 += dc, dbc += dl by the threads of column group 0.  The TR row lanes are added in lane order through LDS.
template <int CW>
__global__ void __launch_bounds__(256) k_head_tail_bwd(const float* __restrict__ dcorr, const float* __restrict__ dlogit,
                                                       const float* __restrict__ h2, const float* __restrict__ f,
                                                       const float* __restrict__ W4, const float* __restrict__ wc, int m, int D, int rows,
                                                       float* __restrict__ g2, float* __restrict__ r, float* __restrict__ partial)
{
    constexpr int TR = 256 / CW;
    __shared__ float4 sh[256];
    const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
    const int c = 4 * (blockIdx.x * CW + tx);
    const int r0 = blockIdx.y * rows, r1 = min(m, r0 + rows);
    const bool live = c < D;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 w0 = zero, w1 = zero, w2 = zero, wl = zero;
    if (live) {
        w0 = *(const float4*)(W4 + c); w1 = *(const float4*)(W4 + D + c); w2 = *(const float4*)(W4 + 2 * (size_t)D + c);
        wl = *(const float4*)(wc + c);
    }
    float4 aw0 = zero, aw1 = zero, aw2 = zero, awc = zero, ab2 = zero, ad = zero;     // ad: (db4[0], db4[1], db4[2], dbc)
    if (live) {
        for (int row = r0 + ty; row < r1; row += TR) {
            const size_t at = (size_t)row * D + c;
            float4 d = zero;
            if (dcorr) { d.x = dcorr[3 * (size_t)row]; d.y = dcorr[3 * (size_t)row + 1]; d.z = dcorr[3 * (size_t)row + 2]; }
            if (dlogit) d.w = dlogit[row];
            float4 g = zero;
            if (dcorr) {
                const float4 h = *(const float4*)(h2 + at);
                g.x = h.x > 0.f ? (d.x * w0.x + d.y * w1.x) + d.z * w2.x : 0.f;
                g.y = h.y > 0.f ? (d.x * w0.y + d.y * w1.y) + d.z * w2.y : 0.f;
                g.z = h.z > 0.f ? (d.x * w0.z + d.y * w1.z) + d.z * w2.z : 0.f;
                g.w = h.w > 0.f ? (d.x * w0.w + d.y * w1.w) + d.z * w2.w : 0.f;
                fma4(aw0, d.x, h); fma4(aw1, d.y, h); fma4(aw2, d.z, h);
                add4(ab2, g);
            }
            *(float4*)(g2 + at) = g;
            float4 o = zero;
            if (dlogit) {
                const float4 v = *(const float4*)(f + at);
                o = make_float4(d.w * wl.x, d.w * wl.y, d.w * wl.z, d.w * wl.w);
                fma4(awc, d.w, v);
            }
            *(float4*)(r + at) = o;
            add4(ad, d);
        }
    }
    // the TR row lanes of a column group, added in lane order; one accumulator after the other through the same 4 KB of LDS
    float* pg = partial + (size_t)blockIdx.y * (5 * (size_t)D + 4);
    auto reduce = [&](float4 acc, float* dst, bool write) {
        __syncthreads();
        sh[threadIdx.x] = acc;
        __syncthreads();
        if (ty == 0 && write) {
            for (int y = 1; y < TR; y++) add4(acc, sh[y * CW + tx]);
            *(float4*)dst = acc;
        }
    };
    reduce(aw0, pg + c, live);
    reduce(aw1, pg + D + c, live);
    reduce(aw2, pg + 2 * (size_t)D + c, live);
    reduce(awc, pg + 3 * (size_t)D + c, live);
    reduce(ab2, pg + 4 * (size_t)D + c, live);
    reduce(ad, pg + 5 * (size_t)D, blockIdx.x == 0 && tx == 0);
}

struct TailSums { float *dW4, *dwc, *db2, *db4, *dbc; };

// Column col < 5 D + 4 of the partials: one wave per column, the chunks dealt to the lanes in order and added in float64 by a fixed
// shuffle tree (layer_bwd.hip, k_colsum_final), then rounded once into the output that column belongs to.
__global__ void __launch_bounds__(256) k_head_tail_final(const float* __restrict__ partial, int nchunk, int D, TailSums out)
{
    const int ncols = 5 * D + 4;
    const int col = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (col >= ncols) return;
    const int lane = rg_lane();
    double s = 0;
    for (int k = lane; k < nchunk; k += RG_WAVE) s += (double)partial[(size_t)k * ncols + col];
    s = rg_wave_sum(s);
    if (lane == 0) {
        const float v = (float)s;
        if (col < 3 * D) out.dW4[col] = v;
        else if (col < 4 * D) out.dwc[col - 3 * D] = v;
        else if (col < 5 * D) { if (out.db2) out.db2[col - 4 * D] = v; }
        else if (col < 5 * D + 3) out.db4[col - 5 * D] = v;
        else out.dbc[0] = v;
    }
}

// dlogit[i] = (g / n) (sigmoid(x_i) - y_i), the sigmoid from e = exp(-|x|) <= 1: 1 / (1 + e) for x >= 0, e / (1 + e) below (no overflow,
// and no cancellation against 1 for large |x|).
__global__ void __launch_bounds__(256) k_bce_logits_bwd(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ grad, int n, float* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float scale = grad[0] / (float)n;
    const float v = x[i], e = expf(-fabsf(v));
    const float s = (v >= 0.f ? 1.0f : e) / (1.0f + e);
    out[i] = scale * (s - y[i]);
}

inline bool misaligned(const void* p) { return ((uintptr_t)p % 16) != 0; }

}  // namespace

extern "C" {

size_t regtr_head_tail_bwd_ws_bytes(int m, int D)
{
    if (m <= 0 || D < 64 || D % 64) return 0;
    return (size_t)rg_cdiv(m, tail_chunk_rows(m)) * tail_partial_cols(D) * sizeof(float);
}

int regtr_head_tail_bwd(const float* dcorr, const float* dlogit, const float* h2, const float* f, const float* W4, const float* wc, int m,
                        int D, float* g2, float* r, float* dW4, float* db4, float* dwc, float* dbc, float* db2, void* ws, size_t ws_bytes,
                        void* stream)
{
    if (m < 0 || D < 64 || D % 64) return RG_ERR_ARG;
    if (m == 0) return RG_OK;
    if (!h2 || !f || !W4 || !wc || !g2 || !r || !dW4 || !db4 || !dwc || !dbc || !ws) return RG_ERR_ARG;
    if (misaligned(h2) || misaligned(f) || misaligned(W4) || misaligned(wc) || misaligned(g2) || misaligned(r) || misaligned(ws))
        return RG_ERR_ARG;
    if (g2 == r || g2 == h2 || g2 == f || r == h2 || r == f) return RG_ERR_ARG;
    if (ws_bytes < regtr_head_tail_bwd_ws_bytes(m, D)) return RG_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int rows = tail_chunk_rows(m), nchunk = rg_cdiv(m, rows), D4 = D / 4;
    float* partial = (float*)ws;
    if (D4 >= 64) k_head_tail_bwd<64><<<dim3(rg_cdiv(D4, 64), nchunk), 256, 0, st>>>(dcorr, dlogit, h2, f, W4, wc, m, D, rows, g2, r, partial);
    else k_head_tail_bwd<16><<<dim3(D4 / 16, nchunk), 256, 0, st>>>(dcorr, dlogit, h2, f, W4, wc, m, D, rows, g2, r, partial);
    const TailSums out = {dW4, dwc, db2, db4, dbc};
    k_head_tail_final<<<rg_cdiv(tail_partial_cols(D), 4), 256, 0, st>>>(partial, nchunk, D, out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_bce_logits_bwd(const float* logit, const float* target, const float* grad, int n, float* dlogit, void* stream)
{
    if (n < 0) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    if (!logit || !target || !grad || !dlogit) return RG_ERR_ARG;
    k_bce_logits_bwd<<<rg_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(logit, target, grad, n, dlogit);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
