// Backward of the backbone's two remaining operators for gfx950 (regtr_amd/backbone_grad.py):
//   * per-cloud InstanceNorm (+ LeakyReLU, + shortcut): regtr_instnorm_stats + regtr_instnorm_apply (norm.hip) taken together,
//         y = act( (x - mean) rstd [+ res | + (res - rmean) rrstd] ),   biased variance, no affine
//     (BatchNormBlock with nn.InstanceNorm1d, kpconv_blocks.py:489,510-519 of the reference; the blocks' LeakyReLU(0.1), :556-561,741).
//     With z the activation's argument, g = dy (z > 0 ? 1 : slope) and xh = (x - mean) rstd, per (cloud, channel) over the cloud's rows:
//         dx = rstd (g - mean(g) - xh mean(g xh)),   dres = g  |  rrstd (g - mean(g) - rh mean(g rh)).
//     Pass 1 (norm.hip's thread mapping and chunking) writes per-(cloud, chunk, channel) sums of g, g xh and g rh in float64, a second
//     launch adds a cloud's chunks in a fixed order, pass 2 applies.  z is recomputed with k_instnorm_apply's own arithmetic (below), so
//     the LeakyReLU side of every element is the forward's.
//   * max-pool over a neighbour table (max_pool, kpconv_blocks.py:127-143): regtr_maxpool_argmax stores, per (query, channel), the
//     winning COLUMN of the table (query owner, one more pass over the forward's rows); regtr_maxpool_gather_bwd then walks the table by
//     support (regtr_nbr_transpose, kpconv_bwd.hip) and adds the dy of the entries that won, one lane per float4 of a dx row,
//     sequentially in ascending entry order.  The support owner cannot decide "did I win?" on its own: that takes the maximum over all H
//     rows of the query, i.e. the forward's whole gather once per ENTRY instead of once per query.
// No floating-point atomics, one owner per output element, bit-reproducible, nothing synchronises with the host.
#include "common.h"

namespace {

inline bool misaligned(const void* p) { return ((uintptr_t)p % 16) != 0; }

// ------------------------------------------------------------------------------------------------ InstanceNorm backward
// (mean, rstd) of channels 4 tx .. 4 tx + 3 of cloud b; NULL: (0, 1), as k_instnorm_apply reads them
__device__ __forceinline__ void load_stats(const float2* __restrict__ stats, int b, int C, int tx, float* mu, float* rs)
{
#pragma unroll
    for (int j = 0; j < 4; j++) { mu[j] = 0.f; rs[j] = 1.f; }
    if (stats) {
        const float4* st = (const float4*)(stats + (size_t)b * C + 4 * tx);
        const float4 a = st[0], c = st[1];
        mu[0] = a.x; rs[0] = a.y; mu[1] = a.z; rs[1] = a.w; mu[2] = c.x; rs[2] = c.y; mu[3] = c.z; rs[3] = c.w;
    }
}

// One element of k_instnorm_apply, operation for operation: xh = (x - mu) * rs rounded, then -- with a shortcut -- ONE fused
// multiply-add z = fma(q - rmu, rrs, xh), which is what `o += (q - rmu) * rrs` is compiled to there (a plain shortcut runs the same
// statement with rmu = 0, rrs = 1).  Contraction is switched off around it so that nothing else fuses.  -> g = dy (z > 0 ? 1 : slope).
__device__ __forceinline__ float in_grad(float x, float mu, float rs, bool has_res, float q, float rmu, float rrs, int act, float slope,
                                         float dy, float& xh, float& rh)
{
#pragma clang fp contract(off)
    xh = (x - mu) * rs;
    rh = 0.f;
    float z = xh;
    if (has_res) {
        const float d = q - rmu;
        rh = d * rrs;
        z = __builtin_fmaf(d, rrs, xh);
    }
    return (act == 1 && !(z > 0.f)) ? dy * slope : dy;
}

// partial[((cloud * nchunk + chunk) * C + c) * 3 + {0, 1, 2}] = sums of g, g xh, g rh over the chunk's rows, accumulated in float64
__global__ void __launch_bounds__(256) k_instnorm_bwd_partial(const float* __restrict__ x, const int* __restrict__ seg_off, int C,
                                                              const float2* __restrict__ stats, const float* __restrict__ res,
                                                              const float2* __restrict__ res_stats, int act, float slope,
                                                              const float* __restrict__ dy, int nchunk, int rows,
                                                              double* __restrict__ partial)
{
    __shared__ double sh[256 * 12];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int r0 = seg_off[b] + chunk * rows, r1 = min(seg_off[b + 1], r0 + rows);
    if (r0 >= r1) return;
    const int C4 = C >> 2, TR = 256 / C4;
    const int tx = threadIdx.x % C4, ty = threadIdx.x / C4;
    float mu[4], rs[4], rmu[4], rrs[4];
    load_stats(stats, b, C, tx, mu, rs);
    load_stats(res_stats, b, C, tx, rmu, rrs);
    double s[12];
#pragma unroll
    for (int j = 0; j < 12; j++) s[j] = 0.0;
    for (int r = r0 + ty; r < r1; r += 4 * TR) {
        // unconditional loads from CLAMPED rows, all in flight before the first use (norm.hip, k_instnorm_apply)
        float4 v[4], gv[4], rv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = *(const float4*)(x + (size_t)min(r + u * TR, r1 - 1) * C + 4 * tx);
#pragma unroll
        for (int u = 0; u < 4; u++) gv[u] = *(const float4*)(dy + (size_t)min(r + u * TR, r1 - 1) * C + 4 * tx);
        if (res) {
#pragma unroll
            for (int u = 0; u < 4; u++) rv[u] = *(const float4*)(res + (size_t)min(r + u * TR, r1 - 1) * C + 4 * tx);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (r + u * TR >= r1) continue;
            const float xv[4] = {v[u].x, v[u].y, v[u].z, v[u].w}, dv[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
            float qv[4] = {0.f, 0.f, 0.f, 0.f};
            if (res) { qv[0] = rv[u].x; qv[1] = rv[u].y; qv[2] = rv[u].z; qv[3] = rv[u].w; }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float xh, rh;
                const float g = in_grad(xv[j], mu[j], rs[j], res != nullptr, qv[j], rmu[j], rrs[j], act, slope, dv[j], xh, rh);
                s[j] += g; s[4 + j] += (double)g * xh; s[8 + j] += (double)g * rh;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 12; j++) sh[threadIdx.x * 12 + j] = s[j];
    __syncthreads();
    if (ty == 0) {
        for (int y = 1; y < TR; y++)
#pragma unroll
            for (int j = 0; j < 12; j++) s[j] += sh[(y * C4 + tx) * 12 + j];
        double* o = partial + (((size_t)b * nchunk + chunk) * C + 4 * tx) * 3;
#pragma unroll
        for (int j = 0; j < 4; j++) { o[3 * j] = s[j]; o[3 * j + 1] = s[4 + j]; o[3 * j + 2] = s[8 + j]; }
    }
}

// means[cloud * C + c] = (mean g, mean g xh, mean g rh, 0) in float32; one wave per (cloud, channel) adds the chunks in a fixed tree
__global__ void __launch_bounds__(256) k_instnorm_bwd_finalize(const double* __restrict__ partial, const int* __restrict__ seg_off, int C,
                                                               int nchunk, int rows, float4* __restrict__ means)
{
    const int b = blockIdx.y, c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (c >= C) return;
    const int lane = rg_lane();
    const int n = seg_off[b + 1] - seg_off[b];
    const int used = n > 0 ? min(nchunk, (n + rows - 1) / rows) : 0;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int k = lane; k < used; k += RG_WAVE) {
        const double* p = partial + (((size_t)b * nchunk + k) * C + c) * 3;
        s0 += p[0]; s1 += p[1]; s2 += p[2];
    }
    s0 = rg_wave_sum(s0); s1 = rg_wave_sum(s1); s2 = rg_wave_sum(s2);
    if (lane == 0) means[(size_t)b * C + c] = n > 0 ? make_float4((float)(s0 / n), (float)(s1 / n), (float)(s2 / n), 0.f)
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
}

// dx = rs ((g - m_g) - xh m_gx);  dres = g (plain shortcut) or rrs ((g - m_g) - rh m_gr) (normalised shortcut).  means may be NULL when
// only a plain shortcut's dres is wanted.
__global__ void __launch_bounds__(256) k_instnorm_bwd_apply(const float* __restrict__ x, const int* __restrict__ seg_off, int C,
                                                            const float2* __restrict__ stats, const float* __restrict__ res,
                                                            const float2* __restrict__ res_stats, int act, float slope,
                                                            const float* __restrict__ dy, const float4* __restrict__ means,
                                                            float* __restrict__ dx, float* __restrict__ dres, int rows)
{
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int r0 = seg_off[b] + chunk * rows, r1 = min(seg_off[b + 1], r0 + rows);
    if (r0 >= r1) return;
    const int C4 = C >> 2, TR = 256 / C4;
    const int tx = threadIdx.x % C4, ty = threadIdx.x / C4;
    float mu[4], rs[4], rmu[4], rrs[4];
    load_stats(stats, b, C, tx, mu, rs);
    load_stats(res_stats, b, C, tx, rmu, rrs);
    float mg[4] = {0.f, 0.f, 0.f, 0.f}, mgx[4] = {0.f, 0.f, 0.f, 0.f}, mgr[4] = {0.f, 0.f, 0.f, 0.f};
    if (means) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float4 m = means[(size_t)b * C + 4 * tx + j];
            mg[j] = m.x; mgx[j] = m.y; mgr[j] = m.z;
        }
    }
    for (int r = r0 + ty; r < r1; r += 4 * TR) {
        float4 v[4], gv[4], rv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = *(const float4*)(x + (size_t)min(r + u * TR, r1 - 1) * C + 4 * tx);
#pragma unroll
        for (int u = 0; u < 4; u++) gv[u] = *(const float4*)(dy + (size_t)min(r + u * TR, r1 - 1) * C + 4 * tx);
        if (res) {
#pragma unroll
            for (int u = 0; u < 4; u++) rv[u] = *(const float4*)(res + (size_t)min(r + u * TR, r1 - 1) * C + 4 * tx);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int rr = r + u * TR;
            if (rr >= r1) continue;
            const float xv[4] = {v[u].x, v[u].y, v[u].z, v[u].w}, dv[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
            float qv[4] = {0.f, 0.f, 0.f, 0.f};
            if (res) { qv[0] = rv[u].x; qv[1] = rv[u].y; qv[2] = rv[u].z; qv[3] = rv[u].w; }
            float ox[4], orr[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float xh, rh;
                const float g = in_grad(xv[j], mu[j], rs[j], res != nullptr, qv[j], rmu[j], rrs[j], act, slope, dv[j], xh, rh);
                {
#pragma clang fp contract(off)
                    const float gc = g - mg[j];
                    ox[j] = rs[j] * (gc - xh * mgx[j]);
                    orr[j] = res_stats ? rrs[j] * (gc - rh * mgr[j]) : g;
                }
            }
            if (dx) *(float4*)(dx + (size_t)rr * C + 4 * tx) = make_float4(ox[0], ox[1], ox[2], ox[3]);
            if (dres) *(float4*)(dres + (size_t)rr * C + 4 * tx) = make_float4(orr[0], orr[1], orr[2], orr[3]);
        }
    }
}

bool instnorm_bwd_shape_ok(int n_clouds, int max_len, int C)
{
    return n_clouds >= 1 && max_len >= 0 && C >= 4 && C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0;
}

// ------------------------------------------------------------------------------------------------ max-pool backward
// arg[q, c] = the first column h (of the H used) whose row holds the maximum of channel c, -1 when that row is the zero shadow row.
// 1 << lq_log2 lanes serve a query (one float4 of channels each, striding over wider rows), as in k_maxpool_gather.  Columns are read
// eight at a time with clamped column numbers -- a repeated column never wins again under `>` -- and the rows with unconditional loads
// from clamped indices, replaced by zeros afterwards where the index was a shadow.
__global__ void __launch_bounds__(256) k_maxpool_argmax(const float* __restrict__ x, int ns, int C, const int* __restrict__ nbr, int ld_nbr,
                                                        int nq, int H, int lq_log2, short* __restrict__ arg)
{
    const int lane = rg_lane(), LQ = 1 << lq_log2;
    const int q = ((rg_xcd_block(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) << (6 - lq_log2)) + (lane >> lq_log2);
    const int qc = q < nq ? q : nq - 1;              // a dead lane repeats the last query (it never stores)
    const int* row = nbr + (size_t)qc * ld_nbr;
    for (int c = (lane & (LQ - 1)) * 4; c < C; c += LQ * 4) {
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int a[4] = {-1, -1, -1, -1};
        for (int h0 = 0; h0 < H; h0 += 8) {
            int idx[8];
#pragma unroll
            for (int u = 0; u < 8; u++) idx[u] = row[min(h0 + u, H - 1)];
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = *(const float4*)(x + (size_t)min(max(idx[u], 0), ns - 1) * C + c);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const bool real = (unsigned)idx[u] < (unsigned)ns;
                const float w[4] = {real ? v[u].x : 0.f, real ? v[u].y : 0.f, real ? v[u].z : 0.f, real ? v[u].w : 0.f};
                const int col = real ? min(h0 + u, H - 1) : -1;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (w[j] > m[j]) { m[j] = w[j]; a[j] = col; }
            }
        }
        if (q < nq) *(short4*)(arg + (size_t)q * C + c) = make_short4((short)a[0], (short)a[1], (short)a[2], (short)a[3]);
    }
}

// k_maxpool_argmax and the forward's maximum in ONE pass over the rows: out[q, c] by regtr_maxpool_gather's own fmaxf chain over the same
// values in the same column order (a repeated last column changes no maximum; a shadow reads as the zero row), arg[q, c] as above.
__global__ void __launch_bounds__(256) k_maxpool_fwd_argmax(const float* __restrict__ x, int ns, int C, const int* __restrict__ nbr,
                                                            int ld_nbr, int nq, int H, int lq_log2, float* __restrict__ out,
                                                            short* __restrict__ arg)
{
    const int lane = rg_lane(), LQ = 1 << lq_log2;
    const int q = ((rg_xcd_block(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) << (6 - lq_log2)) + (lane >> lq_log2);
    const int qc = q < nq ? q : nq - 1;              // a dead lane repeats the last query (it never stores)
    const int* row = nbr + (size_t)qc * ld_nbr;
    for (int c = (lane & (LQ - 1)) * 4; c < C; c += LQ * 4) {
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};      // the winner under `>` (first column on ties)
        float o[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};      // the forward's fmaxf chain
        int a[4] = {-1, -1, -1, -1};
        for (int h0 = 0; h0 < H; h0 += 8) {
            int idx[8];
#pragma unroll
            for (int u = 0; u < 8; u++) idx[u] = row[min(h0 + u, H - 1)];
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = *(const float4*)(x + (size_t)min(max(idx[u], 0), ns - 1) * C + c);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const bool real = (unsigned)idx[u] < (unsigned)ns;
                const float w[4] = {real ? v[u].x : 0.f, real ? v[u].y : 0.f, real ? v[u].z : 0.f, real ? v[u].w : 0.f};
                const int col = real ? min(h0 + u, H - 1) : -1;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    o[j] = fmaxf(o[j], w[j]);
                    if (w[j] > m[j]) { m[j] = w[j]; a[j] = col; }
                }
            }
        }
        if (q < nq) {
            *(float4*)(out + (size_t)q * C + c) = make_float4(o[0], o[1], o[2], o[3]);
            *(short4*)(arg + (size_t)q * C + c) = make_short4((short)a[0], (short)a[1], (short)a[2], (short)a[3]);
        }
    }
}

__global__ void __launch_bounds__(256) k_fill_i16(short* __restrict__ p, size_t n, short v)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// dx[s, c] = sum over support s's entries e = q H + h, ascending, of (arg[q, c] == h ? dy[q, c] : +0).  1 << ls_log2 lanes own a row of
// dx, one float4 of channels each (striding over wider rows).  Four entries' loads are in flight at a time; the adds stay in entry
// order.  The list's tail repeats its last entry with a column that matches nothing: adding +0 to a sum that started at +0 changes no bit.
__global__ void __launch_bounds__(256) k_maxpool_gather_bwd(const float* __restrict__ dy, const short* __restrict__ arg, int nq, int H, int C,
                                                            const int* __restrict__ row_off, const int* __restrict__ ent, int ns, int n_ent,
                                                            int ls_log2, float* __restrict__ dx)
{
    const int lane = rg_lane(), LS = 1 << ls_log2;
    const int s = ((rg_xcd_block(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) << (6 - ls_log2)) + (lane >> ls_log2);
    if (s >= ns) return;
    int e0 = row_off[s], e1 = row_off[s + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > n_ent ? n_ent : e1;                    // (a table that is not this nbr's cannot make the walk leave the entry list)
    for (int c = (lane & (LS - 1)) * 4; c < C; c += LS * 4) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = e0; i0 < e1; i0 += 4) {
            int q[4], h[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                int e = ent[min(i0 + u, e1 - 1)];
                e = e < 0 ? 0 : (e >= n_ent ? n_ent - 1 : e);
                q[u] = e / H;
                h[u] = i0 + u < e1 ? e - q[u] * H : -2;
            }
            float4 g[4];
            short4 a[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                a[u] = *(const short4*)(arg + (size_t)q[u] * C + c);
                g[u] = *(const float4*)(dy + (size_t)q[u] * C + c);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                acc[0] += a[u].x == h[u] ? g[u].x : 0.f;
                acc[1] += a[u].y == h[u] ? g[u].y : 0.f;
                acc[2] += a[u].z == h[u] ? g[u].z : 0.f;
                acc[3] += a[u].w == h[u] ? g[u].w : 0.f;
            }
        }
        *(float4*)(dx + (size_t)s * C + c) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// lanes per row of C channels: C / 4 rounded up to a power of two, at most a wave
int lanes_log2(int C)
{
    int l = 0;
    while ((1 << l) < C / 4 && l < 6) l++;
    return l;
}

}  // namespace

extern "C" {

size_t regtr_instnorm_bwd_ws_bytes(int n_clouds, int max_len, int C)
{
    if (!instnorm_bwd_shape_ok(n_clouds, max_len, C)) return 0;
    const size_t nchunk = (size_t)rg_cdiv(max_len > 0 ? max_len : 1, rg_in_rows(max_len, n_clouds, C));
    return rg_align_up(nchunk * n_clouds * C * 3 * sizeof(double), 256) + rg_align_up((size_t)n_clouds * C * sizeof(float4), 256);
}

int regtr_instnorm_bwd(const float* x, const int* seg_off, int n_clouds, int max_len, int C, const float* stats, const float* residual,
                       const float* res_stats, int act, float slope, const float* dy, float* dx, float* dres, void* ws, size_t ws_bytes,
                       void* stream)
{
    if (!instnorm_bwd_shape_ok(n_clouds, max_len, C) || (act != 0 && act != 1)) return RG_ERR_ARG;
    if (!x || !seg_off || !stats || !dy || (!dx && !dres) || (res_stats && !residual) || (dres && !residual)) return RG_ERR_ARG;
    if (misaligned(x) || misaligned(stats) || misaligned(dy) || misaligned(residual) || misaligned(res_stats) || misaligned(dx) ||
        misaligned(dres))
        return RG_ERR_ARG;
    const bool need_means = dx || res_stats;                  // a plain shortcut's gradient alone is g itself
    if (need_means && (!ws || misaligned(ws))) return RG_ERR_ARG;
    if (need_means && ws_bytes < regtr_instnorm_bwd_ws_bytes(n_clouds, max_len, C)) return RG_ERR_WORKSPACE;
    if (max_len == 0) return RG_OK;
    hipStream_t st = (hipStream_t)stream;
    const int rows = rg_in_rows(max_len, n_clouds, C);
    const int nchunk = rg_cdiv(max_len, rows);
    float4* means = nullptr;
    if (need_means) {
        RgCarver cv(ws, ws_bytes);
        double* partial = cv.take<double>((size_t)nchunk * n_clouds * C * 3);
        means = cv.take<float4>((size_t)n_clouds * C);
        if (!cv.ok()) return RG_ERR_WORKSPACE;
        k_instnorm_bwd_partial<<<dim3(nchunk, n_clouds), 256, 0, st>>>(x, seg_off, C, (const float2*)stats, residual, (const float2*)res_stats,
                                                                        act, slope, dy, nchunk, rows, partial);
        k_instnorm_bwd_finalize<<<dim3(rg_cdiv(C, 4), n_clouds), 256, 0, st>>>(partial, seg_off, C, nchunk, rows, means);
    }
    k_instnorm_bwd_apply<<<dim3(nchunk, n_clouds), 256, 0, st>>>(x, seg_off, C, (const float2*)stats, residual, (const float2*)res_stats, act,
                                                                  slope, dy, means, dx, dres, rows);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_maxpool_argmax(const float* x, int ns, int C, const int* nbr, int ld_nbr, int nq, int H, short* arg, void* stream)
{
    if (ns < 0 || nq < 0 || H < 1 || H > 32767 || ld_nbr < H || C < 4 || C % 4) return RG_ERR_ARG;
    if (nq == 0) return RG_OK;
    if (!nbr || !arg || (ns > 0 && !x) || misaligned(x) || ((uintptr_t)arg % 8)) return RG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (ns == 0) {                                            // no supports: every winner is the shadow row
        const size_t n = (size_t)nq * C;
        k_fill_i16<<<rg_cdiv((long long)n, 256), 256, 0, st>>>(arg, n, (short)-1);
    } else {
        const int l = lanes_log2(C);
        k_maxpool_argmax<<<rg_xcd_grid(rg_cdiv(nq, 4 << (6 - l))), 256, 0, st>>>(x, ns, C, nbr, ld_nbr, nq, H, l, arg);
    }
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_maxpool_fwd_argmax(const float* x, int ns, int C, const int* nbr, int ld_nbr, int nq, int H, float* out, short* arg, void* stream)
{
    if (ns < 0 || nq < 0 || H < 1 || H > 32767 || ld_nbr < H || C < 4 || C % 4) return RG_ERR_ARG;
    if (nq == 0) return RG_OK;
    if (!nbr || !out || !arg || (ns > 0 && !x) || misaligned(x) || misaligned(out) || ((uintptr_t)arg % 8)) return RG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (ns == 0) {                                            // no supports: every row is the zero shadow row
        const size_t n = (size_t)nq * C;
        if (hipMemsetAsync(out, 0, n * sizeof(float), st) != hipSuccess) return RG_ERR_LAUNCH;
        k_fill_i16<<<rg_cdiv((long long)n, 256), 256, 0, st>>>(arg, n, (short)-1);
    } else {
        const int l = lanes_log2(C);
        k_maxpool_fwd_argmax<<<rg_xcd_grid(rg_cdiv(nq, 4 << (6 - l))), 256, 0, st>>>(x, ns, C, nbr, ld_nbr, nq, H, l, out, arg);
    }
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_maxpool_gather_bwd(const float* dy, const short* arg, int nq, int H, int C, const int* row_off, const int* entries, int ns,
                             float* dx, void* stream)
{
    if (ns < 0 || nq < 0 || H < 1 || H > 32767 || C < 4 || C % 4 || (long long)nq * H >= (1LL << 31)) return RG_ERR_ARG;
    if (ns == 0) return RG_OK;
    if (!row_off || !dx || misaligned(dx) || (nq > 0 && (!dy || !arg || !entries || misaligned(dy) || ((uintptr_t)arg % 8)))) return RG_ERR_ARG;
    const int l = lanes_log2(C);
    k_maxpool_gather_bwd<<<rg_xcd_grid(rg_cdiv(ns, 4 << (6 - l))), 256, 0, (hipStream_t)stream>>>(dy, arg, nq, H, C, row_off, entries, ns,
                                                                                                  nq * H, l, dx);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
