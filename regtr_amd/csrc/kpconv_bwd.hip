// Backward of the KPConv operator for gfx950 (KPConv.forward, non-deformable / linear influence / sum aggregation:
// models/backbone_kpconv/kpconv_blocks.py:269-414 of the reference; forward kernels in kpconv.hip).
//
// With g[q, :] = dOut[q, :] / num[q] (regtr_row_div), dWF = g W^T is a dense product (regtr_gemm_f32 / _x3) and
// dW = WF^T g a tall transposed one (regtr_gemm_tn, or regtr_gemm_tn_any below for widths it refuses).  What is left is
//     dX[s, c] = sum over the entries (q, h) with nbr[q, h] == s of  sum_k infl[q, h, k] dWF[q, k Cin + c]
// -- a SCATTER over the neighbour table.  The backward kernels of this library are "one owner per output element, no
// floating-point atomics, bit-reproducible", so the table is transposed first:
//   * regtr_nbr_transpose     nbr [nq, H] -> CSR by support: row_off [ns + 1] and, per support, its incoming entries q H + h in
//                             ascending order.  Count (integer atomics: the counts do not depend on their order), exclusive scan,
//                             fill through an atomic cursor into a scratch list, then every support's list is put in ascending
//                             order by a rank sort (entries are distinct) -- the table is a pure function of nbr.  Shadow entries
//                             (index outside [0, ns)) are dropped.  Independent of KPConv: a max-pool backward walks the same table.
//   * regtr_kpconv_gather_bwd one wave owns one support row of dX.  Per incoming entry the 15 influences are recomputed from the
//                             coordinates with the forward's own statements (lanes = (entry, kernel point), staged in LDS), then
//                             lanes = channels add w_k dWF[q, k Cin + c] in (entry, k) order.  More than half of the 15 influences of an
//                             entry are exactly 0 (extent 0.8 R: an entry is in range of ~6 kernel points): those dWF rows are NOT
//                             read -- the load is steered to a dummy address, so the code stays branch free and only the rows that
//                             count move.
// Also here: regtr_gemm_tn_any (regtr_gemm_tn's split-K scheme with edge guards, any widths) and regtr_row_div.
#include "common.h"

namespace {

constexpr int KP_PAD = 16;
constexpr int BW_WAVES = 4;
constexpr int SCAN_ITEMS = 1024;      // counts per workgroup of the scan (256 threads x 4)

typedef float floatx4 __attribute__((ext_vector_type(4)));

inline bool misaligned(const void* p) { return ((uintptr_t)p % 16) != 0; }

// ------------------------------------------------------------------------------------------------ transposed neighbour table
__global__ void __launch_bounds__(256) k_nbrt_count(const int* __restrict__ nbr, int n_ent, int ns, int* __restrict__ cnt)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    const int idx = nbr[e];
    if ((unsigned)idx < (unsigned)ns) atomicAdd(&cnt[idx], 1);
}

__global__ void __launch_bounds__(256) k_scan_sums(const int* __restrict__ cnt, int n, int* __restrict__ bsum)
{
    __shared__ int sh[4];
    const int i0 = blockIdx.x * SCAN_ITEMS + threadIdx.x * 4;
    int s = 0;
    for (int u = 0; u < 4; u++) s += i0 + u < n ? cnt[i0 + u] : 0;
    int tot;
    rg_block_exclusive_scan<256>(s, &tot, sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of the nb block sums in place (thread t takes a contiguous run of them)
__global__ void __launch_bounds__(256) k_scan_bsums(int* __restrict__ bsum, int nb)
{
    __shared__ int sh[4];
    const int per = (nb + 255) / 256, b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    int s = 0;
    for (int b = b0; b < b1; b++) s += bsum[b];
    int tot;
    int run = rg_block_exclusive_scan<256>(s, &tot, sh);
    for (int b = b0; b < b1; b++) {
        const int v = bsum[b];
        bsum[b] = run;
        run += v;
    }
}

// counts -> exclusive offsets, in place (cnt has n + 1 slots: the last receives the total), and the fill cursors
__global__ void __launch_bounds__(256) k_scan_apply(int* __restrict__ cnt, int n, const int* __restrict__ bsum, int* __restrict__ cursor)
{
    __shared__ int sh[4];
    const int i0 = blockIdx.x * SCAN_ITEMS + threadIdx.x * 4;
    int v[4], s = 0;
    for (int u = 0; u < 4; u++) {
        v[u] = i0 + u < n ? cnt[i0 + u] : 0;
        s += v[u];
    }
    int tot;
    int run = rg_block_exclusive_scan<256>(s, &tot, sh) + bsum[blockIdx.x];
    for (int u = 0; u < 4; u++) {
        if (i0 + u < n) {
            cnt[i0 + u] = run;
            cursor[i0 + u] = run;
        }
        run += v[u];
        if (i0 + u == n - 1) cnt[n] = run;
    }
}

__global__ void __launch_bounds__(256) k_nbrt_fill(const int* __restrict__ nbr, int n_ent, int ns, int* __restrict__ cursor,
                                                   int* __restrict__ tmp)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    const int idx = nbr[e];
    if ((unsigned)idx < (unsigned)ns) tmp[atomicAdd(&cursor[idx], 1)] = e;      // (slot order: any; k_nbrt_sort fixes it)
}

// One wave per support: its entries (distinct integers, in the order the cursor dealt them) go out in ascending order -- every entry
// to the slot given by the number of smaller entries of the list.  Lists of up to 64 entries (all of them on real tables: a support
// is listed by the queries around it) are ranked in registers, longer ones (a hub) against the scratch list in memory.
__global__ void __launch_bounds__(256) k_nbrt_sort(const int* __restrict__ row_off, int ns, const int* __restrict__ tmp,
                                                   int* __restrict__ ent)
{
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= ns) return;
    const int lane = rg_lane();
    const int b = row_off[s], n = row_off[s + 1] - b;
    if (n <= RG_WAVE) {
        const int v = lane < n ? tmp[b + lane] : 0x7fffffff;
        int rank = 0;
        for (int j = 0; j < n; j++) rank += __shfl(v, j, RG_WAVE) < v ? 1 : 0;
        if (lane < n) ent[b + rank] = v;
        return;
    }
    for (int i = lane; i < n; i += RG_WAVE) {
        const int v = tmp[b + i];
        int rank = 0;
        for (int j = 0; j < n; j++) rank += tmp[b + j] < v ? 1 : 0;
        ent[b + rank] = v;
    }
}

// ------------------------------------------------------------------------------------------------ dX
struct GatherBwdArgs {
    const float* dwf; const float* q_xyz; const float* s_xyz; const float* kp; const int* row_off; const int* ent; float* dx;
    int nq, ns, H, Cin, KP, n_ent;
    float extent;
};

// LC lanes serve one entry (channel c = lane % LC + n LC, n < NC), so a wave walks G = 64 / LC entries side by side; the G partial
// sums of a channel are added by a fixed xor tree at the end.  Entries are staged B at a time: lanes = (entry of the batch, kernel
// point) compute the influences into LDS, then lanes = channels consume them.
template <int LC, int NC>
__global__ void __launch_bounds__(BW_WAVES * RG_WAVE) k_kpconv_gather_bwd(GatherBwdArgs g)
{
    constexpr int G = RG_WAVE / LC;
    constexpr int B = G > 4 ? G : 4;
    constexpr int EPS = B / G;              // entries per slot and batch
    __shared__ __align__(16) float w_sh[BW_WAVES][B][KP_PAD];
    __shared__ int q_sh[BW_WAVES][B];
    const int wave = threadIdx.x >> 6, lane = rg_lane();
    const int s = rg_xcd_block(blockIdx.x, gridDim.x) * BW_WAVES + wave;      // XCD-contiguous support ranges: neighbours share dWF rows
    if (s >= g.ns) return;                  // wave-uniform
    const int Cin = g.Cin, KP = g.KP;
    int e0 = g.row_off[s], e1 = g.row_off[s + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > g.n_ent ? g.n_ent : e1;       // (a table that is not this nbr's cannot make the walk leave the entry list)
    const float sx = g.s_xyz[3 * (size_t)s], sy = g.s_xyz[3 * (size_t)s + 1], sz = g.s_xyz[3 * (size_t)s + 2];
    const int k = lane & (KP_PAD - 1);
    const bool kvalid = k < KP;
    const int kc = kvalid ? k : 0;
    const float kx = g.kp[3 * kc], ky = g.kp[3 * kc + 1], kz = g.kp[3 * kc + 2];
    const float inv_extent = 1.0f / g.extent;
    const int slot = lane / LC, cl = lane % LC;
    const size_t row_len = (size_t)KP * Cin;
    float acc[NC];
#pragma unroll
    for (int n = 0; n < NC; n++) acc[n] = 0.f;

    for (int i0 = e0; i0 < e1; i0 += B) {
        __builtin_amdgcn_wave_barrier();
        // ---- influences of the batch's entries: the forward's statements (kpconv.hip, k_kpconv_gather_mfma)
        for (int t = lane; t < B * KP_PAD; t += RG_WAVE) {
            const int eb = t >> 4, i = i0 + eb;
            float w = 0.f;
            int q = 0;
            if (i < e1) {
                q = g.ent[i] / g.H;
                q = q < 0 ? 0 : (q >= g.nq ? g.nq - 1 : q);
                const float rx = sx - g.q_xyz[3 * (size_t)q], ry = sy - g.q_xyz[3 * (size_t)q + 1], rz = sz - g.q_xyz[3 * (size_t)q + 2];
                const float dx = rx - kx, dy = ry - ky, dz = rz - kz;
                float d2;
                {
#pragma clang fp contract(off)
                    d2 = (dx * dx + dy * dy) + dz * dz;                               // kpconv_blocks.py:326-329
                }
                w = fmaxf(__builtin_fmaf(__builtin_amdgcn_sqrtf(d2), -inv_extent, 1.f), 0.f);      // :368
                if (!kvalid) w = 0.f;
            }
            w_sh[wave][eb][k] = w;
            if (k == 0) q_sh[wave][eb] = q;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- lanes = channels.  All loads of an entry are issued before its first fma; a zero influence reads the dummy word.
#pragma unroll
        for (int j = 0; j < EPS; j++) {
            const int eb = slot + G * j;
            const float* row = g.dwf + (size_t)q_sh[wave][eb] * row_len;
            float w[KP_PAD];
#pragma unroll
            for (int k4 = 0; k4 < KP_PAD / 4; k4++) {
                const float4 t = *(const float4*)&w_sh[wave][eb][4 * k4];
                w[4 * k4] = t.x; w[4 * k4 + 1] = t.y; w[4 * k4 + 2] = t.z; w[4 * k4 + 3] = t.w;
            }
            float v[KP_PAD][NC];
#pragma unroll
            for (int kk = 0; kk < KP_PAD; kk++)
#pragma unroll
                for (int n = 0; n < NC; n++) {
                    const int c = cl + n * LC;
                    const float* p = (w[kk] != 0.f && c < Cin) ? row + (size_t)kk * Cin + c : g.kp;
                    v[kk][n] = *p;
                }
#pragma unroll
            for (int kk = 0; kk < KP_PAD; kk++)
#pragma unroll
                for (int n = 0; n < NC; n++) acc[n] = fmaf(w[kk], v[kk][n], acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < NC; n++) {
#pragma unroll
        for (int o = RG_WAVE / 2; o >= LC; o >>= 1) acc[n] += __shfl_xor(acc[n], o, RG_WAVE);
        const int c = cl + n * LC;
        if (slot == 0 && c < Cin) g.dx[(size_t)s * Cin + c] = acc[n];
    }
}

// ------------------------------------------------------------------------------------------------ dW for any widths
// regtr_gemm_tn's scheme (losses.hip) with guarded edges: workgroup (tm, tn, z) sums rows [z chunk, (z + 1) chunk) of one 64 x 64
// tile of a^T b on the f32 MFMA into its own partial slot; a second launch adds the slots in z order in float64.
constexpr int TN_TILE = 64;

__global__ void __launch_bounds__(256) k_gemm_tn_any_part(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb,
                                                          int M, int N1, int N2, int chunk, float* __restrict__ part)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, grp = lane >> 4;
    const int m0 = TN_TILE * blockIdx.x + 16 * wave, n0 = TN_TILE * blockIdx.y;
    const int k0 = blockIdx.z * chunk, k1 = min(M, k0 + chunk);
    const bool a_ok = m0 + col < N1;
    bool b_ok[4];
#pragma unroll
    for (int n = 0; n < 4; n++) b_ok[n] = n0 + 16 * n + col < N2;
    floatx4 acc[4] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 4
    for (int k = k0; k < k1; k += 4) {
        const int kk = k + grp;
        const bool ok = kk < k1;
        const float av = (ok && a_ok) ? A[(size_t)kk * lda + m0 + col] : 0.f;
        const float* br = Bm + (size_t)(ok ? kk : k0) * ldb + n0 + col;
#pragma unroll
        for (int n = 0; n < 4; n++) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, (ok && b_ok[n]) ? br[16 * n] : 0.f, acc[n], 0, 0, 0);
    }
    float* dst = part + (size_t)blockIdx.z * N1 * N2;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int n = 0; n < 4; n++)
            if (m0 + 4 * grp + r < N1 && b_ok[n]) dst[(size_t)(m0 + 4 * grp + r) * N2 + n0 + 16 * n + col] = acc[n][r];
}

__global__ void __launch_bounds__(256) k_gemm_tn_any_reduce(const float* __restrict__ part, int splits, int N1, int N2, float* __restrict__ out,
                                                            int ldo)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N1 * N2) return;
    const int i = idx / N2, j = idx - i * N2;
    const size_t plane = (size_t)N1 * N2;
    double v = 0.0;
    for (int z = 0; z < splits; z++) v += part[z * plane + idx];
    out[(size_t)i * ldo + j] = (float)v;
}

// rows per split: a function of (M, N1, N2) only
int tn_any_splits(int M, int N1, int N2, int& chunk)
{
    const int tiles = rg_cdiv(N1, TN_TILE) * rg_cdiv(N2, TN_TILE);
    const int target = rg_cdiv(2048, tiles);
    chunk = rg_cdiv(rg_cdiv(M > 0 ? M : 1, target), 4) * 4;
    if (chunk < 64) chunk = 64;
    return M > 0 ? rg_cdiv(M, chunk) : 1;
}

__global__ void __launch_bounds__(256) k_row_div(const float* __restrict__ x, int ldx, const float* __restrict__ div, int n, int N,
                                                 float* __restrict__ out, int ldo)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * N) return;
    const size_t r = idx / N;
    const int c = (int)(idx - r * N);
    out[r * ldo + c] = x[r * ldx + c] / div[r];
}

}  // namespace

extern "C" {

size_t regtr_nbr_transpose_ws_bytes(int nq, int H, int ns)
{
    if (nq < 0 || ns < 0 || H < 1 || (long long)nq * H >= (1LL << 31)) return 0;
    // cursor [ns] | block sums | scratch entry list [nq H]
    return rg_align_up((size_t)(ns > 0 ? ns : 1) * sizeof(int), 256) + rg_align_up((size_t)(rg_cdiv(ns, SCAN_ITEMS) + 1) * sizeof(int), 256) +
           rg_align_up((size_t)(nq > 0 ? nq : 1) * H * sizeof(int), 256);
}

int regtr_nbr_transpose(const int* nbr, int nq, int H, int ns, int* row_off, int* entries, void* ws, size_t ws_bytes, void* stream)
{
    if (nq < 0 || ns < 0 || H < 1 || (long long)nq * H >= (1LL << 31)) return RG_ERR_ARG;
    if (!row_off) return RG_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int n_ent = nq * H;
    if (n_ent == 0 || ns == 0) {        // an empty table: every support has an empty list
        if (hipMemsetAsync(row_off, 0, (size_t)(ns + 1) * sizeof(int), st) != hipSuccess) return RG_ERR_LAUNCH;
        return RG_OK;
    }
    if (!nbr || !entries || !ws) return RG_ERR_ARG;
    if (ws_bytes < regtr_nbr_transpose_ws_bytes(nq, H, ns)) return RG_ERR_WORKSPACE;
    RgCarver cv(ws, ws_bytes);
    const int nb = rg_cdiv(ns, SCAN_ITEMS);
    int* cursor = cv.take<int>(ns);
    int* bsum = cv.take<int>(nb + 1);
    int* tmp = cv.take<int>(n_ent);
    if (!cv.ok()) return RG_ERR_WORKSPACE;
    if (hipMemsetAsync(row_off, 0, (size_t)(ns + 1) * sizeof(int), st) != hipSuccess) return RG_ERR_LAUNCH;
    k_nbrt_count<<<rg_cdiv(n_ent, 256), 256, 0, st>>>(nbr, n_ent, ns, row_off);
    k_scan_sums<<<nb, 256, 0, st>>>(row_off, ns, bsum);
    k_scan_bsums<<<1, 256, 0, st>>>(bsum, nb);
    k_scan_apply<<<nb, 256, 0, st>>>(row_off, ns, bsum, cursor);
    k_nbrt_fill<<<rg_cdiv(n_ent, 256), 256, 0, st>>>(nbr, n_ent, ns, cursor, tmp);
    k_nbrt_sort<<<rg_cdiv(ns, 4), 256, 0, st>>>(row_off, ns, tmp, entries);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_kpconv_gather_bwd(const float* dwf, const float* q_xyz, int nq, const float* s_xyz, int ns, int H, int Cin,
                            const float* kernel_points, int KP, float extent, const int* row_off, const int* entries, float* dx,
                            void* stream)
{
    if (nq < 0 || ns < 0 || H < 1 || H > 448 || Cin < 1 || Cin > 256 || KP < 1 || KP > KP_PAD || !(extent > 0.f) ||
        (long long)nq * H >= (1LL << 31))
        return RG_ERR_ARG;
    if (ns == 0) return RG_OK;
    if (!s_xyz || !kernel_points || !row_off || !dx || (nq > 0 && (!dwf || !q_xyz || !entries))) return RG_ERR_ARG;
    if (misaligned(dwf) || misaligned(dx)) return RG_ERR_ARG;
    GatherBwdArgs g{dwf, q_xyz, s_xyz, kernel_points, row_off, entries, dx, nq, ns, H, Cin, KP, nq * H, extent};
    hipStream_t st = (hipStream_t)stream;
    const int grid = rg_xcd_grid(rg_cdiv(ns, BW_WAVES));
    if (Cin == 1) k_kpconv_gather_bwd<1, 1><<<grid, BW_WAVES * RG_WAVE, 0, st>>>(g);
    else if (Cin <= 32) k_kpconv_gather_bwd<32, 1><<<grid, BW_WAVES * RG_WAVE, 0, st>>>(g);
    else if (Cin <= 64) k_kpconv_gather_bwd<64, 1><<<grid, BW_WAVES * RG_WAVE, 0, st>>>(g);
    else if (Cin <= 128) k_kpconv_gather_bwd<64, 2><<<grid, BW_WAVES * RG_WAVE, 0, st>>>(g);
    else k_kpconv_gather_bwd<64, 4><<<grid, BW_WAVES * RG_WAVE, 0, st>>>(g);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

size_t regtr_gemm_tn_any_ws_bytes(int M, int N1, int N2)
{
    if (M < 0 || N1 <= 0 || N2 <= 0 || (long long)N1 * N2 >= (1LL << 28)) return 0;
    int chunk;
    return (size_t)tn_any_splits(M, N1, N2, chunk) * N1 * N2 * sizeof(float);
}

int regtr_gemm_tn_any(const float* a, int lda, const float* b, int ldb, int M, int N1, int N2, float* out, int ldo, void* ws,
                      size_t ws_bytes, void* stream)
{
    if (M < 0 || N1 <= 0 || N2 <= 0 || (long long)N1 * N2 >= (1LL << 28)) return RG_ERR_ARG;
    if (lda < N1 || ldb < N2 || ldo < N2) return RG_ERR_ARG;
    if (!out || !ws || (M > 0 && (!a || !b))) return RG_ERR_ARG;
    if (ws_bytes < regtr_gemm_tn_any_ws_bytes(M, N1, N2)) return RG_ERR_WORKSPACE;
    int chunk;
    const int splits = tn_any_splits(M, N1, N2, chunk);
    const hipStream_t s = (hipStream_t)stream;
    k_gemm_tn_any_part<<<dim3(rg_cdiv(N1, TN_TILE), rg_cdiv(N2, TN_TILE), splits), 256, 0, s>>>(a, lda, b, ldb, M, N1, N2, chunk, (float*)ws);
    RG_RETURN_IF_LAUNCH_FAILED();
    k_gemm_tn_any_reduce<<<rg_cdiv((long long)N1 * N2, 256), 256, 0, s>>>((const float*)ws, splits, N1, N2, out, ldo);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_row_div(const float* x, int ldx, const float* div, int n, int N, float* out, int ldo, void* stream)
{
    if (n < 0 || N < 1 || ldx < N || ldo < N) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    if (!x || !div || !out) return RG_ERR_ARG;
    k_row_div<<<rg_cdiv((long long)n * N, 256), 256, 0, (hipStream_t)stream>>>(x, ldx, div, n, N, out, ldo);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
