// KPConv irregular neighbour gather + kernel-point correlation for gfx950, and the strided-block max-pool gather.
// Reference: KPConv.forward (non-deformable, 'linear' influence, 'sum' aggregation)
//   /root/reference/src/models/backbone_kpconv/kpconv_blocks.py:269-414, max_pool :127-143.
//
// The reference materialises (Nq,H,15,3) differences, (Nq,H,15) influences and (Nq,H,Cin) gathered features as
// separate tensors; here they never exist.  Three kernels, chosen by the launcher from Cin:
//   k_kpconv_gather_mfma<J,V>  Cin a multiple of 32 (every block of both shipped configs but the first): the per-query
//                              correlation runs on the f32 matrix cores, see the comment above the kernel;
//   k_kpconv_gather_c1         Cin == 1 (first block, features = ones): lanes = (query, kernel point);
//   k_kpconv_gather<LQ>        any other Cin -- the general LDS-tile form:
//     phase 1  lanes = neighbours: coalesced read of the index row, gather of the neighbour xyz, centred offsets and the
//              "feature sum > 0" flags into LDS;
//     phase 2  lanes = (neighbour, kernel point): 15 linear influences max(0, 1 - |y - kp_k| / extent) into an LDS-staged
//              [H][16] tile (each lane keeps its kernel point in registers);
//     phase 3  lanes = channels: the neighbour feature rows are gathered once (row-contiguous, line-sized reads),
//              influences are broadcast from LDS as 128-bit reads and 15 accumulators per channel stay in registers.
// Output is the weighted-feature matrix WF[q][k*Cin + c] that feeds the kernel-point contraction with the
// [15*Cin, Cout] weights (gemm_x3.hip / gemm.hip), plus the reference's data-dependent normaliser
//   num[q] = max(1, #{h : sum_c x[n_qh, c] > 0})            kpconv_blocks.py:409-411
// which the GEMM epilogue divides by.
#include "common.h"
#include <type_traits>

namespace {

constexpr int KP_PAD = 16;   // kernel points padded to 16 per neighbour (15 used)
constexpr int GATHER_WAVES = 4;

// flag[j] = (sum_c x'[j, c] > 0) for every support row, x' = x or lrelu(InstanceNorm(x)) when stats are given;
// the shadow row (index ns) is 0 by construction.
__global__ void __launch_bounds__(256) k_rowsum_positive(const float* __restrict__ x, int n, int C, const float2* __restrict__ stats,
                                                         const int* __restrict__ seg_off, int n_seg, float slope,
                                                         float* __restrict__ flag)
{
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = rg_lane();
    const float2* st = stats ? stats + (size_t)rg_find_segment(seg_off, n_seg, row) * C : nullptr;
    float s = 0.f;
    for (int c = lane; c < C; c += RG_WAVE) {
        float v = x[(size_t)row * C + c];
        if (st) { v = (v - st[c].x) * st[c].y; v = v > 0.f ? v : v * slope; }
        s += v;
    }
    s = rg_wave_sum(s);
    if (lane == 0) flag[row] = s > 0.f ? 1.f : 0.f;
}

struct GatherArgs {
    const float* q_xyz; const float* s_xyz; const int* nbr; const float* x; const float* flag; const float* s_xyzf; const float* kp;
    float* wf; float* num;
    const float2* x_stats; const int* q_seg_off;     // optional fused lrelu(InstanceNorm(x)) on the gathered features
    int nq, ns, H, Cin, KP, n_seg, ld_wf;
    float extent, slope;
    int qpw;      // k_kpconv_gather_mfma: queries each wave handles one after another (<= MG_QPW; fewer on small launches)
};

// LQ = lanes per query (16, 32 or 64); a wave handles 64 / LQ queries at a time.
template <int LQ>
__global__ void __launch_bounds__(GATHER_WAVES * RG_WAVE) k_kpconv_gather(GatherArgs g)
{
    constexpr int QW = RG_WAVE / LQ;
    extern __shared__ __align__(16) float smem[];
    const int wave = threadIdx.x >> 6, lane = rg_lane();
    const int H = g.H;
    // per-wave LDS: w[QW][H][16] | rel[QW][H][3] | nidx[QW][H] | flag[QW][H] | x[QW][H] (Cin == 1 only)
    const int per_wave = (QW * H * (KP_PAD + 6) + 3) & ~3;   // keep every wave's tile 16-B aligned
    float* w_s = smem + (size_t)wave * per_wave;
    float* rel_s = w_s + QW * H * KP_PAD;
    int* idx_s = (int*)(rel_s + QW * H * 3);
    float* flg_s = (float*)(idx_s + QW * H);
    float* xs_s = flg_s + QW * H;

    const int q0 = (rg_xcd_block(blockIdx.x, gridDim.x) * GATHER_WAVES + wave) * QW;      // XCD-contiguous query ranges
    if (q0 >= g.nq) return;   // wave-uniform

    // ---- phase 1: neighbour indices, centred offsets, positivity flags
    for (int e = lane; e < QW * H; e += RG_WAVE) {
        const int qi = e / H, h = e - qi * H, q = q0 + qi;
        int idx = g.ns;
        float rx = 1e6f, ry = 1e6f, rz = 1e6f, f = 0.f, x1 = 0.f;
        if (q < g.nq) {
            idx = g.nbr[(size_t)q * H + h];
            float sx = 1e6f, sy = 1e6f, sz = 1e6f;            // shadow support point  (kpconv_blocks.py:309)
            if (idx < g.ns) {
                sx = g.s_xyz[3 * (size_t)idx]; sy = g.s_xyz[3 * (size_t)idx + 1]; sz = g.s_xyz[3 * (size_t)idx + 2];
                f = g.flag[idx];
                if (g.Cin == 1) x1 = g.x[idx];
            }
            rx = sx - g.q_xyz[3 * (size_t)q]; ry = sy - g.q_xyz[3 * (size_t)q + 1]; rz = sz - g.q_xyz[3 * (size_t)q + 2];
        }
        idx_s[e] = idx; flg_s[e] = f; xs_s[e] = x1;
        rel_s[3 * e] = rx; rel_s[3 * e + 1] = ry; rel_s[3 * e + 2] = rz;
    }
    __builtin_amdgcn_wave_barrier();

    // ---- phase 2: linear influences; lane's kernel point is fixed (k = lane % 16)
    {
        const int k = lane & (KP_PAD - 1);
        const bool kvalid = k < g.KP;
        const float kx = kvalid ? g.kp[3 * k] : 0.f, ky = kvalid ? g.kp[3 * k + 1] : 0.f, kz = kvalid ? g.kp[3 * k + 2] : 0.f;
        const float inv_extent = 1.0f / g.extent;
        for (int e = lane; e < QW * H * KP_PAD; e += RG_WAVE) {
            const int qh = e >> 4;   // (qi*H + h)
            const float dx = rel_s[3 * qh] - kx, dy = rel_s[3 * qh + 1] - ky, dz = rel_s[3 * qh + 2] - kz;
            float d2;
            {
#pragma clang fp contract(off)
                d2 = (dx * dx + dy * dy) + dz * dz;                               // kpconv_blocks.py:326-329
            }
            // :368  1 - sqrt(d2)/extent with the hardware sqrt (1 ulp) and a precomputed reciprocal: |error| <~ 2e-7
            float wv = 1.f - __builtin_amdgcn_sqrtf(d2) * inv_extent;
            w_s[e] = (kvalid && wv > 0.f) ? wv : 0.f;
        }
    }
    __builtin_amdgcn_wave_barrier();

    // ---- phase 3: lanes = channels of one query
    const int qi = lane / LQ, cl = lane % LQ, q = q0 + qi;
    if (q >= g.nq) return;
    const float* wq = w_s + (size_t)qi * H * KP_PAD;
    const int* iq = idx_s + qi * H;
    const int Cin = g.Cin;
    {
        const float2* st = nullptr;
        if (g.x_stats) st = g.x_stats + (size_t)rg_find_segment(g.q_seg_off, g.n_seg, q) * Cin;
        for (int c = cl; c < Cin; c += LQ) {
            float acc[KP_PAD];
#pragma unroll
            for (int k = 0; k < KP_PAD; k++) acc[k] = 0.f;
            float mu = 0.f, rs = 1.f;
            if (st) { mu = st[c].x; rs = st[c].y; }
            // neighbour rows are fetched 8 at a time before any of them is consumed: 8 independent gathers in flight per
            // lane hide the L2 / Infinity-Cache latency that a load-use chain per neighbour would expose
            for (int h0 = 0; h0 < H; h0 += 8) {
                float xv[8];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int h = h0 + u;
                    const int idx = h < H ? iq[h] : g.ns;
                    xv[u] = idx < g.ns ? g.x[(size_t)idx * Cin + c] : 0.f;          // zero shadow feature (:388)
                    if (st && idx < g.ns) { const float t = (xv[u] - mu) * rs; xv[u] = t > 0.f ? t : t * g.slope; }
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int h = h0 + u;
                    if (h < H) {
                        const float4* w4 = (const float4*)(wq + h * KP_PAD);
#pragma unroll
                        for (int j = 0; j < KP_PAD / 4; j++) {
                            const float4 wv = w4[j];
                            acc[4 * j + 0] = fmaf(wv.x, xv[u], acc[4 * j + 0]);
                            acc[4 * j + 1] = fmaf(wv.y, xv[u], acc[4 * j + 1]);
                            acc[4 * j + 2] = fmaf(wv.z, xv[u], acc[4 * j + 2]);
                            acc[4 * j + 3] = fmaf(wv.w, xv[u], acc[4 * j + 3]);
                        }
                    }
                }
            }
            float* o = g.wf + (size_t)q * g.KP * Cin + c;
#pragma unroll
            for (int k = 0; k < KP_PAD; k++)
                if (k < g.KP) o[(size_t)k * Cin] = acc[k];
        }
    }
    if (cl == 0) {
        float cnt = 0.f;
        const float* fq = flg_s + qi * H;
        for (int h = 0; h < H; h++) cnt += fq[h];
        g.num[q] = fmaxf(cnt, 1.f);                                               // :410-411
    }
}


// ------------------------------------------------------------------------------------------------------------------
// Matrix-core gather (Cin a multiple of 32).  For one query the kernel-point correlation
//   WF[k, c] = sum_h w[h, k] * x[n_h, c]
// is a [16 x H] x [H x Cin] product, so it runs on v_mfma_f32_16x16x4_f32 (exact f32, an fmaf chain over h in order):
//   A operand  lane (k = l & 15, hh = l >> 4)  holds  w[h = 4 j + hh][k]  -- computed by that very lane from the centred
//              neighbour offset and ITS kernel point, so influences go from the VALU straight into the MFMA with no LDS
//              tile and no broadcast reads;
//   B operand  lane (n = l & 15, hh)  holds  x[n_{4 j + hh}][c0 + V n + v], v < V: ONE 8- or 16-byte load per lane per
//              neighbour group, the 16 lanes of a group reading one whole 128-B / 256-B feature row segment; component
//              v feeds MFMA v, whose output column n therefore is channel c0 + V n + v.  All J loads of a pass are
//              issued before the first MFMA, so tens of KB per CU are in flight and L2 / Infinity-Cache latency hides;
//   D          lane holds WF[k = 4 hh + r][c0 + V n + v] in acc[v][r]: V consecutive channels -> one 8/16-byte store.
// The per-support positivity flag of the normaliser (kpconv_blocks.py:409-410) is a row sum over the very channels the
// wave has just gathered: per-lane partial sums + a 4-step DPP rotate-add over the 16 lanes of a group, so no separate
// pass over x (and no flag gather) is needed.
// ------------------------------------------------------------------------------------------------------------------
typedef float floatx4 __attribute__((ext_vector_type(4)));
#ifndef RG_MG_QPW
#define RG_MG_QPW 8
#endif
constexpr int MG_QPW = RG_MG_QPW;      // queries handled one after another by each wave

template <int V> struct RgVec;
template <> struct RgVec<2> { typedef float2 type; };
template <> struct RgVec<4> { typedef float4 type; };
__device__ __forceinline__ float rg_comp(const float2& v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ float rg_comp(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }
__device__ __forceinline__ void rg_set(float2& v, int i, float f) { if (i == 0) v.x = f; else v.y = f; }
__device__ __forceinline__ void rg_set(float4& v, int i, float f) { if (i == 0) v.x = f; else if (i == 1) v.y = f; else if (i == 2) v.z = f; else v.w = f; }

// sum over the 16 lanes of a DPP row (every lane of the row ends with the same, order-symmetric total)
__device__ __forceinline__ float rg_row16_sum(float v)
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));   // row_ror:8
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));   // row_ror:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));   // row_ror:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));   // row_ror:1
    return v;
}

typedef unsigned rg_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned rg_u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned RG_OOB = 0x80000000u;      // byte offset beyond any buffer this kernel binds (all are < 2 GiB)

// Raw buffer access (buffer_load/store ... offen): 32-bit byte offsets against a scalar resource -- one address VGPR per
// access instead of a 64-bit pair plus the VALU that builds it -- and hardware range checking: an offset of RG_OOB
// loads zeros / drops the store, which is exactly the "shadow row" (kpconv_blocks.py:388) and the k >= KP mask.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rg_rsrc(const void* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
template <int V> __device__ __forceinline__ typename RgVec<V>::type rg_buf_load(__amdgpu_buffer_rsrc_t r, unsigned off);
template <> __device__ __forceinline__ float2 rg_buf_load<2>(__amdgpu_buffer_rsrc_t r, unsigned off)
{
    const rg_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
    return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
}
template <> __device__ __forceinline__ float4 rg_buf_load<4>(__amdgpu_buffer_rsrc_t r, unsigned off)
{
    const rg_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
// Cache policy of the WF stores: nt (non-temporal, aux bit 1).  WF is written once, read once by the next kernel and is far
// larger than every cache (4.6 GB at level 0 of a 64-pair forward): as default-policy stores it evicted the feature rows the
// gather re-reads ~40 times from L2.  Measured on MI355X (tools/gather_bench.py, 64 pairs): all gather launches of a forward
// 5.40 -> 4.94 ms (Cin 64: 950 -> 786 us, Cin 128: 438 -> 358 us); without any store they take 4.42 ms.
#ifndef RG_WF_STORE_AUX
#define RG_WF_STORE_AUX 2
#endif
__device__ __forceinline__ void rg_buf_store(__amdgpu_buffer_rsrc_t r, unsigned off, const float2& v)
{
    __builtin_amdgcn_raw_buffer_store_b64(rg_u32x2{__float_as_uint(v.x), __float_as_uint(v.y)}, r, off, 0, RG_WF_STORE_AUX);
}
__device__ __forceinline__ void rg_buf_store(__amdgpu_buffer_rsrc_t r, unsigned off, const float4& v)
{
    __builtin_amdgcn_raw_buffer_store_b128(rg_u32x4{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}, r, off, 0, RG_WF_STORE_AUX);
}

typedef float rg_f32x2 __attribute__((ext_vector_type(2)));
#ifndef RG_MG_WAVES_PER_EU
#define RG_MG_WAVES_PER_EU 3
#endif
// Per-query neighbour-group count.  A table row is padded with shadows up to H: on the shipped workloads 31 of 40 slots are real (mean;
// DESIGN.md par. 6) and the highest real slot ends 8.1 of the 10 groups.  A group behind it adds (+0) * (finite) to accumulators that
// start at +0 and can therefore never be -0: leaving it out is the identity, bit for bit.  Each query runs through a body compiled for a
// FIXED group count JJ -- the smallest offered value >= jn = ceil((highest real slot + 1) / 4) -- so every body stays branch free inside
// (a guarded load becomes branch / load / vmcnt(0)).  Offered: J, J - STEP, ... (BODIES of them); a body is shadow-safe, so the smallest
// one takes every lower count, jn = 0 (no real neighbour: WF rows of zeros, num 1) included.  The count comes from the HIGHEST real slot,
// not the number of real slots: nothing assumes that shadows are a suffix of the row.
// Measured on MI355X (64-pair tables, same process, alternating, bit-equal outputs; profiles/r07_gather_groups.md): level-0 convolution
// 2050 us with the one fixed-J body, 1940 with bodies {J - 4, J - 2, J}, 1920 with every count 1 ... J, 1898 with the six J - 5 ... J kept
// here (3 % of the rows need fewer: 0.818 of the groups run against 0.814); the gathers of a forward 6.56 -> 6.33 / 6.16 / 6.10 ms.
#ifndef RG_MG_GROUP_STEP
#define RG_MG_GROUP_STEP 1
#endif
#ifndef RG_MG_GROUP_BODIES
#define RG_MG_GROUP_BODIES 6
#endif
// An instantiation that would lose a wave per SIMD to the extra bodies keeps the one fixed-J body.
template <int J, int V, bool PRE> constexpr int rg_mg_bodies() { return RG_MG_GROUP_BODIES; }
template <> constexpr int rg_mg_bodies<10, 2, false>() { return 1; }      // 94 -> 108 VGPRs: 5 -> 4 waves per SIMD
template <int JJ, int JMIN, typename F>
__device__ __forceinline__ void rg_for_group_count(int jn, F&& body)      // jn wave-uniform: scalar branches
{
    if constexpr (JJ - RG_MG_GROUP_STEP >= JMIN) {
        if (jn <= JJ - RG_MG_GROUP_STEP) { rg_for_group_count<JJ - RG_MG_GROUP_STEP, JMIN>(jn, body); return; }
    }
    body(std::integral_constant<int, JJ>{});
}
// PRE: g.s_xyzf holds (x, y, z, positivity flag) records and the features are final (no InstanceNorm fold) -- the launcher's choice
// when the caller passes `s_xyzf` and no x_stats.  Per neighbour ONE 16-byte load replaces three coordinate dwords (plus the flag):
// PMC on the level-0 launch showed the texture-address path 76 % busy, 148 of ~260 lines per query being those scattered dwords,
// and waves 68 % of their time in issue stalls behind it; per query ~170 of ~290 VALU instructions (fold, row sums) go as well.
template <int J, int V, bool PRE>    // J = ceil(H / 4) neighbour groups (H <= 4 J); V floats per lane per row per pass
__global__ void __launch_bounds__(GATHER_WAVES * RG_WAVE, RG_MG_WAVES_PER_EU) k_kpconv_gather_mfma(GatherArgs g)
{
    typedef typename RgVec<V>::type vec;
    constexpr int HP = 4 * J;
    __shared__ float4 nb_sh[GATHER_WAVES][HP];        // (rel.x, rel.y, rel.z, feature-row byte offset) per neighbour
    // readfirstlane: tells the compiler the wave index (hence q and everything derived from it) is wave-uniform, so the
    // per-query buffer resource lives in SGPRs instead of being "waterfalled" lane by lane
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = rg_lane();
    const int k = lane & 15, hh = lane >> 4;
    const int H = g.H, Cin = g.Cin, ns = g.ns, nq = g.nq;
    float4* nb_s = nb_sh[wave];
    const bool kvalid = k < g.KP;
    const int kc = kvalid ? k : 0;
    // a lane without a kernel point (k = 15) sits infinitely far away: its influence clamps to 0 with no extra select
    const float kx = kvalid ? g.kp[3 * kc] : 1e30f, ky = g.kp[3 * kc + 1], kz = g.kp[3 * kc + 2];
    const float inv_extent = 1.0f / g.extent;
    const unsigned row_bytes = (unsigned)Cin * 4u;
    const __amdgpu_buffer_rsrc_t x_rs = rg_rsrc(g.x, (unsigned)ns * row_bytes);
    const __amdgpu_buffer_rsrc_t sxyz_rs = rg_rsrc(g.s_xyz, (unsigned)ns * 12u);
    const __amdgpu_buffer_rsrc_t xyzf_rs = rg_rsrc(PRE ? g.s_xyzf : g.s_xyz, PRE ? (unsigned)ns * 16u : 0u);
    const unsigned lane_off = (unsigned)(V * k) * 4u;                 // this lane's channel bytes within a 16 V pass
    unsigned st_off[4];                                               // WF store offsets of the lane's 4 kernel-point rows
#pragma unroll
    for (int r = 0; r < 4; r++) st_off[r] = (4 * hh + r) < g.KP ? (unsigned)(4 * hh + r) * row_bytes + lane_off : RG_OOB;
    const unsigned wf_q_bytes = (unsigned)g.KP * row_bytes;

    // All gathers are BRANCH FREE (range-checked buffer loads, clamped rows): predicated loads would split the code into
    // basic blocks, and hipcc drains every outstanding load (s_waitcnt vmcnt(0)) at block boundaries, serialising the
    // prefetch.
    // XCD-aware: each XCD (own L2) takes one contiguous eighth of the queries -- neighbouring queries gather the same rows
    const int qpw = g.qpw;
    const int qbase = (rg_xcd_block(blockIdx.x, gridDim.x) * GATHER_WAVES + wave) * qpw;
    if (qbase >= nq) return;
    const int hl = lane < H ? lane : H - 1;
    auto load_idx = [&](int q) -> int {
        const int v = g.nbr[(size_t)(q < nq ? q : nq - 1) * H + hl];
        return (q < nq && lane < H) ? v : ns;
    };
    struct Nb { float rx, ry, rz, f; };
    auto load_nb = [&](int q, int idx) -> Nb {
        const bool real = idx < ns;                                  // else: shadow support point at 1e6 (kpconv_blocks.py:309)
        float sx, sy, sz, f = 0.f;
        if (PRE) {
            const rg_u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(xyzf_rs, real ? (unsigned)idx * 16u : RG_OOB, 0, 0);
            sx = __uint_as_float(r.x); sy = __uint_as_float(r.y); sz = __uint_as_float(r.z); f = __uint_as_float(r.w);
        } else {
            const unsigned so = real ? (unsigned)idx * 12u : RG_OOB;
            sx = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(sxyz_rs, so, 0, 0));
            sy = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(sxyz_rs, so + 4u, 0, 0));
            sz = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(sxyz_rs, so + 8u, 0, 0));
        }
        const unsigned qc = (unsigned)(q < nq ? q : nq - 1);
        const float qx = g.q_xyz[3 * qc], qy = g.q_xyz[3 * qc + 1], qz = g.q_xyz[3 * qc + 2];
        Nb n;
        n.rx = (real ? sx : 1e6f) - qx; n.ry = (real ? sy : 1e6f) - qy; n.rz = (real ? sz : 1e6f) - qz; n.f = f;
        return n;
    };
    // Software pipeline over the wave's queries: the index row of query q+2 and the neighbour coordinates of query q+1
    // are requested while query q is in its gather / MFMA phase, so the idx -> xyz -> features dependency chain of one
    // query overlaps the matrix work of the previous one instead of being exposed three memory latencies deep.
    int idx_cur = load_idx(qbase);
    Nb nb_cur = load_nb(qbase, idx_cur);
    int idx_nxt = load_idx(qbase + 1);
    int seg_cur = 0, seg_end = -1;      // cloud of the current query and its end row (x_stats path)
#pragma unroll 1
    for (int qq = 0; qq < qpw; qq++) {
        const int q = qbase + qq;
        if (q >= nq) return;            // wave-uniform
        __builtin_amdgcn_wave_barrier();
        if (lane < HP) {
            const unsigned ro = idx_cur < ns ? (unsigned)idx_cur * row_bytes : RG_OOB;
            nb_s[lane] = make_float4(nb_cur.rx, nb_cur.ry, nb_cur.rz, __uint_as_float(ro));
        }
        __builtin_amdgcn_wave_barrier();
        const float2* st = nullptr;
        if (!PRE && g.x_stats) {
            // q is wave-uniform and the wave's queries are consecutive: the cloud changes at most rarely, and when it does
            // the whole wave finds it in one round trip (a per-lane binary search would be log2(n) DEPENDENT loads here)
            if (q >= seg_end) {
                seg_cur = rg_find_segment_wave(g.q_seg_off, g.n_seg, q);
                seg_end = g.q_seg_off[seg_cur + 1];
            }
            st = g.x_stats + (size_t)seg_cur * Cin;
        }
        const __amdgpu_buffer_rsrc_t wf_rs = rg_rsrc(g.wf + (size_t)q * g.KP * Cin, wf_q_bytes);
        Nb nb_nxt = nb_cur;
        int idx_nn = ns;
        const float f_cur = nb_cur.f;
        // highest real slot of the row -> groups this query needs (lanes >= H hold ns)
        const unsigned long long real = __ballot(idx_cur < ns);
        const int jn = real ? (64 - __builtin_clzll(real) + 3) >> 2 : 0;
        auto body = [&](auto jj) {
            constexpr int JJ = decltype(jj)::value;
            // ---- influences of kernel point k for neighbours h = 4 j + hh   (the A operands)
            // (Measured, round 4: the same arithmetic on the packed-float32 instructions -- neighbour pairs interleaved in LDS, v_pk_add / v_pk_mul /
            //  v_pk_fma, 75 instead of 120 vector instructions per query -- is bit-identical and NOT faster here: level 0 2118 vs 2114 us, level-0
            //  pool 545 vs 520, level 1 594 vs 584; six more registers cost the Cin = 32 form a wave per SIMD.  This kernel is not bound by the
            //  influence arithmetic; the Cin = 1 kernel below, which is nothing else, keeps the packed form.)
            float w[JJ];
            unsigned row[JJ];       // byte offset of the neighbour's feature row; RG_OOB for a shadow neighbour (reads as zeros)
#pragma unroll
            for (int j = 0; j < JJ; j++) {
                const float4 nb = nb_s[4 * j + hh];
                const float dx = nb.x - kx, dy = nb.y - ky, dz = nb.z - kz;
                float d2;
                {
#pragma clang fp contract(off)
                    d2 = (dx * dx + dy * dy) + dz * dz;                                   // kpconv_blocks.py:326-329
                }
                w[j] = fmaxf(1.f - __builtin_amdgcn_sqrtf(d2) * inv_extent, 0.f);         // :368
                row[j] = __float_as_uint(nb.w) + lane_off;
            }
            float rsum[JJ];
#pragma unroll
            for (int j = 0; j < JJ; j++) rsum[j] = 0.f;
            // ---- channel passes of 16 V channels
#pragma unroll 1
            for (int c0 = 0; c0 < Cin; c0 += 16 * V) {
                const unsigned c0b = (unsigned)c0 * 4u;
                vec xv[JJ];
#pragma unroll
                for (int j = 0; j < JJ; j++) xv[j] = rg_buf_load<V>(x_rs, row[j] + c0b);
                if (c0 == 0) {   // prefetch for the next queries, queued behind this query's feature gathers
                    nb_nxt = load_nb(q + 1, idx_nxt);
                    idx_nn = load_idx(q + 2);
                }
                if (!PRE && st) {   // fused lrelu(InstanceNorm(x)) of the preceding UnaryBlock (wave-uniform branch)
                    float2 ms[V];
#pragma unroll
                    for (int v = 0; v < V; v += 2) {
                        const float4 t = *(const float4*)(st + c0 + V * k + v);
                        ms[v] = make_float2(t.x, t.y); ms[v + 1] = make_float2(t.z, t.w);
                    }
#pragma unroll
                    for (int j = 0; j < JJ; j++)
#pragma unroll
                        for (int v = 0; v < V; v++) {
                            const float t = (rg_comp(xv[j], v) - ms[v].x) * ms[v].y;
                            rg_set(xv[j], v, fmaxf(t, t * g.slope));          // LeakyReLU, 0 < slope < 1
                        }
                }
                // A shadow neighbour's row needs no zeroing for WF: its influence w is exactly 0 (it sits 1e6 away).  Its row
                // sum is discarded below.
                if (!PRE)
#pragma unroll
                for (int j = 0; j < JJ; j++) {   // partial row sums for the normaliser (:409)
                    float s = rg_comp(xv[j], 0);
#pragma unroll
                    for (int v = 1; v < V; v++) s += rg_comp(xv[j], v);
                    rsum[j] += s;
                }
                floatx4 acc[V];
#pragma unroll
                for (int v = 0; v < V; v++) acc[v] = floatx4{0.f, 0.f, 0.f, 0.f};
                // (the J dependent MFMAs of a channel slice as two independent accumulator chains, round 5: level-0 convolution 2170 us against
                //  2136-2142 us, issue-stall share 67.0 % against 66.0 % -- the chain is not what the stalls wait for; profiles/r05_gather_chains.md)
#pragma unroll
                for (int j = 0; j < JJ; j++)
#pragma unroll
                    for (int v = 0; v < V; v++)
                        acc[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j], rg_comp(xv[j], v), acc[v], 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    vec o;
#pragma unroll
                    for (int v = 0; v < V; v++) rg_set(o, v, acc[v][r]);
                    rg_buf_store(wf_rs, st_off[r] + c0b, o);
                }
            }
            // ---- normaliser: positive-row count over the query's real neighbours   (:409-411)
            float cnt = 0.f;
            if (PRE) {   // lanes = neighbours here (a lane beyond H or on a shadow neighbour loaded 0)
                cnt = (float)__builtin_popcountll(__ballot(f_cur > 0.f));
            } else {
#pragma unroll
                for (int j = 0; j < JJ; j++) cnt += (rg_row16_sum(rsum[j]) > 0.f && row[j] < RG_OOB) ? 1.f : 0.f;
                cnt += __shfl_xor(cnt, 16, RG_WAVE);
                cnt += __shfl_xor(cnt, 32, RG_WAVE);
            }
            if (lane == 0) g.num[q] = fmaxf(cnt, 1.f);
        };
        constexpr int JMIN = J - (rg_mg_bodies<J, V, PRE>() - 1) * RG_MG_GROUP_STEP;
        rg_for_group_count<J, (JMIN < 1 ? 1 : JMIN)>(jn, body);
        idx_cur = idx_nxt; nb_cur = nb_nxt; idx_nxt = idx_nn;
    }
}

// (Rounds 3-4 built this gather on the 16-bit matrix pipe as well -- feature rows as f16 pair planes, staged row-wise in LDS and read
//  back with ds_read_b64_tr_b16 as v_mfma_f32_16x16x32_f16 operands; round 4 software-pipelined the row loads, swapped the operand roles
//  for 16-byte stores and cut the contraction to 48 slots.  Correct to 4e-7, a third of the ALU cycles, and still 12-20 % slower than the
//  kernel above: 40-50 % of a wave's time went into ISSUING the row loads against a full vector-memory pipe -- both kernels ingest the
//  gathered rows at ~15 B per clock and CU from L2 / Infinity Cache, and that is the limiter at Cin >= 64.  Removed after the
//  measurement; numbers and phase clocks in profiles/r04_f16_gather_v2.md, docs/NEGATIVES.md.)


// Wave-uniform maximum of a small non-negative int: four DPP rotate-max steps inside the 16-lane rows, then the four rows through SGPRs.
__device__ __forceinline__ int rg_wave_max_uniform(int v)
{
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false));   // row_ror:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false));   // row_ror:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false));   // row_ror:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false));   // row_ror:1
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// Cin == 1 (first encoder block, features = ones): no channel dimension to spread over lanes, so lanes are
// (query, kernel point) pairs: 4 queries x 16 kernel points per wave, each lane walks its query's neighbours once and
// accumulates influence x feature directly -- no influence tile in LDS, 5 floats of LDS per neighbour instead of 22.
// The kernel is pure vector ALU (600 influences per query), so the neighbours are walked TWO at a time on the packed-float32
// instructions (v_pk_add / v_pk_mul / v_pk_fma: the same IEEE operations, two per instruction): the LDS image holds neighbour PAIRS
// (rows padded to an even length), one 8-byte read per quantity and pair.
__global__ void __launch_bounds__(GATHER_WAVES * RG_WAVE) k_kpconv_gather_c1(GatherArgs g)
{
    constexpr int QW = 4;
    extern __shared__ __align__(16) float smem[];
    const int wave = threadIdx.x >> 6, lane = rg_lane();
    const int H = g.H, HP = (H + 1) & ~1, NPAIR = HP >> 1;
    // per (query, neighbour pair): relx[2] | rely[2] | relz[2] | x[2] | flag[2] -- 40 bytes, so the walk below needs ONE address register
    float* pair_s = smem + (size_t)wave * QW * NPAIR * 10;
    const int q0 = (rg_xcd_block(blockIdx.x, gridDim.x) * GATHER_WAVES + wave) * QW;
    if (q0 >= g.nq) return;
    int used = 0;      // slots up to the lane's highest real neighbour
    for (int e = lane; e < QW * HP; e += RG_WAVE) {
        const int qi = e / HP, h = e - qi * HP, q = q0 + qi;
        float rx = 1e6f, ry = 1e6f, rz = 1e6f, f = 0.f, x1 = 0.f;
        if (q < g.nq && h < H) {
            const int idx = g.nbr[(size_t)q * H + h];
            float sx = 1e6f, sy = 1e6f, sz = 1e6f;
            if (idx < g.ns) {
                used = max(used, h + 1);
                if (g.s_xyzf) {   // (x, y, z, feature) in one 16-byte load
                    const float4 r = *(const float4*)(g.s_xyzf + 4 * (size_t)idx);
                    sx = r.x; sy = r.y; sz = r.z; x1 = r.w; f = x1 > 0.f ? 1.f : 0.f;
                } else {
                    sx = g.s_xyz[3 * (size_t)idx]; sy = g.s_xyz[3 * (size_t)idx + 1]; sz = g.s_xyz[3 * (size_t)idx + 2];
                    x1 = g.x[idx]; f = g.flag ? g.flag[idx] : (x1 > 0.f ? 1.f : 0.f);
                }
            }
            rx = sx - g.q_xyz[3 * (size_t)q]; ry = sy - g.q_xyz[3 * (size_t)q + 1]; rz = sz - g.q_xyz[3 * (size_t)q + 2];
        }
        float* d = pair_s + (qi * NPAIR + (h >> 1)) * 10 + (h & 1);      // (the pad slot of an odd H: a shadow neighbour, influence 0)
        d[0] = rx; d[2] = ry; d[4] = rz; d[6] = x1; d[8] = f;
    }
    __builtin_amdgcn_wave_barrier();
    // The walk below stops at the last pair that holds a real neighbour of ANY of the wave's four queries (the wave runs to its longest
    // lane anyway): a shadow's influence and feature are +0, fmaf(+0, x, acc) and cnt += 0 are the identity.
    const int npair = (rg_wave_max_uniform(used) + 1) >> 1;
    const int qi = lane >> 4, k = lane & 15, q = q0 + qi;
    if (q >= g.nq) return;
    const bool kvalid = k < g.KP;
    const float kx = kvalid ? g.kp[3 * k] : 0.f, ky = kvalid ? g.kp[3 * k + 1] : 0.f, kz = kvalid ? g.kp[3 * k + 2] : 0.f;
    const float inv_extent = 1.0f / g.extent;
    const rg_f32x2 ninv{-inv_extent, -inv_extent}, one{1.f, 1.f};
    float acc = 0.f, cnt = 0.f;
    const float* pp = pair_s + qi * NPAIR * 10;
    for (int p = 0; p < npair; p++, pp += 10) {
        const rg_f32x2 dx = *(const rg_f32x2*)(pp) - kx, dy = *(const rg_f32x2*)(pp + 2) - ky, dz = *(const rg_f32x2*)(pp + 4) - kz;
        const rg_f32x2 xv = *(const rg_f32x2*)(pp + 6), fv = *(const rg_f32x2*)(pp + 8);
        rg_f32x2 d2;
        {
#pragma clang fp contract(off)
            d2 = (dx * dx + dy * dy) + dz * dz;                                            // kpconv_blocks.py:326-329
        }
        const rg_f32x2 sq{__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)};
        const rg_f32x2 t = __builtin_elementwise_fma(sq, ninv, one);                        // 1 - d / extent (:368)
        acc = fmaf(fmaxf(t.x, 0.f), xv.x, acc);                                            // (neighbour order kept)
        acc = fmaf(fmaxf(t.y, 0.f), xv.y, acc);
        cnt += fv.x + fv.y;                                                                // (0 / 1 flags: exact in any order)
    }
    if (k < g.ld_wf) g.wf[(size_t)q * g.ld_wf + k] = kvalid ? acc : 0.f;      // ld_wf = KP, or 16 with a zero pad column
    if (k == 0) g.num[q] = fmaxf(cnt, 1.f);
}

// The same, software-pipelined over several 4-query groups per wave (packed support records only): the kernel above spends most of a wave's
// life in the idx -> record dependency chain of its single group (two memory round trips before the first influence).  Measured at level 0
// of a 64-pair forward (2.4 M queries, tools/gather_bench.py --levels 7, same box): scalar influences 772 / 760 us, packed pairs 720 / 732,
// + this pipeline 676 / 681 -- bit-identical outputs; ~570 us is the vector-ALU time of the loop (two quarter-rate v_sqrt_f32 per pair).  Here group g + 1's records and group g + 2's index rows are in flight
// while group g's influences are computed from LDS (two LDS images, ping-pong).  NS = element slots per lane: 4 HP <= 64 NS.
template <int NS>
__global__ void __launch_bounds__(GATHER_WAVES * RG_WAVE) k_kpconv_gather_c1p(GatherArgs g)
{
    constexpr int QW = 4;
    extern __shared__ __align__(16) float smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = rg_lane();
    const int H = g.H, HP = (H + 1) & ~1, NPAIR = HP >> 1, nq = g.nq, ns = g.ns;
    float* buf_s = smem + (size_t)wave * 2 * QW * NPAIR * 10;            // [2][QW][NPAIR][10] (layout of k_kpconv_gather_c1)
    const int groups = g.qpw;                                            // 4-query groups per wave
    const int qbase = (rg_xcd_block(blockIdx.x, gridDim.x) * GATHER_WAVES + wave) * QW * groups;
    if (qbase >= nq) return;
    // element slots of this lane: e = lane + 64 s -> (query e / HP of the group, neighbour column e % HP)
    int e_q[NS], e_h[NS], e_dst[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int e = lane + RG_WAVE * s;
        e_q[s] = e / HP; e_h[s] = e - e_q[s] * HP;
        if (e >= QW * HP) { e_q[s] = -1; e_h[s] = 0; }
        e_dst[s] = (e_q[s] * NPAIR + (e_h[s] >> 1)) * 10 + (e_h[s] & 1);
    }
    // branch-free loads from clamped addresses (a predicated load drains every outstanding one: tools/isa_scan.py)
    auto issue_idx = [&](int qg, int (&idx)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int q = qg + (e_q[s] < 0 ? 0 : e_q[s]);
            const int v = g.nbr[(size_t)(q < nq ? q : nq - 1) * H + (e_h[s] < H ? e_h[s] : H - 1)];
            idx[s] = (e_q[s] >= 0 && q < nq && e_h[s] < H) ? v : -1;     // -1: not an element (pad slot, query beyond the end)
        }
    };
    struct Rec { float4 r; float qx, qy, qz; };
    auto issue_rec = [&](int qg, const int (&idx)[NS], Rec (&rec)[NS]) {
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int q = qg + (e_q[s] < 0 ? 0 : e_q[s]);
            const unsigned qc = (unsigned)(q < nq ? q : nq - 1);
            const int ic = idx[s] < 0 ? 0 : (idx[s] < ns ? idx[s] : ns - 1);
            rec[s].r = *(const float4*)(g.s_xyzf + 4 * (size_t)ic);
            rec[s].qx = g.q_xyz[3 * qc]; rec[s].qy = g.q_xyz[3 * qc + 1]; rec[s].qz = g.q_xyz[3 * qc + 2];
        }
    };
    // -> pairs of the group up to the last one that holds a real neighbour of any of its four queries (k_kpconv_gather_c1)
    auto stage = [&](float* buf, const int (&idx)[NS], const Rec (&rec)[NS]) -> int {
        int used = 0;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            if (e_q[s] < 0) continue;
            const bool elem = idx[s] >= 0, real = elem && idx[s] < ns;
            used = real ? max(used, e_h[s] + 1) : used;
            // (as k_kpconv_gather_c1: a shadow neighbour sits at 1e6 - q, a pad slot at 1e6; both have influence 0 and feature 0)
            const float sx = real ? rec[s].r.x : 1e6f, sy = real ? rec[s].r.y : 1e6f, sz = real ? rec[s].r.z : 1e6f;
            const float x1 = real ? rec[s].r.w : 0.f;
            float* d = buf + e_dst[s];
            d[0] = elem ? sx - rec[s].qx : 1e6f; d[2] = elem ? sy - rec[s].qy : 1e6f; d[4] = elem ? sz - rec[s].qz : 1e6f;
            d[6] = x1; d[8] = x1 > 0.f ? 1.f : 0.f;
        }
        return (rg_wave_max_uniform(used) + 1) >> 1;
    };
    const int qi = lane >> 4, k = lane & 15;
    const bool kvalid = k < g.KP;
    const float kx = kvalid ? g.kp[3 * k] : 0.f, ky = kvalid ? g.kp[3 * k + 1] : 0.f, kz = kvalid ? g.kp[3 * k + 2] : 0.f;
    const float inv_extent = 1.0f / g.extent;
    const rg_f32x2 ninv{-inv_extent, -inv_extent}, one{1.f, 1.f};

    int idx_a[NS], idx_b[NS];
    Rec rec[NS];
    issue_idx(qbase, idx_a);
    issue_rec(qbase, idx_a, rec);
    issue_idx(qbase + QW, idx_b);
    int npair = stage(buf_s, idx_a, rec);
#pragma unroll 1
    for (int gi = 0; gi < groups; gi++) {
        const int qg = qbase + gi * QW;
        if (qg >= nq) return;                                            // wave-uniform
        int idx_c[NS];
        issue_rec(qg + QW, idx_b, rec);                                  // group gi + 1's records (its index row arrived a group ago)
        issue_idx(qg + 2 * QW, idx_c);
        __builtin_amdgcn_wave_barrier();
        const int q = qg + qi;
        const float* pp = buf_s + (gi & 1) * QW * NPAIR * 10 + qi * NPAIR * 10;
        float acc = 0.f, cnt = 0.f;
        for (int p = 0; p < npair; p++, pp += 10) {
            const rg_f32x2 dx = *(const rg_f32x2*)(pp) - kx, dy = *(const rg_f32x2*)(pp + 2) - ky, dz = *(const rg_f32x2*)(pp + 4) - kz;
            const rg_f32x2 xv = *(const rg_f32x2*)(pp + 6), fv = *(const rg_f32x2*)(pp + 8);
            rg_f32x2 d2;
            {
#pragma clang fp contract(off)
                d2 = (dx * dx + dy * dy) + dz * dz;                                        // kpconv_blocks.py:326-329
            }
            const rg_f32x2 sq{__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)};
            const rg_f32x2 t = __builtin_elementwise_fma(sq, ninv, one);                    // 1 - d / extent (:368)
            acc = fmaf(fmaxf(t.x, 0.f), xv.x, acc);
            acc = fmaf(fmaxf(t.y, 0.f), xv.y, acc);
            cnt += fv.x + fv.y;
        }
        if (q < nq) {
            if (k < g.ld_wf) g.wf[(size_t)q * g.ld_wf + k] = kvalid ? acc : 0.f;
            if (k == 0) g.num[q] = fmaxf(cnt, 1.f);
        }
        __builtin_amdgcn_wave_barrier();
        npair = stage(buf_s + ((gi + 1) & 1) * QW * NPAIR * 10, idx_b, rec);
#pragma unroll
        for (int s = 0; s < NS; s++) idx_b[s] = idx_c[s];
    }
}

// out[q, c] = max_h x_pad[nbr[q, h], c]   with a zero shadow row   (kpconv_blocks.py:127-143)
// QW queries per wave: C / 4 lanes (one float4 each) serve a query when C <= 128, so that no lane idles on narrow rows
template <int QW>
__global__ void __launch_bounds__(256) k_maxpool_gather(const float* __restrict__ x, int ns, int C, const int* __restrict__ nbr,
                                                        int ld_nbr, int nq, int H, float* __restrict__ out)
{
    constexpr int LQ = RG_WAVE / QW;                 // lanes per query
    const int lane = rg_lane();
    const int q = (rg_xcd_block(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * QW + lane / LQ;      // XCD-contiguous
    if (q >= nq) return;
    const int* row = nbr + (size_t)q * ld_nbr;
    for (int c = (lane % LQ) * 4; c < C; c += LQ * 4) {
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int h0 = 0; h0 < H; h0 += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int idx = h0 + u < H ? row[h0 + u] : -1;
                v[u] = m;                                                    // out-of-range slot: neutral
                if (idx >= 0) v[u] = idx < ns ? *(const float4*)(x + (size_t)idx * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                m.x = fmaxf(m.x, v[u].x); m.y = fmaxf(m.y, v[u].y); m.z = fmaxf(m.z, v[u].z); m.w = fmaxf(m.w, v[u].w);
            }
        }
        *(float4*)(out + (size_t)q * C + c) = m;
    }
}

}  // namespace

// The same, BRANCH FREE.  The .s of the kernel above is a chain of `global_load ; s_waitcnt vmcnt(0)` pairs -- every index load and every
// row load sits in its own predicated block, so the "8 rows in flight" never were: one dependent round trip after the other (index,
// row, index, row ...).  Here the index row is read with clamped column numbers (a repeated neighbour does not change a maximum), the
// feature rows with range-checked buffer loads (an offset of RG_OOB returns zeros: exactly the zero shadow row), HB rows per batch
// all issued before the first maximum.  Needs ns * C * 4 < 2^32 - 256 (32-bit unsigned buffer offsets; MP_OOB, not RG_OOB, is the out-of-range
// offset here: the level-0 rows of a 192-pair forward are 3.7 GB, and with RG_OOB's 2 GiB bound that launch fell back to the predicated kernel
// above -- 2.65 ms against 1.9 for three times the 64-pair launch).
namespace {
constexpr unsigned MP_OOB = 0xfffffff0u;
template <int QW, int HB>
__global__ void __launch_bounds__(256) k_maxpool_gather_buf(const float* __restrict__ x, int ns, int C, const int* __restrict__ nbr,
                                                            int ld_nbr, int nq, int H, float* __restrict__ out)
{
    constexpr int LQ = RG_WAVE / QW;                 // lanes per query
    const int lane = rg_lane();
    const int q = (rg_xcd_block(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6)) * QW + lane / LQ;      // XCD-contiguous
    const int qc = q < nq ? q : nq - 1;              // a dead lane repeats the last query (it never stores)
    const int* row = nbr + (size_t)qc * ld_nbr;
    const unsigned row_bytes = (unsigned)C * 4u;
    const __amdgpu_buffer_rsrc_t x_rs = rg_rsrc(x, (unsigned)ns * row_bytes);
    for (int c = (lane % LQ) * 4; c < C; c += LQ * 4) {
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        const unsigned cb = (unsigned)c * 4u;
        for (int h0 = 0; h0 < H; h0 += HB) {
            int idx[HB];
#pragma unroll
            for (int u = 0; u < HB; u++) idx[u] = row[min(h0 + u, H - 1)];
            float4 v[HB];
#pragma unroll
            for (int u = 0; u < HB; u++) v[u] = rg_buf_load<4>(x_rs, (unsigned)idx[u] < (unsigned)ns ? (unsigned)idx[u] * row_bytes + cb : MP_OOB);
#pragma unroll
            for (int u = 0; u < HB; u++) {
                m.x = fmaxf(m.x, v[u].x); m.y = fmaxf(m.y, v[u].y); m.z = fmaxf(m.z, v[u].z); m.w = fmaxf(m.w, v[u].w);
            }
        }
        if (q < nq) *(float4*)(out + (size_t)q * C + c) = m;
    }
}
}  // namespace

extern "C" {

int regtr_rowsum_positive(const float* x, int n, int C, const float* stats, const int* seg_off, int n_seg, float slope,
                          float* flag, void* stream)
{
    if (!x || !flag || n < 0 || C < 1 || (stats && (!seg_off || n_seg < 1))) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    k_rowsum_positive<<<rg_cdiv(n, 4), 256, 0, (hipStream_t)stream>>>(x, n, C, (const float2*)stats, seg_off, n_seg, slope,
                                                                       flag);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

// 1 when regtr_kpconv_gather derives the positivity flags from the rows it gathers (flag may then be NULL)
int regtr_kpconv_gather_computes_flag(int Cin, int H) { return (Cin == 1 || (Cin % 32 == 0 && H <= 64)) ? 1 : 0; }

// wf [nq, KP*Cin] (k-major, channel-minor: matches weights.view(KP*Cin, Cout)), num [nq].
int regtr_kpconv_gather(const float* q_xyz, int nq, const float* s_xyz, int ns, const int* nbr, int H, const float* x,
                        int Cin, const float* flag, const float* s_xyzf, const float* kernel_points, int KP, float extent,
                        const float* x_stats, const int* q_seg_off, int n_seg, float slope, float* wf, int ld_wf, float* num,
                        void* stream)
{
    if (ld_wf == 0) ld_wf = KP * Cin;
    if (ld_wf != KP * Cin && !(Cin == 1 && ld_wf == KP_PAD)) return RG_ERR_ARG;
    if (!q_xyz || !s_xyz || !nbr || !x || !kernel_points || !wf || !num || nq < 0 || ns < 0 || H < 1 ||
        Cin < 1 || KP < 1 || KP > KP_PAD || !(extent > 0.f) || (x_stats && (!q_seg_off || n_seg < 1)) ||
        (s_xyzf && (x_stats || (uintptr_t)s_xyzf % 16 || (long long)ns * 16 >= (1LL << 31))))
        return RG_ERR_ARG;
    if (!flag && !regtr_kpconv_gather_computes_flag(Cin, H)) return RG_ERR_ARG;
    if (nq == 0) return RG_OK;
    GatherArgs g{q_xyz, s_xyz, nbr, x, flag, s_xyzf, kernel_points, wf, num, (const float2*)x_stats, q_seg_off,
                 nq, ns, H, Cin, KP, n_seg, ld_wf, extent, slope, MG_QPW};
    hipStream_t st = (hipStream_t)stream;
    if (Cin == 1) {
        if (x_stats) return RG_ERR_ARG;
        const int HP1 = (H + 1) & ~1;
        if (s_xyzf && 4 * HP1 <= 4 * RG_WAVE && nq > 0 && ns > 0) {
            // groups of 4 queries per wave: up to 8 where the level is large enough to keep ~8 workgroups per CU anyway
            int groups = (int)(((long long)nq + 256LL * 8 * GATHER_WAVES * 4 - 1) / (256LL * 8 * GATHER_WAVES * 4));
            groups = groups < 1 ? 1 : (groups > 8 ? 8 : groups);
          if (groups >= 2) {      // (a pair or two per forward: one group per wave fills the chip better -- 14.3 vs 15.6 us at one pair)
            g.qpw = groups;
            const size_t ldsp = (size_t)GATHER_WAVES * 2 * 4 * HP1 * 5 * sizeof(float);
            const int gridp = rg_xcd_grid(rg_cdiv(nq, GATHER_WAVES * 4 * groups));
            if (4 * HP1 <= 2 * RG_WAVE) k_kpconv_gather_c1p<2><<<gridp, GATHER_WAVES * RG_WAVE, ldsp, st>>>(g);
            else if (4 * HP1 <= 3 * RG_WAVE) k_kpconv_gather_c1p<3><<<gridp, GATHER_WAVES * RG_WAVE, ldsp, st>>>(g);
            else k_kpconv_gather_c1p<4><<<gridp, GATHER_WAVES * RG_WAVE, ldsp, st>>>(g);
            RG_RETURN_IF_LAUNCH_FAILED();
            return RG_OK;
          }
        }
        const size_t lds1 = (size_t)GATHER_WAVES * 4 * HP1 * 5 * sizeof(float);
        k_kpconv_gather_c1<<<rg_xcd_grid(rg_cdiv(nq, GATHER_WAVES * 4)), GATHER_WAVES * RG_WAVE, lds1, st>>>(g);
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    }
    const bool aligned16 = (((uintptr_t)x | (uintptr_t)wf | (uintptr_t)x_stats) & 15) == 0;
    if (!flag && !(aligned16 && ns > 0 && (long long)ns * Cin < (1LL << 29))) return RG_ERR_ARG;
    if (regtr_kpconv_gather_computes_flag(Cin, H) && aligned16 && ns > 0 && (long long)ns * Cin < (1LL << 29)) {   // matrix-core path
        // queries per wave: MG_QPW (8) on large levels (the software pipeline over a wave's queries hides the idx -> xyz -> rows chain);
        // a small level (one pair: ~5000 queries at level 1) would be ~150 workgroups of 32 serial-ish queries on 256 CUs, so it gets
        // as few per wave as still puts ~12 waves on every CU
        int qpw = (int)(((long long)nq + 256 * 12 - 1) / (256 * 12));
        qpw = qpw < 1 ? 1 : (qpw > MG_QPW ? MG_QPW : qpw);
        g.qpw = qpw;
        const int grid_m = rg_xcd_grid(rg_cdiv(nq, GATHER_WAVES * qpw));
        const int J = H <= 40 ? 10 : (H <= 52 ? 13 : 16);
        const bool v4 = Cin % 64 == 0;
        const bool pre = s_xyzf != nullptr;
#define RG_LAUNCH_MG2(JJ, VV) do { if (pre) k_kpconv_gather_mfma<JJ, VV, true><<<grid_m, GATHER_WAVES * RG_WAVE, 0, st>>>(g); \
                                   else k_kpconv_gather_mfma<JJ, VV, false><<<grid_m, GATHER_WAVES * RG_WAVE, 0, st>>>(g); } while (0)
#define RG_LAUNCH_MG(JJ) do { if (v4) RG_LAUNCH_MG2(JJ, 4); else RG_LAUNCH_MG2(JJ, 2); } while (0)
        if (J == 10) RG_LAUNCH_MG(10); else if (J == 13) RG_LAUNCH_MG(13); else RG_LAUNCH_MG(16);
#undef RG_LAUNCH_MG
#undef RG_LAUNCH_MG2
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    }
    const int LQ = Cin <= 16 ? 16 : (Cin <= 32 ? 32 : 64);
    const int QW = RG_WAVE / LQ;
    const size_t lds = (size_t)GATHER_WAVES * ((QW * H * (KP_PAD + 6) + 3) & ~3) * sizeof(float);
    if (lds > 160 * 1024) return RG_ERR_ARG;
    const int grid = rg_xcd_grid(rg_cdiv(nq, GATHER_WAVES * QW));
    if (LQ == 16) k_kpconv_gather<16><<<grid, GATHER_WAVES * RG_WAVE, lds, st>>>(g);
    else if (LQ == 32) k_kpconv_gather<32><<<grid, GATHER_WAVES * RG_WAVE, lds, st>>>(g);
    else k_kpconv_gather<64><<<grid, GATHER_WAVES * RG_WAVE, lds, st>>>(g);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}


int regtr_maxpool_gather(const float* x, int ns, int C, const int* nbr, int ld_nbr, int nq, int H, float* out, void* stream)
{
    if (!x || !nbr || !out || ns < 0 || nq < 0 || H < 1 || ld_nbr < H || C < 4 || C % 4) return RG_ERR_ARG;
    if (nq == 0) return RG_OK;
    if (ns > 0 && (unsigned long long)ns * C * 4ull < 0xffffff00ull && ((uintptr_t)x % 16) == 0) {      // the branch-free form (32-bit buffer offsets)
        if (C <= 64) k_maxpool_gather_buf<4, 8><<<rg_xcd_grid(rg_cdiv(nq, 16)), 256, 0, (hipStream_t)stream>>>(x, ns, C, nbr, ld_nbr, nq, H, out);
        else if (C <= 128) k_maxpool_gather_buf<2, 8><<<rg_xcd_grid(rg_cdiv(nq, 8)), 256, 0, (hipStream_t)stream>>>(x, ns, C, nbr, ld_nbr, nq, H, out);
        else k_maxpool_gather_buf<1, 8><<<rg_xcd_grid(rg_cdiv(nq, 4)), 256, 0, (hipStream_t)stream>>>(x, ns, C, nbr, ld_nbr, nq, H, out);
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    }
    if (C <= 64) k_maxpool_gather<4><<<rg_xcd_grid(rg_cdiv(nq, 16)), 256, 0, (hipStream_t)stream>>>(x, ns, C, nbr, ld_nbr, nq, H, out);
    else if (C <= 128) k_maxpool_gather<2><<<rg_xcd_grid(rg_cdiv(nq, 8)), 256, 0, (hipStream_t)stream>>>(x, ns, C, nbr, ld_nbr, nq, H, out);
    else k_maxpool_gather<1><<<rg_xcd_grid(rg_cdiv(nq, 4)), 256, 0, (hipStream_t)stream>>>(x, ns, C, nbr, ld_nbr, nq, H, out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
