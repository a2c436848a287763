// One-shot strip GEMM for the SHALLOW encoder levels: C[M, N] = epilogue(A'[M, K] W[K, N]) with K in {32, 64, 128} input
// columns, N <= 512 outputs and millions of rows -- the UnaryBlock / shortcut Linears of the KPConv levels with >= 131072 rows
// (/root/reference/src/models/backbone_kpconv/kpconv_blocks.py:556-561, 722-741).  Float32-grade on the bf16 matrix cores by the
// same exact three-way split as gemm_x3.hip (six v_mfma_f32_32x32x16_bf16 per product block, smallest terms first).
//
// These launches are HBM streams (a few flops per byte).  The tiled kernel of gemm_x3.hip stages A through LDS behind two
// barriers per k-tile: its eight waves move in lockstep phases, so a CU holds two independent streams, and the short-K launches
// run at 2.5-2.8 TB/s; a read+write probe with the same access patterns and occupancy reaches 5.3 TB/s (tools/probe).  Here
//   * every WAVE owns one strip of 32 rows and goes load -> split -> MFMA -> store -> exit on its own: activations travel from
//     global memory straight into MFMA fragments (the A operand of the 32x32x16 MFMA is 8 consecutive k of one row per lane =
//     two float4 loads), the InstanceNorm+LeakyReLU fold of the producer (a_stats) and the bf16 split happen in registers;
//   * nothing is loaded after a store (on CDNA one counter tracks loads AND stores in issue order: a persistent variant that
//     prefetched its next rows waited on its own store acknowledgements and ran at 2.1 TB/s);
//   * the weight planes (K NB 6 bytes <= 48 KB) are copied into LDS once per 8-wave workgroup (256 rows) while the A loads fly:
//     the only barrier;
//   * the clouds of a 256-row tile come from the per-level table of regtr_tile_segments (one 16-byte load, no search);
//   * InstanceNorm statistics of the result: per-lane float64 sums over the wave's rows, cross-wave reduction in LDS, one partial
//     per (256-row tile, cloud) -- the slot convention of regtr_instnorm_finalize_tiles with tile_rows = 256.
// Outputs of two or more column blocks (N / sg_cols_per_wg >= 2) have a second launch form, k_gemm_strip_cols below: one workgroup per row
// tile walks all column blocks, so the rows are loaded, folded and split once per tile (sg_walks_columns: the shapes that take it).
// Measured on MI355X, 2.4 M rows (tools/stream_bench.py), strip vs tiled kernel, both writing C and the statistics partials:
//   64 -> 128: 522 vs 660 us   32 -> 128 (folded A): 395 vs 580   64 -> 32: 184 vs 338 (5.1 TB/s)   128 -> 32: 283 vs 499 (5.5 TB/s)
//   0.6 M rows: 64 -> 256: 284 vs 381   128 -> 64: 151 vs 150.
// (Also built and dropped: the resnet-block tail as an epilogue -- statistics-only pass, then normalise + shortcut + LeakyReLU from
//  the accumulators.  Both passes pay the split + MFMA work again (~350 us at level 0) and the residual tile next to four live
//  accumulators spills: 0.33 + 1.75 ms against 0.41 + 0.71 ms for this kernel followed by k_instnorm_apply.)
#include "common.h"
#include "mfma_operands.h"

namespace {

constexpr int SG_WAVES = 8;
constexpr int SG_ROWS = 32 * SG_WAVES;       // rows per workgroup = statistics tile

struct SgArgs {
    const float* A; const uint16_t* Wt; float* C;
    const float2* a_stats;
    const int* seg_off;          // cloud offsets of the rows (of A and C alike), n_seg + 1
    const int4* tile_info;       // regtr_tile_segments(seg_off, n_seg, M, 256): (first cloud, last cloud, first's begin, first's end)
    double2* stat_partial;       // optional [(ceil(M / 256) + n_seg) * N]
    size_t plane;                // elements per weight plane (Npad * Kp)
    int M, N, Kp, lda, ldc, n_seg;
    float a_slope;
};

// LDS image of the weights: plane p, column n = one row of K bf16 (CPR = K / 8 sixteen-byte chunks); chunk c of row n sits at
// c ^ swz(n), swz chosen so that the 16 lanes a ds_read_b128 services together (rows {0-3,12-15,20-27} / {4-11,16-19,28-31})
// touch all 64 banks once: CPR 4 -> (n >> 2) & 3, CPR 8 -> (n >> 1) & 7, CPR 16 -> n & 15.
template <int KT> __device__ __forceinline__ unsigned sg_swz(unsigned n)
{
    constexpr int CPR = 2 * KT;
    return CPR == 4 ? ((n >> 2) & 3u) : (CPR == 8 ? ((n >> 1) & 7u) : (n & 15u));
}

// KT = K / 16 (2, 4, 8); NT = 32-column blocks per workgroup column (1, 2, 4); INFOLD: A' = LeakyReLU(InstanceNorm(A))
template <int KT, int NT, bool INFOLD>
__global__ void __launch_bounds__(SG_WAVES* RG_WAVE, (KT <= 4 || NT <= 2) ? 4 : 2) k_gemm_strip(SgArgs g)
{
    constexpr int K = 16 * KT, CPR = 2 * KT, ROWB = K * 2, NB = 32 * NT;
    extern __shared__ __align__(16) unsigned char Ws[];          // [3][NB][K] bf16, chunk-swizzled | double2 red[SG_WAVES][NB]
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // Workgroup -> (row tile, column block), round 6: a 1-D launch in which the column blocks of ONE 256-row tile are consecutive workgroups of
    // ONE XCD (workgroup id -> XCD id % 8): the tile's A rows are fetched from HBM once and served to the other column blocks by that XCD's L2.
    // (Until round 5 the launch was (row tiles, column blocks) with the row tiles fastest: every column block re-read A from HBM a whole pass
    //  later, which kept wide outputs off this kernel -- N <= 256 and at most two column blocks.)
    const int ncol = g.N / NB;
    const int wg_k = (int)(blockIdx.x >> 3), row_tile = (wg_k / ncol) * 8 + (int)(blockIdx.x & 7u);
    if (row_tile * SG_ROWS >= g.M) return;                        // (the whole workgroup, before any barrier)
    const int N = g.N, n0 = (wg_k % ncol) * NB;
    const int m0 = row_tile * SG_ROWS, r0 = m0 + 32 * wave;       // the wave's strip
    const int row = r0 + l31;
    const bool row_ok = row < g.M;
#ifdef SG_PROF
    long long pt[8]; int pi = 0;
#define SG_STAMP() do { pt[pi++] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SG_STAMP() do {} while (0)
#endif
    SG_STAMP();

    // ---- the strip's rows first (the long-latency loads), the tile's clouds, then the weights while those fly
    float4 raw[KT][2];
    {
        const float* ap = g.A + (size_t)(row_ok ? row : g.M - 1) * g.lda + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < KT; ks++) {
            raw[ks][0] = *(const float4*)(ap + 16 * ks);
            raw[ks][1] = *(const float4*)(ap + 16 * ks + 4);
        }
    }
    const int4 ti = g.tile_info[row_tile];
    {
        // the weight planes by LDS-DMA (global_load_lds_dwordx4: 64 sixteen-byte pieces per instruction, no staging registers, every
        // instruction of the workgroup in flight at once behind the A loads).  A DMA fills LDS lane-linearly, so lane i of DMA q is slot
        // s = 64 q + i = (p NB + n) CPR + cs of the image and fetches logical chunk cs ^ swz(n) of column n, plane p.
        // (As a load -> ds_write loop the copy was six dependent round trips per thread -- hipcc keeps the loop rolled, one
        //  s_waitcnt vmcnt(0) per piece: 11-40 k of a wave's ~50 k cycles, profiles/r04_strip_phase_clocks.md.)
        constexpr int NDMA = 3 * NB * CPR / RG_WAVE;
        static_assert(3 * NB * CPR % RG_WAVE == 0, "whole DMA instructions");
#pragma unroll
        for (int q0 = 0; q0 < NDMA; q0 += SG_WAVES) {
            const int q = q0 + wave;
            if (q < NDMA) {                                          // wave-uniform
                const int sidx = q * RG_WAVE + lane;
                const int p = sidx / (NB * CPR), rem = sidx - p * (NB * CPR), n = rem / CPR, cs = rem - n * CPR;
                const uint16_t* src = g.Wt + (size_t)p * g.plane + (size_t)(n0 + n) * g.Kp + (((unsigned)cs ^ sg_swz<KT>((unsigned)n)) * 8);
                __builtin_amdgcn_global_load_lds((const void*)src, (rg_lds_ptr)(Ws + (size_t)q * 1024), 16, 0, 0);
            }
        }
    }
    const int s_lo = ti.x, s_hi = ti.y;
    const bool one_cloud = s_lo == s_hi;                          // workgroup-uniform; almost always
    SG_STAMP();
    __syncthreads();                                              // (carries the vmcnt(0) that lands the DMA)
    SG_STAMP();

    // ---- A fragments: fold, split
    bf16x8 fa[KT][3];
    {
        const float2* sp = nullptr;
        if (INFOLD) {
            const int my_seg = one_cloud ? s_lo : rg_find_segment(g.seg_off, g.n_seg, row_ok ? row : g.M - 1);
            sp = g.a_stats + (size_t)my_seg * K + 8 * hi;
        }
#pragma unroll
        for (int ks = 0; ks < KT; ks++) {
            float x[8] = {raw[ks][0].x, raw[ks][0].y, raw[ks][0].z, raw[ks][0].w, raw[ks][1].x, raw[ks][1].y, raw[ks][1].z, raw[ks][1].w};
            if (INFOLD) {
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const float4 s4 = *(const float4*)(sp + 16 * ks + e);
                    float u = (x[e] - s4.x) * s4.y;
                    x[e] = fmaxf(u, u * g.a_slope);
                    u = (x[e + 1] - s4.z) * s4.w;
                    x[e + 1] = fmaxf(u, u * g.a_slope);
                }
            }
            unsigned w[4][3];
#pragma unroll
            for (int e = 0; e < 4; e++) rg_split2(row_ok ? x[2 * e] : 0.f, row_ok ? x[2 * e + 1] : 0.f, w[e]);
#pragma unroll
            for (int p = 0; p < 3; p++) fa[ks][p] = __builtin_bit_cast(bf16x8, make_uint4(w[0][p], w[1][p], w[2][p], w[3][p]));
        }
    }
    SG_STAMP();
    unsigned f_off[KT];
#pragma unroll
    for (int ks = 0; ks < KT; ks++) f_off[ks] = (unsigned)l31 * ROWB + (((unsigned)(2 * ks + hi)) ^ sg_swz<KT>((unsigned)l31)) * 16u;

    // ---- all MFMAs of the strip (NT independent accumulators)
    floatx16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[j][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KT; ks++)
#pragma unroll
        for (int j = 0; j < NT; j++) {
            bf16x8 fb[3];
#pragma unroll
            for (int p = 0; p < 3; p++)
                fb[p] = __builtin_bit_cast(bf16x8, *(const uint4*)(Ws + (size_t)(p * NB + 32 * j) * ROWB + f_off[ks]));
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][2], fb[0], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1], fb[1], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], fb[2], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1], fb[0], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], fb[1], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], fb[0], acc[j], 0, 0, 0);
        }

    const int rbase = r0 + 4 * hi;
#ifdef SG_PROF
    { float z = 0.f; for (int j = 0; j < NT; j++) z += acc[j][0]; if (z == 1.2345e30f) pt[0] = 0; }   // (the accumulators are complete)
#endif
    SG_STAMP();
    // ---- statistics of the Linear's own output: per cloud of the tile, per column (kpconv_blocks.py:510-519) -- BEFORE the stores: the
    // transposing store below consumes the accumulators in place
    if (g.stat_partial) {                                        // workgroup-uniform
    double2* red = (double2*)(Ws + (size_t)3 * NB * ROWB);        // [SG_WAVES][NB]
    for (int sg = s_lo; sg <= s_hi; sg++) {                      // workgroup-uniform; one pass almost always
        const int c_lo = sg == s_lo ? ti.z : g.seg_off[sg], c_hi = min(sg == s_lo ? ti.w : g.seg_off[sg + 1], g.M);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int rw = rbase + (r & 3) + 8 * (r >> 2);
                if (rw >= c_lo && rw < c_hi) { const double v = (double)acc[j][r]; s += v; q += v * v; }
            }
            s += __shfl_xor(s, 32, RG_WAVE); q += __shfl_xor(q, 32, RG_WAVE);
            if (hi == 0) red[wave * NB + 32 * j + l31] = make_double2(s, q);
        }
        __syncthreads();
        if (t < NB) {
            double2 a = red[t];
#pragma unroll
            for (int w = 1; w < SG_WAVES; w++) { const double2 b = red[w * NB + t]; a.x += b.x; a.y += b.y; }
            g.stat_partial[(size_t)(row_tile + sg) * N + n0 + t] = a;
        }
        if (sg < s_hi) __syncthreads();                          // red is reused by the next cloud
    }
    }
    SG_STAMP();
    // ---- store: a lane holds a COLUMN strip (rows 4 hi + (r & 3) + 8 (r >> 2) of column l31), every instruction writes two full 128-byte lines.
    // (Measured, round 4: the 4 x 4 blocks of a lane quad transposed by DPP quad_perm butterflies so that a lane owns four consecutive columns of
    //  one row -- 4 NT sixteen-byte stores per lane instead of 16 NT dwords, eight full lines per instruction: bit-identical and NOT faster,
    //  313 vs 287 us on the 0.6 M x 64 -> 256 shape; the wave's time in its store phase is queueing in the memory system, not instruction issue:
    //  profiles/r04_strip_phase_clocks.md.)
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int rw = rbase + (r & 3) + 8 * (r >> 2);
            if (rw < g.M) g.C[(size_t)rw * g.ldc + n0 + 32 * j + l31] = acc[j][r];
        }
#ifdef SG_PROF
    SG_STAMP();
    __builtin_amdgcn_s_waitcnt(0);
    SG_STAMP();
    if (lane == 0 && (row_tile == 700 || row_tile == 1500) && n0 == 0 && (wave == 0 || wave == 5))
        printf("gemm_strip KT %d NT %d row tile %d wave %d: loads+Wcopy %lld barrier %lld split %lld mfma %lld stats %lld store-issue %lld drain %lld total %lld\n", KT, NT, row_tile, wave,
               pt[1] - pt[0], pt[2] - pt[1], pt[3] - pt[2], pt[4] - pt[3], pt[5] - pt[4], pt[6] - pt[5], pt[7] - pt[6], pt[7] - pt[0]);
#endif
}

// ---- The COLUMN-WALKING form of the same product for wide outputs (two or more column blocks of the one-shot form).
// One 8-wave workgroup owns a 256-row tile for ALL of its columns: a wave loads, folds and splits its 32 rows ONCE (the one-shot form pays
// that phase, the tile_info / a_stats loads and a wave start-up and tail once per column block) and then walks the columns in SLOTS of 4096
// weights x 3 planes = 24576 bytes at every K (32 / 64 / 128 columns at K = 128 / 64 / 32), one 32-column accumulator block per pass.
// The slots travel through a two-deep LDS ring by LDS-DMA (the source-address swizzle of k_gemm_strip); two slots, two reduction buffers:
// 57344 bytes and 128 registers, so two workgroups per CU stay resident (the persistent ROW-walking form of round 4 lost by dropping to one).
// Per column and per statistics slot the arithmetic and its order are those of k_gemm_strip: C and stat_partial are bit-identical.
//
// Ordering.  gfx950 retires loads, LDS-DMAs and stores through one in-order counter (vmcnt), so inside the walk
//   * slot s + 1 is issued at the TOP of slot s: behind the stores of slot s - 1, ahead of every store of slot s;
//   * it is waited for in the last pass of slot s, after that pass's stores, by vmcnt(SGC_AFTER): the 16 SP stores the wave has issued since
//     (a wave with rows past M issues fewer store instructions -- hipcc branches around an all-off store -- and waits vmcnt(0));
//   * the barrier that follows the wait (the statistics barrier of that pass, or a barrier of its own without statistics) is the one every
//     wave passes before the first ds_read of slot s + 1 (RAW: wait, barrier, read), and the one after every wave's last ds_read of slot s,
//     behind which slot s + 2 is issued into the same ring entry (WAR);
//   * the barriers inside the walk are raw s_barrier behind lgkmcnt(0) only: __syncthreads() would drain the DMA and the stores (vmcnt(0)).
// The reduction buffer alternates per (pass, cloud): a buffer is rewritten two barriers after wave 0 read it.
constexpr int SGC_SLOT = 3 * 4096 * 2;                 // bytes of a ring slot
constexpr int SGC_RED = SG_WAVES * 32 * 16;            // double2 red[SG_WAVES][32]
constexpr size_t SGC_LDS = 2 * SGC_SLOT + 2 * SGC_RED;

typedef unsigned sgc_u4 __attribute__((ext_vector_type(4)));
#define SGC_VM(N_) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N_) : "memory")
#define SGC_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// One LDS-DMA instruction from asm: 64 sixteen-byte pieces, lane i from sbase + voff (bytes) to LDS byte lds_dst + 16 i.  From asm, so that hipcc's
// wait insertion does not know of an LDS write in flight: it answers one with s_waitcnt vmcnt(0) in front of every later LDS access of the loop
// (the reduction buffer's among them), which drains the stores too.  The walk's own counted waits order the DMA (see above).
__device__ __forceinline__ void sgc_dma16(const void* sbase, unsigned voff, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// The walk's stores from asm as well: wave-uniform base + one 32-bit lane offset (as C++ they are sixteen 64-bit lane addresses, which the
// A planes leave no registers for), and every one a counted instruction of the hand-over wait.
__device__ __forceinline__ void sgc_store(const float* sbase, unsigned voff, float v)
{
    asm volatile("global_store_dword %0, %1, %2" :: "v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ void sgc_store16(const double2* sbase, unsigned voff, double2 v)
{
    asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" :: "v"(voff), "v"(__builtin_bit_cast(sgc_u4, v)), "s"(sbase) : "memory");      // (the nop: the data registers are read before hipcc may reuse them)
}

// the three LDS-DMA instructions of this wave for the slot that begins at column n0: lane i of DMA q = 8 p + wave is piece 64 q + i =
// (p SC + n) CPR + cs of the image (SC CPR = 512 pieces per plane at every K: p is the instruction's number, (n, cs) the same in all three);
// w_off: the lane's byte offset of (n, cs ^ swz(n)) in a plane
template <int KT> __device__ __forceinline__ unsigned sgc_w_off(const SgArgs& g, int wave, int lane)
{
    constexpr unsigned CPR = 2 * KT;
    const unsigned rem = (unsigned)(wave * RG_WAVE + lane), n = rem / CPR, cs = rem - n * CPR;
    return (n * (unsigned)g.Kp + ((cs ^ sg_swz<KT>(n)) * 8u)) * 2u;
}
template <int KT> __device__ __forceinline__ void sgc_stage(const SgArgs& g, int n0, unsigned lds_dst, unsigned w_off, int wave)
{
#pragma unroll
    for (int p = 0; p < 3; p++)
        sgc_dma16((const void*)(g.Wt + (size_t)p * g.plane + (size_t)n0 * g.Kp), w_off, lds_dst + (unsigned)(p * SG_WAVES + wave) * 1024u);
}

template <int KT, bool INFOLD>
__global__ void __launch_bounds__(SG_WAVES* RG_WAVE, 4) k_gemm_strip_cols(SgArgs g)
{
    constexpr int K = 16 * KT, CPR = 2 * KT, ROWB = K * 2, SC = 4096 / K, SP = SC / 32;
    constexpr int SGC_AFTER = 16 * SP < 63 ? 16 * SP : 63;      // (the counter holds 63)
    extern __shared__ __align__(16) unsigned char Ws[];          // ring[2][3][SC][K] bf16, chunk-swizzled | double2 red[2][SG_WAVES][32]
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int row_tile = (int)blockIdx.x;                         // (consecutive row tiles on the 8 XCDs in turn)
    if (row_tile * SG_ROWS >= g.M) return;                        // (the whole workgroup, before any barrier)
    const int N = g.N;
    const int m0 = row_tile * SG_ROWS, r0 = m0 + 32 * wave;
    const int row = r0 + l31;
    const bool row_ok = row < g.M;
    const bool wave_full = r0 + 32 <= g.M;                        // wave-uniform: every store of the wave is a whole instruction

    // ---- the A phase, once: rows, clouds, slot 0 behind them, fold, split (as k_gemm_strip)
    float4 raw[KT][2];
    {
        const float* ap = g.A + (size_t)(row_ok ? row : g.M - 1) * g.lda + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < KT; ks++) {
            raw[ks][0] = *(const float4*)(ap + 16 * ks);
            raw[ks][1] = *(const float4*)(ap + 16 * ks + 4);
        }
    }
    const int4 ti = g.tile_info[row_tile];
    const unsigned lds_base = (unsigned)(unsigned long long)(rg_lds_ptr)(&Ws[0]);
    sgc_stage<KT>(g, 0, lds_base, sgc_w_off<KT>(g, wave, lane), wave);
    const int s_lo = ti.x, s_hi = ti.y;
    const bool one_cloud = s_lo == s_hi;
    bf16x8 fa[KT][3];
    {
        const float2* sp = nullptr;
        if (INFOLD) {
            const int my_seg = one_cloud ? s_lo : rg_find_segment(g.seg_off, g.n_seg, row_ok ? row : g.M - 1);
            sp = g.a_stats + (size_t)my_seg * K + 8 * hi;
        }
#pragma unroll
        for (int ks = 0; ks < KT; ks++) {
            float x[8] = {raw[ks][0].x, raw[ks][0].y, raw[ks][0].z, raw[ks][0].w, raw[ks][1].x, raw[ks][1].y, raw[ks][1].z, raw[ks][1].w};
            if (INFOLD) {
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const float4 s4 = *(const float4*)(sp + 16 * ks + e);
                    float u = (x[e] - s4.x) * s4.y;
                    x[e] = fmaxf(u, u * g.a_slope);
                    u = (x[e + 1] - s4.z) * s4.w;
                    x[e + 1] = fmaxf(u, u * g.a_slope);
                }
            }
            unsigned w[4][3];
#pragma unroll
            for (int e = 0; e < 4; e++) rg_split2(row_ok ? x[2 * e] : 0.f, row_ok ? x[2 * e + 1] : 0.f, w[e]);
#pragma unroll
            for (int p = 0; p < 3; p++) fa[ks][p] = __builtin_bit_cast(bf16x8, make_uint4(w[0][p], w[1][p], w[2][p], w[3][p]));
            if constexpr (KT == 8) __builtin_amdgcn_sched_barrier(0);      // (one k-step's split at a time: 64 registers of rows become 96 of planes)
        }
    }
    SGC_VM(0);                                                    // slot 0 has landed
    __syncthreads();

    const int nslot = (N + SC - 1) / SC;
    int par = 0;
    for (int s = 0; s < nslot; s++) {
        // The lane's offsets are derived again in front of every phase from an opaque copy of the thread id (SGC_LANE): hoisted out of the
        // walk they hold some ten registers beside the 96 of the K = 128 A planes and the 16 accumulators, and an A plane goes to scratch.
#define SGC_LANE() unsigned tl = (unsigned)t; asm volatile("" : "+v"(tl)); const int lane = (int)(tl & 63u), l31 = lane & 31, hi = lane >> 5
        const bool more = s + 1 < nslot;                          // workgroup-uniform
        if (more) { SGC_LANE(); (void)l31; (void)hi; sgc_stage<KT>(g, (s + 1) * SC, lds_base + (unsigned)((s + 1) & 1) * SGC_SLOT, sgc_w_off<KT>(g, wave, lane), wave); }
        const int npass = min(SP, (N - s * SC) >> 5);             // (SP wherever `more`)
#pragma unroll 1
        for (int j = 0; j < npass; j++) {
            const int n0 = s * SC + 32 * j;
            // ---- the MFMAs of one 32-column block: ks ascending, the six terms smallest first
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
            {
            SGC_LANE();
            const unsigned f_base = (unsigned)l31 * ROWB;
            const unsigned f_swz = (unsigned)hi ^ sg_swz<KT>((unsigned)l31);      // chunk (2 ks + hi) ^ swz = (2 ks) ^ (hi ^ swz)
#pragma unroll
            for (int ks = 0; ks < KT; ks++) {
                unsigned fo = (unsigned)(s & 1) * SGC_SLOT + (unsigned)(32 * j) * ROWB + f_base + (((unsigned)(2 * ks)) ^ f_swz) * 16u;
                const unsigned char* fp = Ws + fo;
                if constexpr (KT == 8) {
                    // 96 registers hold the A planes: two fragment registers instead of three, plane 1 read twice (the second offset laundered
                    // so that the read is not merged with the first), the order pinned so that no third fragment is live
                    bf16x8 b0 = __builtin_bit_cast(bf16x8, *(const uint4*)fp);
                    bf16x8 bx = __builtin_bit_cast(bf16x8, *(const uint4*)(fp + (size_t)SC * ROWB));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][2], b0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1], bx, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    asm volatile("" : "+v"(fo));
                    const unsigned char* fq = Ws + fo;
                    bx = __builtin_bit_cast(bf16x8, *(const uint4*)(fq + (size_t)2 * SC * ROWB));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], bx, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1], b0, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    bx = __builtin_bit_cast(bf16x8, *(const uint4*)(fq + (size_t)SC * ROWB));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], bx, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], b0, acc, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                } else {
                    bf16x8 fb[3];
#pragma unroll
                    for (int p = 0; p < 3; p++) fb[p] = __builtin_bit_cast(bf16x8, *(const uint4*)(fp + (size_t)p * SC * ROWB));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][2], fb[0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1], fb[1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], fb[2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][1], fb[0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], fb[1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ks][0], fb[0], acc, 0, 0, 0);
                }
            }
            }
            // ---- the block's stores first: sixteen whole instructions of a full wave, behind which the hand-over below counts.  They read the
            // accumulator from asm, where hipcc pads no hazard: twelve wait states between the last MFMA's result and its first reader.
            asm volatile("s_nop 7\n\ts_nop 3" : "+v"(acc));
            {
                SGC_LANE();
                const int rbase = r0 + 4 * hi;
                const unsigned c_off = ((unsigned)(4 * hi) * (unsigned)g.ldc + (unsigned)l31) * 4u;      // bytes from the wave's first row
                const float* cw = g.C + (size_t)r0 * g.ldc + n0;   // wave-uniform; the lane adds c_off = (4 hi ldc + l31) floats
                if (wave_full) {
#pragma unroll
                    for (int r = 0; r < 16; r++) sgc_store(cw + (size_t)((r & 3) + 8 * (r >> 2)) * g.ldc, c_off, acc[r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        if (rbase + (r & 3) + 8 * (r >> 2) < g.M) sgc_store(cw + (size_t)((r & 3) + 8 * (r >> 2)) * g.ldc, c_off, acc[r]);
                }
            }
            // ---- hand-over: slot s + 1 has landed once at most this wave's stores of slot s are outstanding
            const bool hand = more && j == npass - 1;             // workgroup-uniform
            if (hand) { if (wave_full) SGC_VM(SGC_AFTER); else SGC_VM(0); }
            // ---- statistics of the block, as k_gemm_strip: per-lane float64 over r, xor-32, waves 0..7 in LDS.  (A row outside the cloud adds
            // +0.0 and fma(0, 0, q) instead of being skipped: the same sums, and one live value at a time beside the A planes.)
            if (g.stat_partial) {                                 // workgroup-uniform
                int c_lo = ti.z, c_hi = min(ti.w, g.M);
#pragma unroll 1
                for (int sg = s_lo;;) {                           // workgroup-uniform; one pass almost always
                    double2* red = (double2*)(Ws + 2 * SGC_SLOT + (size_t)par * SGC_RED);
                    SGC_LANE();
                    const int rbase = r0 + 4 * hi;
                    asm volatile("" : "+v"(acc));                 // (keeps the sixteen float64 conversions inside this loop: 32 registers if hoisted)
                    const unsigned d0 = (unsigned)(rbase - c_lo), span = (unsigned)(c_hi - c_lo);
                    double sm = 0.0, q = 0.0;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const double v = (double)(d0 + (unsigned)((r & 3) + 8 * (r >> 2)) < span ? acc[r] : 0.f);
                        sm += v; q += v * v;
                        if constexpr (KT == 8) __builtin_amdgcn_sched_barrier(0);
                    }
                    sm += __shfl_xor(sm, 32, RG_WAVE); q += __shfl_xor(q, 32, RG_WAVE);
                    if (hi == 0) red[wave * 32 + l31] = make_double2(sm, q);
                    SGC_BARRIER();
                    if (tl < 32u) {
                        double2 a = red[tl];
#pragma unroll
                        for (int w = 1; w < SG_WAVES; w++) { const double2 b = red[w * 32 + tl]; a.x += b.x; a.y += b.y; }
                        sgc_store16(g.stat_partial + (size_t)(row_tile + sg) * N + n0, tl * 16u, a);
                    }
                    par ^= 1;
                    if (++sg > s_hi) break;
                    c_lo = __builtin_amdgcn_readfirstlane(g.seg_off[sg]); c_hi = min(__builtin_amdgcn_readfirstlane(g.seg_off[sg + 1]), g.M);
                }
            } else if (hand) SGC_BARRIER();
        }
    }
#undef SGC_LANE
}

// columns per workgroup column: the widest of 128 / 64 / 32 that divides N and whose weight planes + reduction buffer fit 64 KB of LDS (two
// workgroups per CU, four for the small ones)
int sg_cols_per_wg(int N, int K)
{
    for (int nb = 128; nb >= 32; nb /= 2)
        if (nb <= N && N % nb == 0 && (size_t)nb * K * 6 + (size_t)SG_WAVES * nb * 16 <= 64 * 1024) return nb;
    return 0;
}

// the (K, N) that take the column-walking form in the product: every shape with two or more column blocks that was measured, each faster per
// launch than one workgroup per column block by more than that form's run-to-run spread (profiles/strip_columns_launch_forms.md: 12 - 29 %
// against 0.5 - 11 %).  The encoder's large levels run (128, 256), (128, 512) and (64, 256); a shape that was not measured stays on k_gemm_strip.
bool sg_walks_columns(int N, int K)
{
    return (K == 128 && (N == 96 || N == 128 || N == 256 || N == 512)) || (K == 64 && (N == 192 || N == 256 || N == 512)) ||
           (K == 32 && (N == 192 || N == 256));
}

}  // namespace

extern "C" {

// 1 when regtr_gemm_stream serves the shape: K in {32, 64, 128}, N a multiple of 32 up to 512
int regtr_gemm_stream_supported(int M, int N, int K)
{
    return (M >= 0 && (K == 32 || K == 64 || K == 128) && N >= 32 && N <= 512 && N % 32 == 0 && sg_cols_per_wg(N, K) > 0) ? 1 : 0;
}

// rows per workgroup = statistics tile = the `rows` of the tile_info table (regtr_tile_segments) and of regtr_instnorm_finalize_tiles
int regtr_gemm_stream_tile_rows(void) { return SG_ROWS; }

// C[M, N] = A' W for the short-K, tall shapes of the shallow encoder levels; see the file header.
//   planes        weight planes of regtr_gemm_split_weights(W, .., N, K, ..)
//   a_stats       optional [n_seg, K, 2]: A' = LeakyReLU_a_slope(InstanceNorm(A)) per cloud (K <= 64)
//   seg_off       cloud offsets of the rows [n_seg + 1];  tile_info = regtr_tile_segments(seg_off, n_seg, M, 256, ..)
//   stat_partial  optional: (ceil(M / 256) + n_seg) * N double2 of per-(tile, cloud) column sums of C for
//                 regtr_instnorm_finalize_tiles(tile_rows = 256)
//   form          launch form of the strip<KT, NT, fold> route: 0 the measured choice per (K, N) (sg_walks_columns), 1 one workgroup per column
//                 block (k_gemm_strip), 2 one workgroup walking all column blocks (k_gemm_strip_cols) wherever there are two or more.  The
//                 forms write the same bits.
int regtr_gemm_stream_form(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K,
                           const float* a_stats, float a_slope, const int* seg_off, int n_seg, const void* tile_info,
                           double* stat_partial, int form, void* stream)
{
    if (!A || !planes || !C || !regtr_gemm_stream_supported(M, N, K) || lda < K || ldc < N || form < 0 || form > 2) return RG_ERR_ARG;
    if ((lda % 4) || ((uintptr_t)A % 16) || ((uintptr_t)planes % 16)) return RG_ERR_ARG;
    if (!seg_off || n_seg < 1 || !tile_info || ((uintptr_t)tile_info % 16)) return RG_ERR_ARG;
    if (a_stats && (K > 64 || ((uintptr_t)a_stats % 16))) return RG_ERR_ARG;
    if (stat_partial && ((uintptr_t)stat_partial % 16)) return RG_ERR_ARG;
    if (M == 0) return RG_OK;
    const RgPlaneDims pd = rg_plane_dims(N, K);
    SgArgs g{A, (const uint16_t*)planes, C, (const float2*)a_stats, seg_off, (const int4*)tile_info, (double2*)stat_partial,
             pd.elems(), M, N, pd.Kp, lda, ldc, n_seg, a_slope};
    const int NB = sg_cols_per_wg(N, K);
    hipStream_t st = (hipStream_t)stream;
    const int row_wg = rg_cdiv(rg_cdiv(M, SG_ROWS), 8) * 8;         // row tiles padded to the 8 XCDs
    if (regtr_gemm_stream_walks_columns(N, K, form)) {
        const dim3 grid((unsigned)row_wg);
#define SGC_L(KT_) do { if (a_stats) k_gemm_strip_cols<KT_, (KT_ <= 4)><<<grid, SG_WAVES * RG_WAVE, SGC_LDS, st>>>(g); \
                        else k_gemm_strip_cols<KT_, false><<<grid, SG_WAVES * RG_WAVE, SGC_LDS, st>>>(g); } while (0)
        if (K == 32) SGC_L(2);
        else if (K == 64) SGC_L(4);
        else SGC_L(8);
#undef SGC_L
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    }
    const size_t lds = (size_t)3 * NB * K * 2 + (size_t)SG_WAVES * NB * 16;
    const long long n_wg = (long long)row_wg * (N / NB);                                  // x column blocks
    if (n_wg > 0x7fffffffLL) return RG_ERR_ARG;
    const dim3 grid((unsigned)n_wg);
#define SG_L3(KT_, NT_) do { if (a_stats) k_gemm_strip<KT_, NT_, (KT_ <= 4)><<<grid, SG_WAVES * RG_WAVE, lds, st>>>(g); \
                             else k_gemm_strip<KT_, NT_, false><<<grid, SG_WAVES * RG_WAVE, lds, st>>>(g); } while (0)
#define SG_L2(KT_) do { if (NB == 32) SG_L3(KT_, 1); else if (NB == 64) SG_L3(KT_, 2); else SG_L3(KT_, 4); } while (0)
    if (K == 32) SG_L2(2);
    else if (K == 64) SG_L2(4);
    else SG_L2(8);
#undef SG_L2
#undef SG_L3
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

// 1 when regtr_gemm_stream_form(.., form, ..) launches the column-walking kernel for this (N, K), 0 when k_gemm_strip
int regtr_gemm_stream_walks_columns(int N, int K, int form)
{
    const int NB = sg_cols_per_wg(N, K);
    return (NB > 0 && N / NB >= 2 && (form == 2 || (form == 0 && sg_walks_columns(N, K)))) ? 1 : 0;
}

int regtr_gemm_stream(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K,
                      const float* a_stats, float a_slope, const int* seg_off, int n_seg, const void* tile_info,
                      double* stat_partial, void* stream)
{
    return regtr_gemm_stream_form(A, lda, planes, C, ldc, M, N, K, a_stats, a_slope, seg_off, n_seg, tile_info, stat_partial, 0, stream);
}

}  // extern "C"
