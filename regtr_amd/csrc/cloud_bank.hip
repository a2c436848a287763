// The cloud bank's one kernel for gfx950 (regtr_amd/cloud_bank.py; RegTR.register, CloudBank.select).
//
// regtr_gather_segments -- packs whole clouds of a bank into a new order: destination cloud d = bank cloud cloud_of[d], its rows copied
//                          from bank_seg[cloud_of[d]] ... to dst_seg[d] ..., for up to three row arrays at once: feats [*, D], pe [*, D]
//                          (optional) and xyz [*, 3] (optional).  A copy, nothing else: ~2 KB per token at D = 256 with pe, so the bar is
//                          the HBM copy rate and the shape is the plain streaming one --
//                            * grid (row tiles of the longest selected cloud, destination clouds), GS_THREADS lanes, GS_ROWS rows per
//                              workgroup: a 64-pair register (128 clouds of ~440 tokens) is ~2000 workgroups of 4 waves on 256 CUs
//                              (a handful of VGPRs, no LDS: nothing but the CU's wave slots limits how many are resident);
//                            * a wide row is D / 4 float4: consecutive lanes take consecutive 16-byte pieces of a row, then the next
//                              row (D = 256: one wave-instruction = one 1 KiB row), GS_UNROLL loads in flight per lane before the first
//                              store -- at D = 256 every lane moves 8 pieces per array;
//                            * the xyz rows of a tile are 3 GS_ROWS consecutive floats (12-byte rows have no 16-byte alignment): the
//                              first 3 GS_ROWS lanes copy one float each;
//                            * rows past the cloud's end are CLAMPED to its last row on the load side and not stored; a tile wholly
//                              past the end, or an empty cloud, leaves before its first load (workgroup-uniform).
//                          Every destination row is written exactly once by one lane group; no atomics, no workspace, no LDS: the
//                          result is bit-reproducible.  The tables are clamped to the arrays (n_bank rows in, n_out rows out), so no
//                          table content can make an access leave them.
#include "common.h"

namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_ROWS = 32;        // rows of one cloud per workgroup
constexpr int GS_UNROLL = 4;       // 16-byte loads in flight per lane and array

struct GatherSegArgs {
    const float4* feats; const float4* pe; const float* xyz;
    float4* out_feats; float4* out_pe; float* out_xyz;
    const int* bank_seg; const int* cloud_of; const int* dst_seg;
    int n_bank_clouds, n_bank, n_out, Q;      // Q = D / 4: 16-byte pieces per wide row
};

// rows [r0, r0 + GS_ROWS) of one cloud: piece i of the tile is (row r0 + i / Q, piece i % Q)
__device__ __forceinline__ void gs_copy_wide(const float4* __restrict__ src, float4* __restrict__ dst, int r0, int len, int Q)
{
    const int pieces = GS_ROWS * Q;
    for (int i0 = threadIdx.x; i0 < pieces; i0 += GS_UNROLL * GS_THREADS) {
        float4 v[GS_UNROLL];
        int row[GS_UNROLL], q[GS_UNROLL];
#pragma unroll
        for (int u = 0; u < GS_UNROLL; u++) {
            const int i = min(i0 + u * GS_THREADS, pieces - 1);
            row[u] = r0 + i / Q;
            q[u] = i % Q;
            v[u] = src[(size_t)min(row[u], len - 1) * Q + q[u]];          // clamped row: always inside the cloud
        }
#pragma unroll
        for (int u = 0; u < GS_UNROLL; u++)
            if (i0 + u * GS_THREADS < pieces && row[u] < len) dst[(size_t)row[u] * Q + q[u]] = v[u];
    }
}

__global__ __launch_bounds__(GS_THREADS) void k_gather_segments(GatherSegArgs a)
{
    const int d = blockIdx.y;
    const int c = min(max(a.cloud_of[d], 0), a.n_bank_clouds - 1);
    const int s0 = min(max(a.bank_seg[c], 0), a.n_bank);
    const int d0 = min(max(a.dst_seg[d], 0), a.n_out);
    const int len = min(min(a.bank_seg[c + 1], a.n_bank) - s0, a.n_out - d0);
    const int r0 = blockIdx.x * GS_ROWS;
    if (r0 >= len) return;                                  // (an empty cloud, or a tile past this cloud's end)
    gs_copy_wide(a.feats + (size_t)s0 * a.Q, a.out_feats + (size_t)d0 * a.Q, r0, len, a.Q);
    if (a.pe) gs_copy_wide(a.pe + (size_t)s0 * a.Q, a.out_pe + (size_t)d0 * a.Q, r0, len, a.Q);
    if (a.xyz && threadIdx.x < 3 * GS_ROWS) {
        const int i = 3 * r0 + (int)threadIdx.x;            // float i of the cloud's xyz rows
        const float v = a.xyz[3 * (size_t)s0 + min(i, 3 * len - 1)];
        if (i < 3 * len) a.out_xyz[3 * (size_t)d0 + i] = v;
    }
}

inline bool gs_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int regtr_gather_segments(const float* feats, const float* pe, const float* xyz, int D, const int* bank_seg, int n_bank_clouds, int n_bank,
                          const int* cloud_of, const int* dst_seg, int n_dst, int n_out, int max_len, float* out_feats, float* out_pe,
                          float* out_xyz, void* stream)
{
    if (D < 4 || D % 4 != 0 || n_bank_clouds < 0 || n_bank < 0 || n_dst < 0 || n_out < 0 || max_len < 0) return RG_ERR_ARG;
    if (n_dst > 65535) return RG_ERR_ARG;                   // (gridDim.y)
    if (n_dst == 0 || max_len == 0 || n_out == 0) return RG_OK;      // no selected row: the pointers (of empty arrays: often NULL) are not looked at
    if ((pe != nullptr) != (out_pe != nullptr) || (xyz != nullptr) != (out_xyz != nullptr)) return RG_ERR_ARG;
    if (!gs_aligned16(feats) || !gs_aligned16(pe) || !gs_aligned16(out_feats) || !gs_aligned16(out_pe)) return RG_ERR_ARG;
    if (!feats || !out_feats || !bank_seg || !cloud_of || !dst_seg || n_bank_clouds < 1) return RG_ERR_ARG;
    GatherSegArgs a{(const float4*)feats, (const float4*)pe, xyz, (float4*)out_feats, (float4*)out_pe, out_xyz,
                    bank_seg, cloud_of, dst_seg, n_bank_clouds, n_bank, n_out, D / 4};
    k_gather_segments<<<dim3(rg_cdiv(max_len, GS_ROWS), n_dst), GS_THREADS, 0, (hipStream_t)stream>>>(a);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
