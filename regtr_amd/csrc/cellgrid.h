// The read side of the support-point cell grid that regtr_cellgrid_build (preprocess.hip) writes: the live table size, the home slot of a
// key, the cell of a point, the packed slot a probe reads, the lookup, and where the packed table and the cell-sorted supports lie in the
// caller's workspace.  Shared by the query kernels of preprocess.hip and by icp.hip, so that both probe one table with one arithmetic.
#pragma once
#include "common.h"

namespace {

// tile of the exclusive scan over uint64 (preprocess.hip); the grid workspace holds one scan descriptor per tile of its table
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

// ------------------------------------------------------------------------------------------------
// spatial hash: slots hold the index of the first point that claimed them ("representative")
// ------------------------------------------------------------------------------------------------
// Hash tables are ALLOCATED for the level-0 capacity (live counts exist only on the device) but SIZED, on the device, for
// the live count of their level: the power of two >= 1.5 n (>= 64).  Clears, key passes, scans and the packed-slot pass
// then touch 1.5-3 n slots instead of 3 x capacity, and probes of a deep level stay in a table 1/64 the size.
__device__ __forceinline__ unsigned rg_live_table(int n)
{
    unsigned want = (unsigned)n + ((unsigned)n >> 1);
    if (want < 64u) want = 64u;
    return 1u << (32 - __clz((int)(want - 1u)));
}
static inline unsigned rg_table_capacity(int n_cap)       // host twin: upper bound of rg_live_table over n <= n_cap
{
    unsigned want = (unsigned)n_cap + ((unsigned)n_cap >> 1);
    if (want < 64u) want = 64u;
    return rg_next_pow2(want);
}

constexpr int CELL_BITS = 21;
constexpr int64_t CELL_BIAS = 1 << 20;

// Home slot of a key: the plain 64-bit mix, salted with the cloud.
// (Measured and dropped, round 6: BLOCK-LOCAL homes for the cell keys of the radius grid -- the 4 x 4 x 4 block of cells picks a 64-slot region,
//  the cell's position in its block the slot inside it -- so that the 27 probes of a neighbourhood fall into <= 8 regions of 2 KB instead of 27 random
//  lines of a table of up to 537 MB, a wave's slot run is one spatial block and the cell-sorted supports are spatially coherent.  Tables bit-identical;
//  192-pair pyramid 12.17 -> 18.46 ms: k_radius_query_self 1219 -> 2533 us per launch, k_radius_query 788 -> 1105, k_insert 267 -> 278
//  (profiles/r06_d_block_hash.md).  A planar surface fills CONTIGUOUS runs of 16 slots of its region; where two blocks share a region a probe walks such a
//  run, and a wave waits for the slowest of its 27 probing lanes -- most neighbourhoods then pay 5-10 dependent round trips instead of 1-2; and the
//  occupied slots bunch into 27 % of the regions, so the cell-centric kernel's slot runs are badly balanced.  The locality bought nothing even where
//  neither effect applies (k_insert): these kernels wait on dependent round trips and issue slots, not on HBM bytes.)
__device__ __forceinline__ unsigned rg_home_slot(uint64_t key, int cid, unsigned mask)
{
    return rg_hash64(key ^ ((uint64_t)(cid + 1) * 0x9E3779B97F4A7C15ULL)) & mask;
}

__device__ __forceinline__ void cell_of(float x, float y, float z, double inv_cs, int64_t& cx, int64_t& cy, int64_t& cz)
{
    cx = (int64_t)floor((double)x * inv_cs);
    cy = (int64_t)floor((double)y * inv_cs);
    cz = (int64_t)floor((double)z * inv_cs);
}
__device__ __forceinline__ uint64_t cell_key(int64_t cx, int64_t cy, int64_t cz)
{
    const uint64_t m = (1ULL << CELL_BITS) - 1;
    return ((uint64_t)(cx + CELL_BIAS) & m) | (((uint64_t)(cy + CELL_BIAS) & m) << CELL_BITS) |
           (((uint64_t)(cz + CELL_BIAS) & m) << (2 * CELL_BITS));
}

// One probe = ONE memory round trip: everything a radius query needs from a hash slot, packed into 32 bytes by
// k_pack_slots once the cell starts are known (the separate rep / tkey / tcid / cnt / cell_start arrays would be three
// dependent loads per probe, and the query kernel is latency bound).
struct __align__(16) CellSlot {
    uint64_t key;
    int cid;
    int used;        // >= 0: occupied
    int cnt;
    unsigned start;
    int pad[2];
};

// lookup in the packed table: (count, start) of cell `key` of cloud `cid`, count 0 when the cell is empty
__device__ __forceinline__ void slot_find(const CellSlot* __restrict__ slots, unsigned mask, uint64_t key, int cid, int& cnt,
                                          int& start)
{
    unsigned h = rg_home_slot(key, cid, mask);
    cnt = 0; start = 0;
    for (;;) {
        const uint4 a = *(const uint4*)&slots[h];                 // key | cid | used
        const uint2 b = *(const uint2*)((const char*)&slots[h] + 16);   // cnt | start
        if ((int)a.w < 0) return;
        if ((((uint64_t)a.y << 32) | a.x) == key && (int)a.z == cid) { cnt = (int)b.x; start = (int)b.y; return; }
        h = (h + 1) & mask;
    }
}

struct GridView {
    const CellSlot* slots;
    const float4* sorted;
    double inv_cs;
};

// ------------------------------------------------------------------------------------------------
// the grid workspace (regtr_cellgrid_ws_bytes): what the build writes and where the query kernels find it
// ------------------------------------------------------------------------------------------------
struct GridBuffers {
    uint64_t* pkey; int* pcid; int* slot_of; int* rep; int* cnt; int* fill;
    uint64_t* tkey; int* tcid; uint64_t* scan_in; uint64_t* cell_start; uint64_t* bsum; float4* sorted; CellSlot* slots;
    unsigned T;
    size_t bytes;
};

GridBuffers carve_grid(void* ws, size_t ws_bytes, int ns_cap)
{
    GridBuffers b;
    RgCarver c(ws, ws_bytes);
    const unsigned T = rg_table_capacity(ns_cap);
    b.T = T;
    b.pkey = c.take<uint64_t>(ns_cap); b.pcid = c.take<int>(ns_cap); b.slot_of = c.take<int>(ns_cap);
    b.rep = c.take<int>(T); b.cnt = c.take<int>(T); b.fill = c.take<int>(T);
    b.tkey = c.take<uint64_t>(T); b.tcid = c.take<int>(T);
    b.scan_in = c.take<uint64_t>(T); b.cell_start = c.take<uint64_t>(T);
    b.bsum = c.take<uint64_t>(rg_cdiv(T, SCAN_TILE) + 2);           // scan state (ticket + one descriptor per tile) + the live table length
    b.sorted = c.take<float4>(ns_cap);
    b.slots = c.take<CellSlot>(T);
    b.bytes = rg_align_up(c.off, 256);
    return b;
}

// 1 / cell size of the grid a radius is searched on: cells of radius * (1 + 1e-6), so a ball never reaches past its 27 cells
inline double grid_inv_cell(float radius) { return 1.0 / ((double)radius * (1.0 + 1e-6)); }

// what the query kernels read of a carved grid workspace built (regtr_cellgrid_build) with `radius`
GridView grid_view(const GridBuffers& b, float radius) { return GridView{b.slots, b.sorted, grid_inv_cell(radius)}; }

}  // namespace
