// Shared device helpers for the gfx950 kernels.  CDNA4 only: 64-wide wavefronts are assumed throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "regtr_hip.h"      // the public C ABI: every definition below is checked against its declaration at compile time

#define RG_WAVE 64

// status codes of the C-ABI (include/regtr_hip.h)
#define RG_OK 0
#define RG_ERR_LAUNCH (-1)
#define RG_ERR_ARG (-2)
#define RG_ERR_WORKSPACE (-3)

#define RG_RETURN_IF_LAUNCH_FAILED()                      \
    do {                                                  \
        if (hipGetLastError() != hipSuccess) return RG_ERR_LAUNCH; \
    } while (0)

// A kernel launched with more dynamic LDS than the default limit: raise the kernel's limit on the CURRENT device, once per device
// and kernel (a process-wide flag would leave a second GPU of the process at the default), thread-safe.  false = the device refused.
template <auto Kernel>
static inline bool rg_allow_dynamic_lds(size_t bytes)
{
    static unsigned long long ok_mask = 0;       // bit d: the attribute has been set on device d (devices >= 64: set every time)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    if (dev < 64 && (__atomic_load_n(&ok_mask, __ATOMIC_ACQUIRE) >> dev & 1)) return true;
    if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    if (dev < 64) __atomic_fetch_or(&ok_mask, 1ull << dev, __ATOMIC_RELEASE);
    return true;
}

static inline size_t rg_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int rg_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
static inline int rg_xcd_grid(int nblocks) { return (nblocks + 7) / 8 * 8; }
static inline unsigned rg_next_pow2(unsigned x)
{
    unsigned p = 1;
    while (p < x) p <<= 1;
    return p;
}

// Rows of one cloud per workgroup of an InstanceNorm launch (norm.hip forward, norm_pool_bwd.hip backward) over clouds of at most max_len
// rows.  128 everywhere a launch fills the chip anyway; a pair or two per forward leaves the deep levels with a handful of 128-row workgroups
// (751 rows x 1024 channels: 8 workgroups, each thread walking 128 rows -- 35 us for 9 MB), so the chunk is halved until the launch has ~1000
// workgroups or a workgroup is down to four row steps / 8 rows.  Host-side and a function of the launch geometry only (never of the data);
// the statistics kernels add a cloud's chunks in chunk order whatever their length, so results stay run-to-run deterministic.
static inline int rg_in_rows(int max_len, int n_clouds, int C)
{
    const int TR = 256 / (C >> 2);
    int rows = 128;
    while (rows > 4 * TR && rows > 8 && (long long)rg_cdiv(max_len > 0 ? max_len : 1, rows) * n_clouds < 1024) rows >>= 1;
    return rows;
}

// carve a sub-buffer out of a caller-provided workspace (256-B aligned)
struct RgCarver {
    char* base;
    size_t off;
    size_t cap;
    explicit RgCarver(void* p, size_t bytes) : base((char*)p), off(0), cap(bytes) {}
    template <typename T>
    T* take(size_t n)
    {
        off = rg_align_up(off, 256);
        T* p = (T*)(base + off);
        off += n * sizeof(T);
        return p;
    }
    bool ok() const { return off <= cap; }
};

__device__ __forceinline__ int rg_lane() { return threadIdx.x & (RG_WAVE - 1); }

// Workgroup b of a launch runs on XCD b % 8, and every XCD has its own L2.  Kernels whose neighbouring work items touch
// overlapping memory (queries gathering the rows of their spatial neighbours) want neighbouring items on ONE L2: launch a
// grid padded to a multiple of 8 (rg_xcd_grid) and take work block rg_xcd_block(blockIdx.x, gridDim.x) -- every XCD then owns
// one contiguous eighth of the blocks instead of every eighth block.
__device__ __forceinline__ int rg_xcd_block(int b, int grid_padded) { return (b & 7) * (grid_padded >> 3) + (b >> 3); }

// index of the segment containing row i, given exclusive offsets off[0..nseg] (off[0] = 0)
__device__ __forceinline__ int rg_find_segment(const int* __restrict__ off, int nseg, int i)
{
    int lo = 0, hi = nseg;  // invariant: off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// The same for a WAVE-UNIFORM row i, by the whole wave at once: lanes read 64 boundaries per step (one coalesced load, one
// memory round trip) and count those <= i with a ballot -- instead of log2(nseg) DEPENDENT loads per lane.
__device__ __forceinline__ int rg_find_segment_wave(const int* __restrict__ off, int nseg, int i)
{
    int seg = 0;
    for (int base = 0; base < nseg; base += RG_WAVE) {      // boundaries off[1 .. nseg - 1]; off[b] <= i  =>  segment >= b
        const int b = base + rg_lane() + 1;
        const bool le = b < nseg && off[b] <= i;
        seg += __popcll(__ballot(le));
    }
    return seg;
}

__device__ __forceinline__ uint32_t rg_hash64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return (uint32_t)k;
}

// float <-> int with the same ordering as the floats (for atomicMin/atomicMax on floats)
__device__ __forceinline__ int rg_f2ord(float f)
{
    int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float rg_ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7FFFFFFF); }

__device__ __forceinline__ float rg_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, RG_WAVE);
    return v;
}
__device__ __forceinline__ double rg_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, RG_WAVE);
    return v;
}
__device__ __forceinline__ float rg_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, RG_WAVE));
    return v;
}

// Sum over the THREADS values of the calling workgroup in float64, in a fixed order (every thread calls it; every thread gets the sum):
// the xor tree over each wave, then the waves in order.  sh: THREADS / RG_WAVE doubles of LDS.  The leading barrier lets consecutive
// calls share them; a kernel that calls this once and touches sh nowhere else passes REUSE = false and does without it.
template <int THREADS, bool REUSE = true>
__device__ __forceinline__ double rg_block_sum(double v, double* sh)
{
    v = rg_wave_sum(v);
    if (REUSE) __syncthreads();
    if (rg_lane() == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < THREADS / RG_WAVE; w++) t += sh[w];
    return t;
}

// Exclusive scan over the THREADS values of the calling workgroup (every thread calls it; any integer type); *total = their sum.
// sh: THREADS / RG_WAVE values of LDS, free for reuse when the call returns.
template <int THREADS, typename T>
__device__ __forceinline__ T rg_block_exclusive_scan(T v, T* total, T* sh)
{
    const int lane = rg_lane(), wave = threadIdx.x >> 6;
    T inc = v;      // wave inclusive scan
#pragma unroll
    for (int o = 1; o < RG_WAVE; o <<= 1) {
        const T t = __shfl_up(inc, o, RG_WAVE);
        if (lane >= o) inc += t;
    }
    if (lane == RG_WAVE - 1) sh[wave] = inc;
    __syncthreads();
    T wave_off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / RG_WAVE; w++) {
        const T s = sh[w];
        if (w < wave) wave_off += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return wave_off + inc - v;
}
