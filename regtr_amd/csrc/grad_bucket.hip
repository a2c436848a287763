// Packs the gradients of MANY tensors into one flat float32 bucket for gfx950: the accumulation buffer of gradient accumulation and the
// payload of the ONE all-reduce of data-parallel training (regtr_amd/grad_bucket.py).  Per tensor t and element i
//   accumulate == 0:  bucket[offset_t + i] = scale g_t[i]                       (g_t NULL: 0)
//   accumulate != 0:  bucket[offset_t + i] = fmaf(scale, g_t[i], bucket[...])   (g_t NULL: nothing is written)
// and nothing else of the bucket is touched: the padding between the segments keeps the zeros it was allocated with.
//
// MANY TENSORS PER LAUNCH as csrc/multi_tensor.h describes it (the by-value descriptor, the host walk, a workgroup's search for its
// tensor and slice); this file adds the entry -- GbEntry: (g, destination, n), GB_CHUNK per launch -- and the kernel body.  A workgroup
// owns one slice of GB_SLICE elements of one tensor.
// The destination of every group of four elements is 16-byte aligned (the bucket is, offsets are multiples of 4): 16-byte stores always,
// 16-byte loads of g where g sits on a 16-byte boundary (global_load_dwordx4 in the built ISA: check it after a change, the compiler
// folds a less explicit form into single-dword loads) and four 4-byte-aligned loads otherwise -- the same numbers either way.  One owner
// per element, no atomics, no workspace, no host wait; the result is a function of the inputs alone (bit-reproducible).
// Compiled with -ffp-contract=off (regtr_amd/build.py): the only fused operation is the fmaf written out below.
#include <math.h>

#include "common.h"
#include "multi_tensor.h"

namespace {

constexpr int GB_THREADS = 256;
constexpr int GB_SLICE = 4096;            // elements per workgroup (regtr_grad_pack_slice): four 16-byte groups per lane
constexpr int GB_CHUNK = 48;              // tensors per launch: regtr_optim_chunk_tensors()' number (csrc/optim.hip)

struct GbEntry {
    const float* g;                       // NULL: zeros (only under assign; an accumulate call makes no entry for it)
    float* dst;                           // bucket + offset
    long long n;
    int wg0;                              // first workgroup of this tensor within the launch
    int pad_;
};
static_assert(sizeof(GbEntry) == 32, "GbEntry layout");

typedef MtChunk<GbEntry, GB_CHUNK> GbChunk;
static_assert(sizeof(GbChunk) <= 4096 - 64, "the descriptor and the other arguments must fit the 4 KiB kernel-argument segment");

typedef float gb_f4 __attribute__((ext_vector_type(4)));       // a 16-byte-aligned vector: one global_load / store_dwordx4

// One slice [lo, hi) of one tensor.  VEC: g sits on a 16-byte boundary and is read with 16-byte-aligned 16-byte loads; otherwise four
// scalar loads per group, which promise 4-byte alignment only (the compiler may still issue them as one dwordx4 of that alignment, which
// the memory system splits) -- the same numbers.  A template, dispatched once per workgroup, so that the two forms stay two loops in
// the ISA: as one loop with a wave-uniform `vec ? :` the compiler folded the 16-byte load into four single-dword loads.  The bucket
// side is 16-byte aligned in both.
template <bool VEC, bool ZERO, bool ACC>
__device__ __forceinline__ void gb_slice(const float* __restrict__ g, float* __restrict__ dst, long long lo, long long hi, float scale)
{
    for (long long i = lo + 4 * (long long)threadIdx.x; i < hi; i += 4 * GB_THREADS) {
        if (i + 4 <= hi) {
            gb_f4 x = {0.f, 0.f, 0.f, 0.f};
            if (!ZERO) {
                if (VEC) {
                    x = *reinterpret_cast<const gb_f4*>(__builtin_assume_aligned(g + i, 16));
                } else {
                    x.x = g[i]; x.y = g[i + 1]; x.z = g[i + 2]; x.w = g[i + 3];
                }
            }
            gb_f4* out = reinterpret_cast<gb_f4*>(__builtin_assume_aligned(dst + i, 16));
            gb_f4 r;
            if (ACC) {
                const gb_f4 o = *out;
                r.x = fmaf(scale, x.x, o.x); r.y = fmaf(scale, x.y, o.y); r.z = fmaf(scale, x.z, o.z); r.w = fmaf(scale, x.w, o.w);
            } else if (ZERO) {
                r = x;                                                         // zeros, whatever the scale (an infinite one included)
            } else {
                r.x = scale * x.x; r.y = scale * x.y; r.z = scale * x.z; r.w = scale * x.w;
            }
            *out = r;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (i + k < hi) {
                    const float x = ZERO ? 0.f : g[i + k];
                    dst[i + k] = ACC ? fmaf(scale, x, dst[i + k]) : (ZERO ? 0.f : scale * x);
                }
            }
        }
    }
}

// Block b < n_wg of a launch, both kernels' body.  ok == 0 (the guarded kernel under a cleared flag; accumulate == 0 then): zeros.
__device__ __forceinline__ void gb_block(const GbChunk& c, int b, float scale, int accumulate, int ok)
{
    const GbEntry& e = c.e[mt_find_entry(c, b)];
    const float* g = e.g;
    float* dst = e.dst;
    long long lo, hi;
    mt_slice<GB_SLICE>(b, e, lo, hi);
    // one choice per workgroup (per tensor: wave-uniform)
    if (ok == 0 || g == nullptr) {                                             // (a NULL g only under assign: an accumulate call makes no entry)
        gb_slice<true, true, false>(g, dst, lo, hi, scale);
    } else if (((uintptr_t)g & 15) == 0) {
        if (accumulate != 0) gb_slice<true, false, true>(g, dst, lo, hi, scale);
        else gb_slice<true, false, false>(g, dst, lo, hi, scale);
    } else {
        if (accumulate != 0) gb_slice<false, false, true>(g, dst, lo, hi, scale);
        else gb_slice<false, false, false>(g, dst, lo, hi, scale);
    }
}

__global__ __launch_bounds__(GB_THREADS) void k_grad_pack(const GbChunk c, float scale, int accumulate)
{
    if ((int)blockIdx.x < c.n_wg) gb_block(c, blockIdx.x, scale, accumulate, 1);
}

// k_grad_pack under a device flag (skip_nonfinite): flag[0] != 0 -- k_grad_pack's arithmetic exactly; flag[0] == 0 -- zeros in every
// segment under assign, nothing written under accumulate.  The flag is wave-uniform and read once per workgroup.  n_good (optional, the
// first launch of a call only): thread 0 of workgroup 0 counts the flag into it with ordinary stores -- set under assign, added under
// accumulate, never scaled.  The grid holds at least one workgroup so that a call without an element to pack still counts.
__global__ __launch_bounds__(GB_THREADS) void k_grad_pack_guarded(const GbChunk c, float scale, int accumulate, const int* __restrict__ flag,
                                                                  float* __restrict__ n_good)
{
    const int b = blockIdx.x;
    const int ok = __builtin_amdgcn_readfirstlane(flag[0]);
    if (n_good != nullptr && b == 0 && threadIdx.x == 0) n_good[0] = (accumulate != 0 ? n_good[0] : 0.0f) + (ok != 0 ? 1.0f : 0.0f);
    if (b >= c.n_wg) return;
    if (ok == 0 && accumulate != 0) return;
    gb_block(c, b, scale, accumulate, ok);
}

// both entry points' argument checks
int gb_check(const regtr_bucket_tensor_t* t, int n_tensors, float* bucket, long long n_bucket, float scale)
{
    if (n_tensors < 0 || n_bucket < 0 || (n_tensors > 0 && !t) || scale != scale || ((uintptr_t)bucket & 15)) return RG_ERR_ARG;
    long long end = 0;                                                         // one past the previous segment
    bool work = false;
    for (int i = 0; i < n_tensors; i++) {
        if (t[i].n < 0 || t[i].n >= (1ll << 40) || ((uintptr_t)t[i].g & 3)) return RG_ERR_ARG;
        if (t[i].offset < 0 || (t[i].offset & 3) || t[i].offset < end || t[i].offset > n_bucket || t[i].n > n_bucket - t[i].offset)
            return RG_ERR_ARG;                                                 // inside [0, n_bucket), ascending, no overlap
        end = t[i].offset + t[i].n;
        work = work || t[i].n > 0;
    }
    if (work && !bucket) return RG_ERR_ARG;
    return RG_OK;
}

// the walk over a checked table: a tensor with nothing to write (no element; no gradient under accumulate) makes no entry
template <typename Launch>
int gb_walk(const regtr_bucket_tensor_t* t, int n_tensors, float* bucket, int accumulate, Launch launch)
{
    return mt_walk<GbChunk>(
        n_tensors, false, [&](int i) { return !t[i].g && accumulate != 0 ? 0 : (t[i].n + GB_SLICE - 1) / GB_SLICE; },
        [&](int i, GbEntry& e) { e.g = t[i].g; e.dst = bucket + t[i].offset; e.n = t[i].n; e.pad_ = 0; }, launch);
}

}  // namespace

extern "C" {

int regtr_grad_pack_slice(void) { return GB_SLICE; }

int regtr_grad_pack(const regtr_bucket_tensor_t* t, int n_tensors, float* bucket, long long n_bucket, float scale, int accumulate,
                    void* stream)
{
    const int st = gb_check(t, n_tensors, bucket, n_bucket, scale);
    if (st != RG_OK) return st;
    return gb_walk(t, n_tensors, bucket, accumulate, [&](const GbChunk& c) {
        k_grad_pack<<<c.n_wg, GB_THREADS, 0, (hipStream_t)stream>>>(c, scale, accumulate);
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    });
}

int regtr_grad_pack_guarded(const regtr_bucket_tensor_t* t, int n_tensors, float* bucket, long long n_bucket, float scale, int accumulate,
                            const int* flag, float* n_good, void* stream)
{
    if (!flag || (((uintptr_t)flag | (uintptr_t)n_good) & 3)) return RG_ERR_ARG;
    const int st = gb_check(t, n_tensors, bucket, n_bucket, scale);
    if (st != RG_OK) return st;
    bool first = true;                                                         // the call's first launch counts the flag into n_good
    auto launch = [&](const GbChunk& c) {
        k_grad_pack_guarded<<<c.n_wg > 0 ? c.n_wg : 1, GB_THREADS, 0, (hipStream_t)stream>>>(c, scale, accumulate, flag, first ? n_good : nullptr);
        RG_RETURN_IF_LAUNCH_FAILED();
        first = false;
        return RG_OK;
    };
    const int walked = gb_walk(t, n_tensors, bucket, accumulate, launch);
    if (walked != RG_OK || !first || !n_good) return walked;
    return launch(GbChunk{});                                                  // nothing to pack: one workgroup, for the count alone
}

}  // extern "C"
