// The optimiser step on the device for gfx950: the global gradient norm of torch.nn.utils.clip_grad_norm_ and the single-tensor
// AdamW / Adam update of torch.optim, over MANY tensors per launch (the reference's trainer.py:104-121 step over 140-157 parameter
// tensors).
//
// MULTI-TENSOR DESCRIPTOR -- OptChunk, a plain struct passed BY VALUE as the kernel argument: up to OPT_CHUNK entries of
//   (p, g, m, v, n, the per-tensor scalars, wg0 = the first workgroup index of the tensor within the launch)
// plus the entry count.  3856 bytes: with the other arguments it stays inside the 4 KiB kernel-argument segment.  There is no
// device-side pointer table, no host-to-device copy and nothing cached across steps: the host entry point walks the caller's tensor
// list, fills one chunk after another on the stack and launches each; 157 tensors are four launches.  A workgroup finds its (tensor,
// slice) by a binary search of blockIdx.x in the entries' wg0 prefix -- scalar loads from the argument segment, the index wave-uniform
// by construction and passed through readfirstlane so that everything read from the entry stays in SGPRs.
//
// regtr_grad_sumsq       -- workgroup w of tensor t sums the squares of slice [s OPT_NORM_SLICE, (s + 1) OPT_NORM_SLICE) of g_t in float64:
//                           lane l takes elements 1024 j + 4 l + (0..3) for j ascending, then the fixed xor tree over the wave and the
//                           waves in order; one float64 partial per slice at index part0_t + s.  The slicing is a function of the tensor
//                           lengths alone (never of the grid, the chunking or a pointer's alignment: a gradient that does not start on a
//                           16-byte boundary is read with scalar loads in the SAME element order), so the partials and their order are a
//                           function of the shapes.
// regtr_grad_norm_finish -- one workgroup adds the partials in float64 (a strided partial per lane ascending, the xor tree, the waves in
//                           order), total_norm = (float)sqrt(sum), clip_coef = min(1, max_norm / (total_norm + 1e-6)) in float32 as
//                           clip_grad_norm_ computes it (a NaN stays a NaN); max_norm <= 0: coef = 1.
// regtr_adam_step        -- per element in float32, rounded per operation (no contraction), torch's _single_tensor_adam order:
//                             g' = g coef;  decoupled: p = p (1 - lr wd)   else: g' = g' + wd p
//                             m = b1 m + (1 - b1) g';  v = b2 v + ((1 - b2) g') g'
//                             p = p - (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
//                           16-byte loads and stores when p, g, m and v all sit on 16-byte boundaries, scalar ones otherwise and for the
//                           n % 4 tail.  The clipped gradient is NOT written back to g (clip_grad_norm_ scales .grad in place; nothing
//                           in the reference reads it afterwards).
//
// No atomics, no workspace beyond the partials, no host wait; every result is a function of the inputs alone (bit-reproducible).
// Compiled with -ffp-contract=off (regtr_amd/build.py).
#include <math.h>

#include "common.h"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_NORM_SLICE = 8192;      // elements per workgroup of regtr_grad_sumsq (regtr_optim_norm_slice)
constexpr int OPT_STEP_SLICE = 4096;      // elements per workgroup of regtr_adam_step (regtr_optim_step_slice)
constexpr int OPT_CHUNK = 48;             // tensors per launch (regtr_optim_chunk_tensors)

struct OptEntry {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    float decay, wd, b1, omb1, b2, omb2, step_size, sqrt_bc2, eps;      // float64 on the host, rounded once
    int wg0;                                                            // first workgroup of this tensor within the launch
};
static_assert(sizeof(OptEntry) == 80, "OptEntry layout");

struct OptChunk {
    OptEntry e[OPT_CHUNK];
    int n_entries;
    int n_wg;
    long long part0;                      // regtr_grad_sumsq: index of the chunk's first partial
};
static_assert(sizeof(OptChunk) <= 4096 - 64, "the descriptor and the other arguments must fit the 4 KiB kernel-argument segment");

// the entry whose workgroup range holds block b: the last one with wg0 <= b (entries hold at least one workgroup each)
__device__ __forceinline__ int opt_find_entry(const OptChunk& c, int b)
{
    int lo = 0, hi = c.n_entries;         // invariant: e[lo].wg0 <= b < e[hi].wg0 (e[n_entries].wg0 = n_wg)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c.e[mid].wg0 <= b) lo = mid; else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

__device__ __forceinline__ double opt_block_sum(double s, double* sh)
{
    s = rg_wave_sum(s);                                                        // fixed xor tree
    if (rg_lane() == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < OPT_THREADS / RG_WAVE; w++) t += sh[w];               // waves in order
    return t;
}

__global__ __launch_bounds__(OPT_THREADS) void k_grad_sumsq(const OptChunk c, double* __restrict__ partials)
{
    __shared__ double sh[OPT_THREADS / RG_WAVE];
    const int b = blockIdx.x;
    if (b >= c.n_wg) return;
    const int ei = opt_find_entry(c, b);
    const float* __restrict__ g = c.e[ei].g;
    const long long n = c.e[ei].n;
    const int slice = b - c.e[ei].wg0;
    const long long lo = (long long)slice * OPT_NORM_SLICE;
    const long long hi = lo + OPT_NORM_SLICE < n ? lo + OPT_NORM_SLICE : n;
    const bool vec = ((uintptr_t)g & 15) == 0;                                 // (per tensor: wave-uniform)
    double s = 0.0;
    for (long long i = lo + 4 * (long long)threadIdx.x; i < hi; i += 4 * OPT_THREADS) {
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (i + 4 <= hi) {
            if (vec) {
                const float4 q = *reinterpret_cast<const float4*>(g + i);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) x[k] = g[i + k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (i + k < hi) x[k] = g[i + k];                              // (a zero adds +0.0: the sum is that of the real elements)
        }
#pragma unroll
        for (int k = 0; k < 4; k++) s += (double)x[k] * (double)x[k];
    }
    const double t = opt_block_sum(s, sh);
    if (threadIdx.x == 0) partials[c.part0 + b] = t;
}

__global__ __launch_bounds__(OPT_THREADS) void k_grad_norm_finish(const double* __restrict__ partials, long long n_partials, float max_norm,
                                                                  float* __restrict__ out)
{
    __shared__ double sh[OPT_THREADS / RG_WAVE];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n_partials; i += OPT_THREADS) s += partials[i];
    const double t = opt_block_sum(s, sh);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(t);
        float coef = 1.0f;
        if (max_norm > 0.0f) {
            const float c = max_norm / (norm + 1e-6f);
            coef = c > 1.0f ? 1.0f : c;                                        // torch.clamp(c, max=1): a NaN stays a NaN
        }
        out[0] = norm;
        out[1] = coef;
    }
}

__device__ __forceinline__ void opt_update(float& p, float g, float& m, float& v, float coef, const OptEntry& e, bool decoupled)
{
    g = g * coef;
    if (decoupled) p = p * e.decay;
    else g = g + e.wd * p;
    m = e.b1 * m + e.omb1 * g;
    v = e.b2 * v + (e.omb2 * g) * g;
    const float denom = sqrtf(v) / e.sqrt_bc2 + e.eps;
    p = p - e.step_size * (m / denom);
}

__global__ __launch_bounds__(OPT_THREADS) void k_adam_step(const OptChunk c, const float* __restrict__ clip_coef, int decoupled)
{
    const int b = blockIdx.x;
    if (b >= c.n_wg) return;
    const int ei = opt_find_entry(c, b);
    const OptEntry& e = c.e[ei];
    float* __restrict__ p = e.p;
    const float* __restrict__ g = e.g;
    float* __restrict__ m = e.m;
    float* __restrict__ v = e.v;
    const long long n = e.n;
    const long long lo = (long long)(b - e.wg0) * OPT_STEP_SLICE;
    const long long hi = lo + OPT_STEP_SLICE < n ? lo + OPT_STEP_SLICE : n;
    const float coef = clip_coef ? clip_coef[0] : 1.0f;
    const bool dec = decoupled != 0;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;      // (per tensor: wave-uniform)
    for (long long i = lo + 4 * (long long)threadIdx.x; i < hi; i += 4 * OPT_THREADS) {
        if (vec && i + 4 <= hi) {
            float4 P = *reinterpret_cast<const float4*>(p + i), M = *reinterpret_cast<const float4*>(m + i);
            float4 V = *reinterpret_cast<const float4*>(v + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            opt_update(P.x, G.x, M.x, V.x, coef, e, dec);
            opt_update(P.y, G.y, M.y, V.y, coef, e, dec);
            opt_update(P.z, G.z, M.z, V.z, coef, e, dec);
            opt_update(P.w, G.w, M.w, V.w, coef, e, dec);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (i + k < hi) {
                    float P = p[i + k], M = m[i + k], V = v[i + k];
                    opt_update(P, g[i + k], M, V, coef, e, dec);
                    p[i + k] = P; m[i + k] = M; v[i + k] = V;
                }
            }
        }
    }
}

// Walks the caller's tensors, `launch`-ing one full chunk after another.  slice: elements per workgroup; need_state: p, m, v are used.
template <typename Launch>
int opt_for_each_chunk(const regtr_optim_tensor_t* t, int n_tensors, int slice, bool need_state, Launch launch)
{
    if (n_tensors < 0 || (n_tensors > 0 && !t)) return RG_ERR_ARG;
    for (int i = 0; i < n_tensors; i++) {
        if (t[i].n < 0 || t[i].n >= (1ll << 40)) return RG_ERR_ARG;
        if (t[i].n > 0 && (!t[i].g || (need_state && (!t[i].p || !t[i].m || !t[i].v)))) return RG_ERR_ARG;
        if ((uintptr_t)t[i].g & 3) return RG_ERR_ARG;
        if (need_state && (((uintptr_t)t[i].p | (uintptr_t)t[i].m | (uintptr_t)t[i].v) & 3)) return RG_ERR_ARG;
    }
    OptChunk c;
    c.n_entries = 0; c.n_wg = 0; c.part0 = 0;
    for (int i = 0; i <= n_tensors; i++) {
        const long long wgs = i < n_tensors ? (t[i].n + slice - 1) / slice : 0;
        const bool flush = i == n_tensors || c.n_entries == OPT_CHUNK || (long long)c.n_wg + wgs > 0x7fffffffll;
        if (flush && c.n_entries > 0) {
            const int st = launch(c);
            if (st != RG_OK) return st;
            c.part0 += c.n_wg;
            c.n_entries = 0; c.n_wg = 0;
        }
        if (i == n_tensors || wgs == 0) continue;                              // (an empty tensor: nothing to do)
        OptEntry& e = c.e[c.n_entries++];
        const double lr = t[i].lr, wd = t[i].weight_decay, b1 = t[i].beta1, b2 = t[i].beta2;
        e.p = t[i].p; e.g = t[i].g; e.m = t[i].m; e.v = t[i].v; e.n = t[i].n;
        e.decay = (float)(1.0 - lr * wd); e.wd = (float)wd;
        e.b1 = (float)b1; e.omb1 = (float)(1.0 - b1); e.b2 = (float)b2; e.omb2 = (float)(1.0 - b2);
        e.step_size = (float)(lr / t[i].bias_correction1); e.sqrt_bc2 = (float)t[i].sqrt_bias_correction2; e.eps = (float)t[i].eps;
        e.wg0 = c.n_wg;
        c.n_wg += (int)wgs;
    }
    return RG_OK;
}

}  // namespace

extern "C" {

int regtr_optim_norm_slice(void) { return OPT_NORM_SLICE; }
int regtr_optim_step_slice(void) { return OPT_STEP_SLICE; }
int regtr_optim_chunk_tensors(void) { return OPT_CHUNK; }

int regtr_grad_sumsq(const regtr_optim_tensor_t* tensors, int n_tensors, double* partials, long long n_partials, void* stream)
{
    if (n_tensors < 0 || n_partials < 0 || (n_tensors > 0 && !tensors)) return RG_ERR_ARG;
    long long need = 0;
    for (int i = 0; i < n_tensors; i++) {
        if (tensors[i].n < 0 || tensors[i].n >= (1ll << 40)) return RG_ERR_ARG;
        need += (tensors[i].n + OPT_NORM_SLICE - 1) / OPT_NORM_SLICE;
    }
    if (need != n_partials || (need > 0 && !partials)) return RG_ERR_ARG;      // the caller sized the partials from the same lengths
    return opt_for_each_chunk(tensors, n_tensors, OPT_NORM_SLICE, false, [&](const OptChunk& c) {
        k_grad_sumsq<<<c.n_wg, OPT_THREADS, 0, (hipStream_t)stream>>>(c, partials);
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    });
}

int regtr_grad_norm_finish(const double* partials, long long n_partials, float max_norm, float* norm_coef, void* stream)
{
    if (n_partials < 0 || !norm_coef || (n_partials > 0 && !partials) || max_norm != max_norm) return RG_ERR_ARG;
    k_grad_norm_finish<<<1, OPT_THREADS, 0, (hipStream_t)stream>>>(partials, n_partials, max_norm, norm_coef);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_adam_step(const regtr_optim_tensor_t* tensors, int n_tensors, const float* clip_coef, int decoupled, void* stream)
{
    for (int i = 0; i < n_tensors && tensors; i++) {
        const regtr_optim_tensor_t& t = tensors[i];
        if (!(t.bias_correction1 > 0.0) || !(t.sqrt_bias_correction2 > 0.0) || !(t.eps >= 0.0) || t.lr != t.lr || t.weight_decay != t.weight_decay)
            return RG_ERR_ARG;
    }
    return opt_for_each_chunk(tensors, n_tensors, OPT_STEP_SLICE, true, [&](const OptChunk& c) {
        k_adam_step<<<c.n_wg, OPT_THREADS, 0, (hipStream_t)stream>>>(c, clip_coef, decoupled);
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    });
}

}  // extern "C"
