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

// the entry whose workgroup range holds block b: the last one with wg0 <= b (OptChunk's entries hold at least one workgroup each; an
// empty entry of an OptGuardChunk shares its wg0 with the entry after it, or has n_wg: it is never the LAST one with wg0 <= b)
template <typename Chunk>
__device__ __forceinline__ int opt_find_entry(const Chunk& c, int b)
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

// ---- the guarded step (skip_nonfinite): the decision to leave a step out is taken and obeyed on the device --------------------------------
// The guard word, four int32 on the device: {ok, applied_steps, skipped_steps, reserved}.  ONE lane of ONE workgroup (thread 0 of
// k_grad_norm_finish_guarded) writes it with ordinary stores; every other kernel only reads guard[0], once per workgroup.
constexpr int OPT_GUARD_CHUNK = 40;       // tensors per guarded launch (regtr_optim_guarded_chunk_tensors): the entries carry float64 scalars

struct OptGuardEntry {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    double lr, wd, b1, b2, eps;           // the host's float64 hyper-parameters: every float32 scalar is formed from them on the device
    int step;                             // index of the tensor's step count in the device vector
    int wg0;                              // first workgroup of this tensor within the launch (an empty tensor holds none)
};
static_assert(sizeof(OptGuardEntry) == 88, "OptGuardEntry layout");

struct OptGuardChunk {
    OptGuardEntry e[OPT_GUARD_CHUNK];
    int n_entries;
    int n_wg;
};
static_assert(sizeof(OptGuardChunk) <= 3856, "the guarded descriptor must not outgrow OptChunk: the 4 KiB kernel-argument segment");

// beta^t for an integer t >= 0 by binary exponentiation (never the math library's pow: a numpy restatement reproduces this bit for bit).
// Plain float64 squarings double the relative error at every step -- 0.999^t came out up to 5e4 ulp off for t <= 2^20 -- so every value
// is carried as an unevaluated sum hi + lo (Dekker's product over Veltkamp's split: float64 multiplies, adds and subtracts only, in the
// order written, no fma and no contraction), which leaves the result within 1 ulp of the correctly rounded power.
__device__ __forceinline__ void opt_dd_mul(double ah, double al, double bh, double bl, double& hi, double& lo)
{
    const double SPLIT = 134217729.0;                                          // 2^27 + 1
    const double p = ah * bh;
    double c = SPLIT * ah;
    const double a1 = c - (c - ah), a2 = ah - a1;
    c = SPLIT * bh;
    const double b1 = c - (c - bh), b2 = bh - b1;
    double e = ((a1 * b1 - p) + a1 * b2 + a2 * b1) + a2 * b2;                  // ah bh = p + e exactly
    e = e + (ah * bl + al * bh);
    hi = p + e;
    lo = e - (hi - p);
}

__device__ __forceinline__ double opt_ipow(double b, long long t)
{
    double rh = 1.0, rl = 0.0, bh = b, bl = 0.0;
    while (t > 0) {
        if (t & 1) opt_dd_mul(rh, rl, bh, bl, rh, rl);
        opt_dd_mul(bh, bl, bh, bl, bh, bl);
        t >>= 1;
    }
    return rh;
}

// the two per-step scalars of a tensor at step count t, float64 rounded once: lr / (1 - b1^t) and sqrt(1 - b2^t)
__device__ __forceinline__ void opt_bias_scalars(double lr, double b1, double b2, float t, float& step_size, float& sqrt_bc2)
{
    const long long ti = (long long)t;
    step_size = (float)(lr / (1.0 - opt_ipow(b1, ti)));
    sqrt_bc2 = (float)sqrt(1.0 - opt_ipow(b2, ti));
}

__global__ __launch_bounds__(OPT_THREADS) void k_grad_norm_finish_guarded(const double* __restrict__ partials, long long n_partials,
                                                                          float max_norm, const float* __restrict__ grad_scale,
                                                                          float* __restrict__ out, int* __restrict__ guard)
{
    __shared__ double sh[OPT_THREADS / RG_WAVE];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n_partials; i += OPT_THREADS) s += partials[i];
    const double t = opt_block_sum(s, sh);
    if (threadIdx.x == 0) {
        const float gs = grad_scale ? grad_scale[0] : 1.0f;
        const float norm = (float)sqrt(t) * gs;                                // (gs == 1: k_grad_norm_finish's bits)
        float coef = 1.0f;
        if (max_norm > 0.0f) {
            const float c = max_norm / (norm + 1e-6f);
            coef = c > 1.0f ? 1.0f : c;
        }
        const int ok = (isfinite(norm) && isfinite(gs)) ? 1 : 0;
        out[0] = norm;
        out[1] = coef;
        guard[0] = ok;
        guard[1] = guard[1] + ok;
        guard[2] = guard[2] + (1 - ok);
    }
}

// steps[e.step] += 1 for every tensor of the chunk (the empty ones too) when the guard says ok, and the tensor's two per-step scalars
// from the advanced count into step_scalars[2 e.step ..]: one thread per entry, so the float64 power, divide and square root run once
// per TENSOR (formed in k_adam_step_guarded they ran once per workgroup, ~2900 times a step: +34 us of kernel time, measured)
__global__ __launch_bounds__(64) void k_adam_steps_advance(const OptGuardChunk c, float* __restrict__ steps, float* __restrict__ step_scalars,
                                                           const int* __restrict__ guard)
{
    if (guard[0] == 0) return;
    const int i = threadIdx.x;
    if (i < c.n_entries) {
        const OptGuardEntry& e = c.e[i];
        const float t = steps[e.step] + 1.0f;                                  // (distinct indices: the caller's contract)
        steps[e.step] = t;
        opt_bias_scalars(e.lr, e.b1, e.b2, t, step_scalars[2 * (long long)e.step], step_scalars[2 * (long long)e.step + 1]);
    }
}

__global__ __launch_bounds__(OPT_THREADS) void k_adam_step_guarded(const OptGuardChunk c, const float* __restrict__ step_scalars,
                                                                   const float* __restrict__ clip_coef,
                                                                   const float* __restrict__ grad_scale, const int* __restrict__ guard,
                                                                   int decoupled)
{
    const int b = blockIdx.x;
    if (b >= c.n_wg) return;
    if (__builtin_amdgcn_readfirstlane(guard[0]) == 0) return;                // a skipped step: not one byte is written
    const int ei = opt_find_entry(c, b);
    const OptGuardEntry& ge = c.e[ei];
    OptEntry e;                                                                // k_adam_step's scalars, in opt_for_each_chunk's order
    e.decay = (float)(1.0 - ge.lr * ge.wd); e.wd = (float)ge.wd;
    e.b1 = (float)ge.b1; e.omb1 = (float)(1.0 - ge.b1); e.b2 = (float)ge.b2; e.omb2 = (float)(1.0 - ge.b2);
    e.eps = (float)ge.eps;
    e.step_size = step_scalars[2 * (long long)ge.step];                       // (k_adam_steps_advance left them, from the advanced count)
    e.sqrt_bc2 = step_scalars[2 * (long long)ge.step + 1];
    float* __restrict__ p = ge.p;
    const float* __restrict__ g = ge.g;
    float* __restrict__ m = ge.m;
    float* __restrict__ v = ge.v;
    const long long n = ge.n;
    const long long lo = (long long)(b - ge.wg0) * OPT_STEP_SLICE;
    const long long hi = lo + OPT_STEP_SLICE < n ? lo + OPT_STEP_SLICE : n;
    const float coef = clip_coef ? clip_coef[0] : 1.0f;
    const float gs = grad_scale ? grad_scale[0] : 1.0f;
    const bool dec = decoupled != 0;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;      // (per tensor: wave-uniform)
    for (long long i = lo + 4 * (long long)threadIdx.x; i < hi; i += 4 * OPT_THREADS) {
        if (vec && i + 4 <= hi) {
            float4 P = *reinterpret_cast<const float4*>(p + i), M = *reinterpret_cast<const float4*>(m + i);
            float4 V = *reinterpret_cast<const float4*>(v + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            opt_update(P.x, G.x * gs, M.x, V.x, coef, e, dec);                 // (gs == 1: g itself)
            opt_update(P.y, G.y * gs, M.y, V.y, coef, e, dec);
            opt_update(P.z, G.z * gs, M.z, V.z, coef, e, dec);
            opt_update(P.w, G.w * gs, M.w, V.w, coef, e, dec);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (i + k < hi) {
                    float P = p[i + k], M = m[i + k], V = v[i + k];
                    opt_update(P, g[i + k] * gs, M, V, coef, e, dec);
                    p[i + k] = P; m[i + k] = M; v[i + k] = V;
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_adam_bias_scalars(double lr, double b1, double b2, const float* __restrict__ steps, int n,
                                                          float* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) opt_bias_scalars(lr, b1, b2, steps[i], out[2 * i], out[2 * i + 1]);
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

int regtr_optim_guarded_chunk_tensors(void) { return OPT_GUARD_CHUNK; }

int regtr_grad_norm_finish_guarded(const double* partials, long long n_partials, float max_norm, const float* grad_scale, float* norm_coef,
                                   int* guard, void* stream)
{
    if (n_partials < 0 || !norm_coef || !guard || (n_partials > 0 && !partials) || max_norm != max_norm) return RG_ERR_ARG;
    if (((uintptr_t)norm_coef | (uintptr_t)guard | (uintptr_t)grad_scale) & 3) return RG_ERR_ARG;
    k_grad_norm_finish_guarded<<<1, OPT_THREADS, 0, (hipStream_t)stream>>>(partials, n_partials, max_norm, grad_scale, norm_coef, guard);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_adam_step_guarded(const regtr_optim_guarded_tensor_t* t, int n_tensors, float* steps, float* step_scalars, long long n_steps,
                            const float* clip_coef, const float* grad_scale, const int* guard, int decoupled, void* stream)
{
    if (n_tensors < 0 || n_steps < 0 || (n_tensors > 0 && (!t || !steps || !step_scalars || !guard))) return RG_ERR_ARG;
    if (((uintptr_t)steps | (uintptr_t)step_scalars | (uintptr_t)clip_coef | (uintptr_t)grad_scale | (uintptr_t)guard) & 3) return RG_ERR_ARG;
    for (int i = 0; i < n_tensors; i++) {
        if (t[i].n < 0 || t[i].n >= (1ll << 40) || t[i].step_index < 0 || t[i].step_index >= n_steps) return RG_ERR_ARG;
        if (t[i].n > 0 && (!t[i].g || !t[i].p || !t[i].m || !t[i].v)) return RG_ERR_ARG;
        if (((uintptr_t)t[i].g | (uintptr_t)t[i].p | (uintptr_t)t[i].m | (uintptr_t)t[i].v) & 3) return RG_ERR_ARG;
        if (!(t[i].eps >= 0.0) || t[i].lr != t[i].lr || t[i].weight_decay != t[i].weight_decay) return RG_ERR_ARG;
        if (!(t[i].beta1 >= 0.0 && t[i].beta1 < 1.0) || !(t[i].beta2 >= 0.0 && t[i].beta2 < 1.0)) return RG_ERR_ARG;
    }
    OptGuardChunk c;
    c.n_entries = 0; c.n_wg = 0;
    for (int i = 0; i <= n_tensors; i++) {
        const long long wgs = i < n_tensors ? (t[i].n + OPT_STEP_SLICE - 1) / OPT_STEP_SLICE : 0;
        const bool flush = i == n_tensors || c.n_entries == OPT_GUARD_CHUNK || (long long)c.n_wg + wgs > 0x7fffffffll;
        if (flush && c.n_entries > 0) {
            // the counts first (an empty tensor's too), then the update reads them: two launches of one stream, in order
            k_adam_steps_advance<<<1, 64, 0, (hipStream_t)stream>>>(c, steps, step_scalars, guard);
            RG_RETURN_IF_LAUNCH_FAILED();
            if (c.n_wg > 0) {
                k_adam_step_guarded<<<c.n_wg, OPT_THREADS, 0, (hipStream_t)stream>>>(c, step_scalars, clip_coef, grad_scale, guard, decoupled);
                RG_RETURN_IF_LAUNCH_FAILED();
            }
            c.n_entries = 0; c.n_wg = 0;
        }
        if (i == n_tensors) continue;
        OptGuardEntry& e = c.e[c.n_entries++];
        e.p = t[i].p; e.g = t[i].g; e.m = t[i].m; e.v = t[i].v; e.n = t[i].n;
        e.lr = t[i].lr; e.wd = t[i].weight_decay; e.b1 = t[i].beta1; e.b2 = t[i].beta2; e.eps = t[i].eps;
        e.step = t[i].step_index;
        e.wg0 = c.n_wg;
        c.n_wg += (int)wgs;
    }
    return RG_OK;
}

int regtr_adam_bias_scalars(double lr, double beta1, double beta2, const float* steps, int n, float* out, void* stream)
{
    if (n < 0 || (n > 0 && (!steps || !out)) || (((uintptr_t)steps | (uintptr_t)out) & 3)) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    k_adam_bias_scalars<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(lr, beta1, beta2, steps, n, out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
