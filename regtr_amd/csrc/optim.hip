// The optimiser step on the device for gfx950: the global gradient norm of torch.nn.utils.clip_grad_norm_ and the single-tensor
// AdamW / Adam update of torch.optim, over MANY tensors per launch (the reference's trainer.py:104-121 step over 140-157 parameter
// tensors).
//
// MANY TENSORS PER LAUNCH as csrc/multi_tensor.h describes it: the descriptor (MtChunk, by value in the kernel-argument segment), the
// host walk that fills and launches one chunk after another (mt_walk) and a workgroup's search for its (tensor, slice) (mt_find_entry,
// mt_slice) live there, once.  This file adds the entries -- OptEntry: (p, g, m, v, n, nine float32 scalars), 48 per launch, 157 tensors
// are four launches; OptGuardEntry: the guarded step's, with the float64 hyper-parameters, 40 per launch -- and the kernels.
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
#include "multi_tensor.h"

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

typedef MtChunk<OptEntry, OPT_CHUNK> OptChunk;                                // (3856 bytes)
static_assert(sizeof(OptChunk) <= 4096 - 64, "the descriptor and the other arguments must fit the 4 KiB kernel-argument segment");

__global__ __launch_bounds__(OPT_THREADS) void k_grad_sumsq(const OptChunk c, double* __restrict__ partials)
{
    __shared__ double sh[OPT_THREADS / RG_WAVE];
    const int b = blockIdx.x;
    if (b >= c.n_wg) return;
    const int ei = mt_find_entry(c, b);
    const float* __restrict__ g = c.e[ei].g;
    long long lo, hi;
    mt_slice<OPT_NORM_SLICE>(b, c.e[ei], lo, hi);
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
    const double t = rg_block_sum<OPT_THREADS, false>(s, sh);      // (sh is used this once: no leading barrier)
    if (threadIdx.x == 0) partials[c.part0 + b] = t;
}

// Both finishes.  grad_scale (NULL: none) multiplies the norm before the coefficient is formed; guard (NULL: none) is the guard word,
// four int32 on the device, {ok, applied_steps, skipped_steps, reserved}: ONE lane of ONE workgroup -- thread 0 here -- writes it with
// ordinary stores; every other kernel only reads guard[0], once per workgroup.
__global__ __launch_bounds__(OPT_THREADS) void k_grad_norm_finish(const double* __restrict__ partials, long long n_partials, float max_norm,
                                                                  const float* __restrict__ grad_scale, float* __restrict__ out,
                                                                  int* __restrict__ guard)
{
    __shared__ double sh[OPT_THREADS / RG_WAVE];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n_partials; i += OPT_THREADS) s += partials[i];
    const double t = rg_block_sum<OPT_THREADS, false>(s, sh);      // (sh is used this once: no leading barrier)
    if (threadIdx.x == 0) {
        float norm = (float)sqrt(t), gs = 1.0f;
        if (grad_scale) {
            gs = grad_scale[0];
            norm = norm * gs;                                                  // (gs == 1: the unscaled bits)
        }
        float coef = 1.0f;
        if (max_norm > 0.0f) {
            const float c = max_norm / (norm + 1e-6f);
            coef = c > 1.0f ? 1.0f : c;                                        // torch.clamp(c, max=1): a NaN stays a NaN
        }
        out[0] = norm;
        out[1] = coef;
        if (guard) {
            const int ok = (isfinite(norm) && isfinite(gs)) ? 1 : 0;
            guard[0] = ok;
            guard[1] = guard[1] + ok;
            guard[2] = guard[2] + (1 - ok);
        }
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

// The elements [lo, hi) of one tensor, both step kernels' loop.  e: the scalars only.  SCALED: the gradient is multiplied by gs first
// (the guarded step; gs == 1 leaves g's bits).  Everything here is wave-uniform but i.
template <bool SCALED>
__device__ __forceinline__ void opt_step_slice(float* p_, const float* g_, float* m_, float* v_, long long lo, long long hi, const OptEntry& e,
                                               float coef, float gs, int decoupled)
{
    float* __restrict__ p = p_;
    const float* __restrict__ g = g_;
    float* __restrict__ m = m_;
    float* __restrict__ v = v_;
    const bool dec = decoupled != 0;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;      // (per tensor: wave-uniform)
    for (long long i = lo + 4 * (long long)threadIdx.x; i < hi; i += 4 * OPT_THREADS) {
        if (vec && i + 4 <= hi) {
            float4 P = *reinterpret_cast<const float4*>(p + i), M = *reinterpret_cast<const float4*>(m + i);
            float4 V = *reinterpret_cast<const float4*>(v + i);
            const float4 G = *reinterpret_cast<const float4*>(g + i);
            opt_update(P.x, SCALED ? G.x * gs : G.x, M.x, V.x, coef, e, dec);
            opt_update(P.y, SCALED ? G.y * gs : G.y, M.y, V.y, coef, e, dec);
            opt_update(P.z, SCALED ? G.z * gs : G.z, M.z, V.z, coef, e, dec);
            opt_update(P.w, SCALED ? G.w * gs : G.w, M.w, V.w, coef, e, dec);
            *reinterpret_cast<float4*>(p + i) = P;
            *reinterpret_cast<float4*>(m + i) = M;
            *reinterpret_cast<float4*>(v + i) = V;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (i + k < hi) {
                    float P = p[i + k], M = m[i + k], V = v[i + k];
                    opt_update(P, SCALED ? g[i + k] * gs : g[i + k], M, V, coef, e, dec);
                    p[i + k] = P; m[i + k] = M; v[i + k] = V;
                }
            }
        }
    }
}

__global__ __launch_bounds__(OPT_THREADS) void k_adam_step(const OptChunk c, const float* __restrict__ clip_coef, int decoupled)
{
    const int b = blockIdx.x;
    if (b >= c.n_wg) return;
    const OptEntry& e = c.e[mt_find_entry(c, b)];
    long long lo, hi;
    mt_slice<OPT_STEP_SLICE>(b, e, lo, hi);
    opt_step_slice<false>(e.p, e.g, e.m, e.v, lo, hi, e, clip_coef ? clip_coef[0] : 1.0f, 1.0f, decoupled);
}

// ---- the guarded step (skip_nonfinite): the decision to leave a step out is taken and obeyed on the device --------------------------------
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

typedef MtChunk<OptGuardEntry, OPT_GUARD_CHUNK> OptGuardChunk;
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
    const OptGuardEntry& ge = c.e[mt_find_entry(c, b)];
    OptEntry e;                                                                // k_adam_step's scalars, in opt_walk's order
    e.decay = (float)(1.0 - ge.lr * ge.wd); e.wd = (float)ge.wd;
    e.b1 = (float)ge.b1; e.omb1 = (float)(1.0 - ge.b1); e.b2 = (float)ge.b2; e.omb2 = (float)(1.0 - ge.b2);
    e.eps = (float)ge.eps;
    e.step_size = step_scalars[2 * (long long)ge.step];                       // (k_adam_steps_advance left them, from the advanced count)
    e.sqrt_bc2 = step_scalars[2 * (long long)ge.step + 1];
    long long lo, hi;
    mt_slice<OPT_STEP_SLICE>(b, ge, lo, hi);
    opt_step_slice<true>(ge.p, ge.g, ge.m, ge.v, lo, hi, e, clip_coef ? clip_coef[0] : 1.0f, grad_scale ? grad_scale[0] : 1.0f, decoupled);
}

__global__ __launch_bounds__(64) void k_adam_bias_scalars(double lr, double b1, double b2, const float* __restrict__ steps, int n,
                                                          float* __restrict__ out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) opt_bias_scalars(lr, b1, b2, steps[i], out[2 * i], out[2 * i + 1]);
}

// one tensor of either table: n in [0, 2^40), 4-byte aligned pointers, none of them NULL with elements to work on (state: p, m, v too)
bool opt_tensor_ok(const float* p, const float* g, const float* m, const float* v, long long n, bool state)
{
    if (n < 0 || n >= (1ll << 40) || ((uintptr_t)g & 3) || (n > 0 && !g)) return false;
    return !state || (!(((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 3) && !(n > 0 && (!p || !m || !v)));
}

// the walk over a checked regtr_optim_tensor_t table, `slice` elements per workgroup; an empty tensor makes no entry
template <typename Launch>
int opt_walk(const regtr_optim_tensor_t* t, int n_tensors, int slice, Launch launch)
{
    return mt_walk<OptChunk>(
        n_tensors, false, [&](int i) { return (t[i].n + slice - 1) / slice; },
        [&](int i, OptEntry& e) {
            const double lr = t[i].lr, wd = t[i].weight_decay, b1 = t[i].beta1, b2 = t[i].beta2;
            e.p = t[i].p; e.g = t[i].g; e.m = t[i].m; e.v = t[i].v; e.n = t[i].n;
            e.decay = (float)(1.0 - lr * wd); e.wd = (float)wd;
            e.b1 = (float)b1; e.omb1 = (float)(1.0 - b1); e.b2 = (float)b2; e.omb2 = (float)(1.0 - b2);
            e.step_size = (float)(lr / t[i].bias_correction1); e.sqrt_bc2 = (float)t[i].sqrt_bias_correction2; e.eps = (float)t[i].eps;
        },
        launch);
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
        if (!opt_tensor_ok(nullptr, tensors[i].g, nullptr, nullptr, tensors[i].n, false)) return RG_ERR_ARG;
        need += (tensors[i].n + OPT_NORM_SLICE - 1) / OPT_NORM_SLICE;
    }
    if (need != n_partials || (need > 0 && !partials)) return RG_ERR_ARG;      // the caller sized the partials from the same lengths
    return opt_walk(tensors, n_tensors, OPT_NORM_SLICE, [&](const OptChunk& c) {
        k_grad_sumsq<<<c.n_wg, OPT_THREADS, 0, (hipStream_t)stream>>>(c, partials);
        RG_RETURN_IF_LAUNCH_FAILED();
        return RG_OK;
    });
}

int regtr_grad_norm_finish(const double* partials, long long n_partials, float max_norm, float* norm_coef, void* stream)
{
    if (n_partials < 0 || !norm_coef || (n_partials > 0 && !partials) || max_norm != max_norm) return RG_ERR_ARG;
    k_grad_norm_finish<<<1, OPT_THREADS, 0, (hipStream_t)stream>>>(partials, n_partials, max_norm, nullptr, norm_coef, nullptr);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_adam_step(const regtr_optim_tensor_t* tensors, int n_tensors, const float* clip_coef, int decoupled, void* stream)
{
    if (n_tensors < 0 || (n_tensors > 0 && !tensors)) return RG_ERR_ARG;
    for (int i = 0; i < n_tensors; i++) {
        const regtr_optim_tensor_t& t = tensors[i];
        if (!opt_tensor_ok(t.p, t.g, t.m, t.v, t.n, true)) return RG_ERR_ARG;
        if (!(t.bias_correction1 > 0.0) || !(t.sqrt_bias_correction2 > 0.0) || !(t.eps >= 0.0) || t.lr != t.lr || t.weight_decay != t.weight_decay)
            return RG_ERR_ARG;
    }
    return opt_walk(tensors, n_tensors, OPT_STEP_SLICE, [&](const OptChunk& c) {
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
    k_grad_norm_finish<<<1, OPT_THREADS, 0, (hipStream_t)stream>>>(partials, n_partials, max_norm, grad_scale, norm_coef, guard);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_adam_step_guarded(const regtr_optim_guarded_tensor_t* t, int n_tensors, float* steps, float* step_scalars, long long n_steps,
                            const float* clip_coef, const float* grad_scale, const int* guard, int decoupled, void* stream)
{
    if (n_tensors < 0 || n_steps < 0 || (n_tensors > 0 && (!t || !steps || !step_scalars || !guard))) return RG_ERR_ARG;
    if (((uintptr_t)steps | (uintptr_t)step_scalars | (uintptr_t)clip_coef | (uintptr_t)grad_scale | (uintptr_t)guard) & 3) return RG_ERR_ARG;
    for (int i = 0; i < n_tensors; i++) {
        if (!opt_tensor_ok(t[i].p, t[i].g, t[i].m, t[i].v, t[i].n, true) || t[i].step_index < 0 || t[i].step_index >= n_steps) return RG_ERR_ARG;
        if (!(t[i].eps >= 0.0) || t[i].lr != t[i].lr || t[i].weight_decay != t[i].weight_decay) return RG_ERR_ARG;
        if (!(t[i].beta1 >= 0.0 && t[i].beta1 < 1.0) || !(t[i].beta2 >= 0.0 && t[i].beta2 < 1.0)) return RG_ERR_ARG;
    }
    return mt_walk<OptGuardChunk>(
        n_tensors, true /* an empty tensor's count advances too */, [&](int i) { return (t[i].n + OPT_STEP_SLICE - 1) / OPT_STEP_SLICE; },
        [&](int i, OptGuardEntry& e) {
            e.p = t[i].p; e.g = t[i].g; e.m = t[i].m; e.v = t[i].v; e.n = t[i].n;
            e.lr = t[i].lr; e.wd = t[i].weight_decay; e.b1 = t[i].beta1; e.b2 = t[i].beta2; e.eps = t[i].eps;
            e.step = t[i].step_index;
        },
        [&](const OptGuardChunk& c) {
            // the counts first (an empty tensor's too), then the update reads them: two launches of one stream, in order
            k_adam_steps_advance<<<1, 64, 0, (hipStream_t)stream>>>(c, steps, step_scalars, guard);
            RG_RETURN_IF_LAUNCH_FAILED();
            if (c.n_wg > 0) {
                k_adam_step_guarded<<<c.n_wg, OPT_THREADS, 0, (hipStream_t)stream>>>(c, step_scalars, clip_coef, grad_scale, guard, decoupled);
                RG_RETURN_IF_LAUNCH_FAILED();
            }
            return RG_OK;
        });
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
