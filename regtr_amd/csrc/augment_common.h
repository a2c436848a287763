// What the two training-augmentation sources (augment.hip: the 3DMatch chain, augment_modelnet.hip: the ModelNet chain) share: the
// counter-based random numbers and the float32 rigid-transform arithmetic, rounded per operation.  Both sources are compiled with
// -ffp-contract=off (regtr_amd/build.py).
//
// RANDOM NUMBERS -- one convention for both chains:
//   Philox4x32-10 (Salmon et al., SC'11) with
//     key     = (seed & 0xffffffff, seed >> 32)
//     counter = (index, cloud_or_pair, purpose, step)
//   a uniform is u = ((x >> 8) + 0.5) 2^-24 of one output word x, so 0 < u < 1; normals are Box-Muller pairs of two uniforms,
//   z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2), words (x0, x1) -> (z0, z1), (x2, x3) -> (z2, z3).
//   purpose 0-2: augment.hip; purpose 3-7: augment_modelnet.hip.  Each file states which word feeds which decision.
#pragma once
#include <math.h>

#include "common.h"

namespace {

struct Philox4 { uint32_t x[4]; };

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox4 o;
    o.x[0] = c0; o.x[1] = c1; o.x[2] = c2; o.x[3] = c3;
    return o;
}

__device__ __forceinline__ double uniform_d(uint32_t x) { return ((double)(x >> 8) + 0.5) * (1.0 / 16777216.0); }

__device__ __forceinline__ void box_muller_d(uint32_t xa, uint32_t xb, double& z0, double& z1)
{
    const double r = sqrt(-2.0 * log(uniform_d(xa)));
    double s, c;
    sincos(6.283185307179586476925 * uniform_d(xb), &s, &c);
    z0 = r * c; z1 = r * s;
}

// float32 Box-Muller of the jitter.  ln u is taken where it is accurate: k + 0.5 is a float32 number only for k < 2^23, so the upper half
// of the range goes through u = 1 - v, v = (2^24 - k - 0.5) 2^-24 (exact in float32), ln u = log1p(-v): a rounded u there would come out
// as 1 for the largest k and lose the whole radius.  The angle's uniform is rounded to float32 (2^-25 relative).
__device__ __forceinline__ void box_muller_f(uint32_t xa, uint32_t xb, float& z0, float& z1)
{
    const uint32_t k = xa >> 8;
    const float ln = k < (1u << 23) ? logf(((float)k + 0.5f) * (1.0f / 16777216.0f))
                                    : log1pf(-(((float)((1u << 24) - k) - 0.5f) * (1.0f / 16777216.0f)));
    const float r = sqrtf(-2.0f * ln);
    const float u2 = (float)(((double)(xb >> 8) + 0.5) * (1.0 / 16777216.0));
    float s, c;
    sincosf(6.2831853071795864769f * u2, &s, &c);
    z0 = r * c; z1 = r * s;
}

// ---- 3x4 rigid transforms in float32, rounded per operation, sums left to right (row-major T[12] = [R | t])
__device__ __forceinline__ float dot3_rn(float a0, float a1, float a2, float b0, float b1, float b2)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
}

__device__ __forceinline__ void se3_cat_rn(const float* a, const float* b, float* o)          // se3_torch.py:32-40
{
    float t[12];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) t[4 * i + j] = dot3_rn(a[4 * i], a[4 * i + 1], a[4 * i + 2], b[j], b[4 + j], b[8 + j]);
        t[4 * i + 3] = __fadd_rn(dot3_rn(a[4 * i], a[4 * i + 1], a[4 * i + 2], b[3], b[7], b[11]), a[4 * i + 3]);
    }
#pragma unroll
    for (int e = 0; e < 12; e++) o[e] = t[e];
}

__device__ __forceinline__ void se3_inv_rn(const float* a, float* o)                          // se3_torch.py:43-48: [R^T | (-R^T) t]
{
    float t[12];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) t[4 * i + j] = a[4 * j + i];
        t[4 * i + 3] = dot3_rn(-a[i], -a[4 + i], -a[8 + i], a[3], a[7], a[11]);
    }
#pragma unroll
    for (int e = 0; e < 12; e++) o[e] = t[e];
}

__device__ __forceinline__ void transform_rn(const float* T, float x, float y, float z, float out[3])     // as regtr_se3_transform
{
#pragma unroll
    for (int r = 0; r < 3; r++)
        out[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4 * r], x), __fmul_rn(T[4 * r + 1], y)), __fmul_rn(T[4 * r + 2], z)), T[4 * r + 3]);
}

}  // namespace
