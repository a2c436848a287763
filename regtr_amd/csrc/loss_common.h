// Device helpers shared by the feature-loss kernels (losses.hip: InfoNCE, circle_loss.hip: circle loss): the ragged-pair bounds check,
// the pose transform and the float32 coordinate distance that decides "inside r_p" / "outside r_n".  One copy, so that both losses
// classify a point pair identically.  Every step is an explicitly rounded intrinsic: no contraction whatever the compile flags.
#pragma once
#include <math.h>

#include "common.h"

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2)
{
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) { s = s + s2; m = M; return; }          // both empty (s = s2 = 0)
    s = s * expf(m - M) + s2 * expf(m2 - M);
    m = M;
}

__device__ __forceinline__ void transform_rn(const float* T, float x, float y, float z, float out[3])
{
#pragma unroll
    for (int r = 0; r < 3; r++)
        out[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4 * r], x), __fmul_rn(T[4 * r + 1], y)), __fmul_rn(T[4 * r + 2], z)), T[4 * r + 3]);
}

// d = sqrt_rn((dx^2 + dy^2) + dz^2), the differences taken anchor - positive
__device__ __forceinline__ float coord_dist_rn(float ax, float ay, float az, float px, float py, float pz)
{
    const float dx = __fsub_rn(ax, px), dy = __fsub_rn(ay, py), dz = __fsub_rn(az, pz);
    return __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

__device__ __forceinline__ bool pair_ok(const int* off, int b, int n, int& lo, int& hi)
{
    lo = off[b];
    hi = off[b + 1];
    return 0 <= lo && lo <= hi && hi <= n;
}
