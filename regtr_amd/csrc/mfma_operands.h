// The 16-bit operand formats of the matrix-core kernels (gemm_x3.hip, gemm_stream.hip, block_tail.hip, attention.hip; gemm.hip shares the
// accumulator type): float32-grade products rest on two exact splits of a float32 value, and every kernel and every weight-plane
// buffer has to agree on them, so they are defined here and nowhere else.  tests/test_f16_pair_model.py models the f16 pair on the CPU.
//
//   bf16 planes (NP = 1 | 2 | 3):  x = x0 + x1 + x2 exactly,  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)  (8 significant bits
//     each; every bf16 x bf16 product is exact in f32).  NP = 3 is float32-grade with six MFMA terms, NP = 2 keeps the three leading terms
//     (relative error ~2^-16 per product), NP = 1 is plain bf16.  Finite inputs only: an infinite operand splits into Inf + NaN.
//   f16 pair:  x = h0 + h1 / RG_F16_SCALE,  h0 = f16(x), h1 = f16((x - h0) * RG_F16_SCALE) -- 22 mantissa bits in TWO planes where the bf16
//     split needs three for 24.  A product is a0 w0 + (a0 w1 + a1 w0) / 2048 + O(2^-22 |a w|): THREE v_mfma_f32_32x32x16_f16 instead of six
//     bf16 ones, the two low terms in a second accumulator that is scaled once where it is read (rg_fold_low).  The scale keeps the low
//     plane out of f16's subnormal range, where an unscaled residual of anything below 0.12 would sit.  Range: |x| < 65504 (f16); values
//     below 6.1e-5 have a subnormal (coarse) h0 whose rounding the scaled h1 picks up again.
#pragma once
#include "common.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));       // accumulator of a 32x32 MFMA
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));         // one MFMA operand fragment (eight f16 travel in it too: the type only carries the bits)
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* rg_lds_ptr;        // destination of __builtin_amdgcn_global_load_lds

constexpr float RG_F16_SCALE = 2048.f;

// Weight planes are Wt[plane][Npad][Kp] 16-bit values, k contiguous, zero padded: columns to 128 (the widest tile), k to a 32-wide k-tile
struct RgPlaneDims { int Npad, Kp; size_t elems() const { return (size_t)Npad * Kp; } };
static inline RgPlaneDims rg_plane_dims(int N, int K) { return {rg_cdiv(N, 128) * 128, rg_cdiv(K, 32) * 32}; }

__device__ __forceinline__ unsigned rg_pack_bf16(float a, float b)
{
    bf16x2 v;
    v.x = (__bf16)a; v.y = (__bf16)b;            // v_cvt_pk_bf16_f32, round to nearest even
    return __builtin_bit_cast(unsigned, v);
}

__device__ __forceinline__ unsigned rg_pack_f16(float a, float b)
{
    f16x2 v;
    v.x = (_Float16)a; v.y = (_Float16)b;
    return __builtin_bit_cast(unsigned, v);
}

// (a, b) -> three packed bf16 pairs, one per plane: a = a0 + a1 + a2 exactly (likewise b)
__device__ __forceinline__ void rg_split2(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2)
{
    p0 = rg_pack_bf16(a, b);
    const float ra = a - __uint_as_float(p0 << 16), rb = b - __uint_as_float(p0 & 0xffff0000u);
    p1 = rg_pack_bf16(ra, rb);
    p2 = rg_pack_bf16(ra - __uint_as_float(p1 << 16), rb - __uint_as_float(p1 & 0xffff0000u));
}
// (a, b) -> the two packed planes of the f16 pair
__device__ __forceinline__ void rg_split2_f16(float a, float b, unsigned& p0, unsigned& p1)
{
    p0 = rg_pack_f16(a, b);
    const f16x2 h = __builtin_bit_cast(f16x2, p0);
    p1 = rg_pack_f16((a - (float)h.x) * RG_F16_SCALE, (b - (float)h.y) * RG_F16_SCALE);
}
// the same into an array of planes: the leading NP of the three bf16 planes (the rest is dead code), or with F16 the f16 pair
template <int NP, bool F16 = false>
__device__ __forceinline__ void rg_split2(float a, float b, unsigned (&p)[NP])
{
    static_assert(NP >= 1 && NP <= 3 && (!F16 || NP == 2), "one to three bf16 planes; the f16 pair has two");
    unsigned unused;
    if constexpr (F16) rg_split2_f16(a, b, p[0], p[1]);
    else rg_split2(a, b, p[0], NP > 1 ? p[1] : unused, NP > 2 ? p[2] : unused);
}

// f16 pair: fold the scaled low accumulator into the high one.  Returns chk with one FMA per value folded in: x * 0 is 0 for a finite x and
// NaN otherwise, so after the last fold chk tells whether any product came out non-finite (rg_report_range).
__device__ __forceinline__ float rg_fold_low(floatx16& acc, const floatx16& lo, float chk = 0.f)
{
#pragma unroll
    for (int r = 0; r < 16; r++) { acc[r] += lo[r] * (1.0f / RG_F16_SCALE); chk = fmaf(acc[r], 0.f, chk); }
    return chk;
}
// f16 pair: an operand at or beyond f16's range converts to +-Inf and its residual plane to NaN, so every product of that row (or
// column) is non-finite -- the raw accumulators tell.  live: whether this wave's values are results at all (a reference: passed by value,
// hipcc combines the two scalar conditions in another order than the kernels were measured with).
__device__ __forceinline__ void rg_report_range(int* status, float chk, const bool& live = true)
{
    if (status && live && chk != chk) atomicOr(status, REGTR_STATUS_F16_RANGE);
}

}  // namespace
