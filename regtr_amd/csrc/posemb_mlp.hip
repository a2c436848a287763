// pe = L5(relu(L4(relu(L3(relu(L2(relu(L1(xyz)))))))))     PositionEmbeddingLearned.forward (position_embedding.py:53-72)
//
// The learned positional embedding: a five-Linear ReLU MLP 3 -> 32 -> 64 -> 128 -> 256 -> d_model over the coarse key points, in ONE
// launch.  A workgroup (4 waves) owns a tile of 32 rows; the four hidden activations live in two LDS buffers that the layers ping-pong
// between (A: h1 and h3, B: h2 and h4 -- 32 x (129 + 257) floats = 48.3 KB, so three workgroups fit a CU) and never reach memory unless
// the caller asks for them (`acts`, what the backward reads).  Only pe (n, d_model) is written.
//
// Arithmetic: float32 with float32's operand range.  L1 (K = 3) is three vector FMAs per element; L2..L5 run on the exact-f32 MFMA
// (v_mfma_f32_32x32x2_f32): per output element ONE fmaf chain in k order from zero, then + bias, then the ReLU -- the arithmetic of
// regtr_gemm_f32 without split-K, so a row's result is a function of that row's xyz and the weights only (not of n, of the row's
// position in its tile, or of `acts`).  No f16 pair, no 16-bit operand: nothing normalises xyz or these activations.
//
// Operands: A[row = lane & 31][k = lane >> 5] from LDS (odd row strides: the 32 rows of a k hit 32 banks); B[k][col = lane & 31]
// straight from the (K, N)-layout weights in global memory -- a 32-row tile is one MFMA tall, so a B value is used by exactly one
// MFMA of one wave and LDS staging would add a pass without any reuse.  The weights (434 KB at d_model 256) are L2 resident and read by
// every workgroup; each lane's loads of a 32-deep k batch are issued one batch (16 or 32 MFMAs, 1-2 k cycles) ahead of their use.
// A wave owns column tiles of 32 (L2, L3) or pairs of them (L4, L5: two independent accumulators on one A read).
// The ReLU is `v < 0 ? 0 : v`: a NaN stays a NaN, as in torch (fmaxf would return 0).
#include "common.h"
#include "mfma_operands.h"

namespace {

constexpr int PM_ROWS = 32;
constexpr int PM_LDA = 128 + 1;      // buffer A row stride (h1: 32 wide, h3: 128 wide)
constexpr int PM_LDB = 256 + 1;      // buffer B row stride (h2: 64 wide, h4: 256 wide)
constexpr int PM_ACTS = 480;         // 32 + 64 + 128 + 256: the row width of `acts`

struct PosembArgs {
    const float* xyz; const float* w[5]; const float* b[5];
    float* pe; float* acts;
    int n, d_model;
};

// out[32][N] = act(in[32][K] W[K][N] + bias) for this workgroup's tile.  lds_out (row stride ld_out): where the next layer reads it, or
// nullptr; g_out (row stride ld_g, pointing at the tile's first row and this layer's first column): the copy in memory, or nullptr;
// rows_valid: the rows of the tile that exist (the others are computed from a clamped row and never stored to memory).
template <int K, int NT, bool RELU>
__device__ __forceinline__ void pm_layer(const float* in, int ld_in, const float* __restrict__ W, const float* __restrict__ bias, int N,
                                         float* lds_out, int ld_out, float* __restrict__ g_out, int ld_g, int rows_valid)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
    const float* a = in + l31 * ld_in + hi;
    for (int g = wave; g < N / (32 * NT); g += 4) {
        const int c0 = g * 32 * NT;
        const float* bp = W + (size_t)hi * N + c0 + l31;
        floatx16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
        float bc[NT][16], bn[NT][16];
#pragma unroll
        for (int s = 0; s < 16; s++)
#pragma unroll
            for (int t = 0; t < NT; t++) bc[t][s] = bp[(size_t)(2 * s) * N + 32 * t];
#pragma unroll
        for (int k0 = 0; k0 < K; k0 += 32) {
            if (k0 + 32 < K) {
#pragma unroll
                for (int s = 0; s < 16; s++)
#pragma unroll
                    for (int t = 0; t < NT; t++) bn[t][s] = bp[(size_t)(k0 + 32 + 2 * s) * N + 32 * t];
            }
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const float av = a[k0 + 2 * s];
#pragma unroll
                for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bc[t][s], acc[t], 0, 0, 0);
            }
            if (k0 + 32 < K) {
#pragma unroll
                for (int s = 0; s < 16; s++)
#pragma unroll
                    for (int t = 0; t < NT; t++) bc[t][s] = bn[t][s];
            }
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const int col = c0 + 32 * t + l31;
            const float bv = bias[col];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
                float v = acc[t][r] + bv;
                if (RELU) v = v < 0.f ? 0.f : v;
                if (lds_out) lds_out[row * ld_out + col] = v;
                if (g_out && row < rows_valid) g_out[(size_t)row * ld_g + col] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_posemb_mlp(PosembArgs p)
{
    __shared__ float bufA[PM_ROWS * PM_LDA];
    __shared__ float bufB[PM_ROWS * PM_LDB];
    const int t = threadIdx.x;
    const size_t m0 = (size_t)blockIdx.x * PM_ROWS;
    const int rows_valid = (int)min((size_t)PM_ROWS, (size_t)p.n - m0);
    float* acts = p.acts ? p.acts + m0 * PM_ACTS : nullptr;

    // L1: 3 -> 32 on the vector unit, the fmaf chain of a K = 3 exact-f32 GEMM (xyz rows are 12 bytes: scalar loads)
#pragma unroll
    for (int i = 0; i < PM_ROWS * 32 / 256; i++) {
        const int e = t + 256 * i, row = e >> 5, col = e & 31;
        const float* x = p.xyz + 3 * (m0 + min(row, rows_valid - 1));
        float v = fmaf(x[2], p.w[0][64 + col], fmaf(x[1], p.w[0][32 + col], x[0] * p.w[0][col])) + p.b[0][col];
        v = v < 0.f ? 0.f : v;
        bufA[row * PM_LDA + col] = v;
        if (acts && row < rows_valid) acts[(size_t)row * PM_ACTS + col] = v;
    }
    __syncthreads();
    pm_layer<32, 1, true>(bufA, PM_LDA, p.w[1], p.b[1], 64, bufB, PM_LDB, acts ? acts + 32 : nullptr, PM_ACTS, rows_valid);
    __syncthreads();
    pm_layer<64, 1, true>(bufB, PM_LDB, p.w[2], p.b[2], 128, bufA, PM_LDA, acts ? acts + 96 : nullptr, PM_ACTS, rows_valid);
    __syncthreads();
    pm_layer<128, 2, true>(bufA, PM_LDA, p.w[3], p.b[3], 256, bufB, PM_LDB, acts ? acts + 224 : nullptr, PM_ACTS, rows_valid);
    __syncthreads();
    pm_layer<256, 2, false>(bufB, PM_LDB, p.w[4], p.b[4], p.d_model, nullptr, 0, p.pe + m0 * p.d_model, p.d_model, rows_valid);
}

}  // namespace

extern "C" {

// w_kn / bias: HOST arrays of the five layers' device pointers, the weights in (K, N) layout -- (3, 32), (32, 64), (64, 128), (128, 256),
// (256, d_model).  acts (optional): (n, 480) = h1 | h2 | h3 | h4, the activations after their ReLUs.
int regtr_posemb_mlp(const float* xyz, int n, const float* const* w_kn, const float* const* bias, int d_model, float* pe, float* acts,
                     void* stream)
{
    if (n < 0 || d_model < 64 || d_model > 512 || d_model % 64 != 0 || !w_kn || !bias) return RG_ERR_ARG;
    PosembArgs p;
    for (int l = 0; l < 5; l++) {
        if (!w_kn[l] || !bias[l] || (uintptr_t)w_kn[l] % 16 != 0 || (uintptr_t)bias[l] % 16 != 0) return RG_ERR_ARG;
        p.w[l] = w_kn[l];
        p.b[l] = bias[l];
    }
    if ((uintptr_t)pe % 16 != 0 || (uintptr_t)acts % 16 != 0 || (uintptr_t)xyz % 4 != 0) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    if (!xyz || !pe) return RG_ERR_ARG;
    p.xyz = xyz; p.pe = pe; p.acts = acts; p.n = n; p.d_model = d_model;
    k_posemb_mlp<<<rg_cdiv(n, PM_ROWS), 256, 0, (hipStream_t)stream>>>(p);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
