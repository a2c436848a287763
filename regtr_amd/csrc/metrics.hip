// Validation / test metrics on the device for gfx950: the registration errors of the reference's se3_compare (utils/se3_torch.py:93-105,
// models/generic_reg_model.py:197-209) and the RPMNet / DCP metrics of benchmark/benchmark_modelnet.py:33-90, the modified Chamfer
// distance included.
//
// regtr_nearest      -- for every query point of C packed ragged clouds the nearest point of the support cloud of the same index, in
//                       float32 rounded per operation so that a numpy float32 restatement reproduces it bit for bit
//                       (tests/metrics_ref.py):
//                         transformed point  ((r0 x + r1 y) + r2 z) + t per row (as regtr_se3_transform), when a pose is given
//                         d2 = (dx dx + dy dy) + dz dz,  d = q - s
//                         the minimum by a strict <, supports scanned in ascending index: the lowest index wins a tie, a NaN distance
//                         never wins, a query without a candidate below +inf gives +inf and index -1.
//                       Grid (query tiles, clouds), NR_THREADS lanes with NR_QPT queries each in registers (query tile NR_QTILE = 768: a
//                       717-point ModelNet cloud is ONE workgroup, so its support cloud is staged once).  The support cloud goes through
//                       LDS in tiles of NR_TILE points, transformed once at staging time, as float4 (x, y, z, 0): every lane of a wave
//                       reads the SAME 16-byte slot, one broadcast LDS read without bank conflicts (ds_read_b96: the compiler drops
//                       the unused fourth word), and that read feeds NR_QPT distance evaluations.  A cloud longer than the tile (3DMatch's 22 k points x 16 bytes exceed the LDS) loops over tiles in
//                       ascending order, which keeps the tie rule.  32 KiB of static LDS: two workgroups share a CU's 160 KiB with room to
//                       spare, and no launch attribute has to be raised.
// regtr_segment_mean -- per-cloud mean of a float32 vector as float64: a strided float64 partial per lane (rows ascending), the fixed xor
//                       tree, the waves in order -- regtr_cloud_centroids' convention.  One workgroup per cloud.
// regtr_pose_metrics -- one thread per (layer, pair), everything in float64, sums left to right:
//                         [0] rot_err_deg, [1] trans_err of pred o gt^-1 = [Rp Rg^T | tp - Rp Rg^T tg]      (se3_compare)
//                         [2] err_r_deg,   [3] err_t     of gt^-1 o pred = [Rg^T Rp | Rg^T (tp - tg)]       (benchmark_modelnet.py:63-67)
//                         [4] t_mse, [5] t_mae over the three translation components                         (:57-60)
//                         [6] r_mse, [7] r_mae over the extrinsic-xyz Euler angles in degrees                (:52-58), closed form
//                             a = atan2(R21, R22), b = -asin(clamp(R20, -1, 1)), c = atan2(R10, R00)         (R = Rz(c) Ry(b) Rx(a))
//                       and the composed transform pred o gt^-1 rounded to float32 (the Chamfer term applies it to the raw cloud, :72).
//                       At gimbal lock (|R20| within rounding of 1) scipy switches to a convention of its own (third angle 0), which is
//                       NOT reproduced: a and c then come from atan2 of rounding noise.  The output stays finite.
//
// No floating-point atomics, no host wait, no grid barrier: every launch is independent and its result a function of its inputs alone.
// Compiled with -ffp-contract=off (regtr_amd/build.py).
#include "augment_common.h"      // transform_rn: the float32 rigid transform rounded per operation

namespace {

constexpr int NR_THREADS = 256;
constexpr int NR_QPT = 3;
constexpr int NR_QTILE = NR_THREADS * NR_QPT;      // 768 (regtr_amd/ops.py: NEAREST_QUERY_TILE)
constexpr int NR_TILE = 2048;                       // supports per LDS tile: 32 KiB as float4

__global__ __launch_bounds__(NR_THREADS) void k_nearest(const float* __restrict__ q_xyz, const int* __restrict__ q_off, int n_q,
                                                        const float* __restrict__ s_xyz, const int* __restrict__ s_off, int n_s,
                                                        const float* __restrict__ q_pose, const float* __restrict__ s_pose,
                                                        float* __restrict__ d2_out, int* __restrict__ idx_out)
{
    __shared__ float4 sh[NR_TILE];
    const int c = blockIdx.y, tid = threadIdx.x;
    const int qlo = min(max(q_off[c], 0), n_q), qhi = min(max(q_off[c + 1], qlo), n_q);
    const int q0 = qlo + (int)blockIdx.x * NR_QTILE;
    if (q0 >= qhi) return;                                                     // (block-uniform) no query of this cloud in this tile
    const int slo = min(max(s_off[c], 0), n_s), shi = min(max(s_off[c + 1], slo), n_s);

    float Tq[12], Ts[12];
    if (q_pose) {
#pragma unroll
        for (int e = 0; e < 12; e++) Tq[e] = q_pose[12 * (size_t)c + e];
    }
    if (s_pose) {
#pragma unroll
        for (int e = 0; e < 12; e++) Ts[e] = s_pose[12 * (size_t)c + e];
    }

    float qx[NR_QPT], qy[NR_QPT], qz[NR_QPT], best[NR_QPT];
    int bi[NR_QPT];
#pragma unroll
    for (int k = 0; k < NR_QPT; k++) {
        const int q = q0 + k * NR_THREADS + tid;
        float p[3] = {0.f, 0.f, 0.f};
        if (q < qhi) {
            p[0] = q_xyz[3 * (size_t)q]; p[1] = q_xyz[3 * (size_t)q + 1]; p[2] = q_xyz[3 * (size_t)q + 2];
            if (q_pose) {
                float o[3];
                transform_rn(Tq, p[0], p[1], p[2], o);
                p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
            }
        }
        qx[k] = p[0]; qy[k] = p[1]; qz[k] = p[2];
        best[k] = __builtin_huge_valf();
        bi[k] = -1;
    }

    for (int j0 = slo; j0 < shi; j0 += NR_TILE) {                             // tiles in ascending order: the lowest index wins a tie
        const int m = min(NR_TILE, shi - j0);
        __syncthreads();                                                       // the previous tile has been read by every wave
        for (int i = tid; i < m; i += NR_THREADS) {
            const size_t r = (size_t)(j0 + i);
            float p[3] = {s_xyz[3 * r], s_xyz[3 * r + 1], s_xyz[3 * r + 2]};
            if (s_pose) {
                float o[3];
                transform_rn(Ts, p[0], p[1], p[2], o);
                p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
            }
            sh[i] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        const int base = j0 - slo;
#pragma unroll 4
        for (int i = 0; i < m; i++) {
            const float4 s = sh[i];                                            // wave-uniform address: one broadcast read of the slot
#pragma unroll
            for (int k = 0; k < NR_QPT; k++) {
                const float dx = __fsub_rn(qx[k], s.x), dy = __fsub_rn(qy[k], s.y), dz = __fsub_rn(qz[k], s.z);
                const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                if (d < best[k]) { best[k] = d; bi[k] = base + i; }            // strict: NaN never wins, the first of equals stays
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NR_QPT; k++) {
        const int q = q0 + k * NR_THREADS + tid;
        if (q < qhi) {
            d2_out[q] = best[k];
            if (idx_out) idx_out[q] = bi[k];
        }
    }
}

constexpr int SM_THREADS = 256;

__global__ __launch_bounds__(SM_THREADS) void k_segment_mean(const float* __restrict__ v, const int* __restrict__ off, int n,
                                                             double* __restrict__ out)
{
    __shared__ double sh[SM_THREADS / RG_WAVE];
    const int c = blockIdx.x;
    const int lo = min(max(off[c], 0), n), hi = min(max(off[c + 1], lo), n);
    double s = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += SM_THREADS) s += (double)v[i];       // a lane's rows in ascending order
    s = rg_wave_sum(s);                                                                   // fixed xor tree
    if (rg_lane() == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < SM_THREADS / RG_WAVE; w++) t += sh[w];                        // waves in order
        out[c] = hi > lo ? t / (double)(hi - lo) : 0.0;
    }
}

__device__ __forceinline__ double clamp1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }      // (a NaN stays a NaN)

__device__ __forceinline__ void euler_xyz_deg(const double* R, double* e)                // R row-major 3x3
{
    const double k = 180.0 / 3.14159265358979323846;
    e[0] = atan2(R[7], R[8]) * k;
    e[1] = -asin(clamp1(R[6])) * k;
    e[2] = atan2(R[3], R[0]) * k;
}

__global__ __launch_bounds__(64) void k_pose_metrics(const float* __restrict__ pred, const float* __restrict__ gt, int gt_stride, int n_layers, int n_pairs,
                               double* __restrict__ out, float* __restrict__ composed)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_layers * n_pairs) return;
    const int b = g % n_pairs;
    const double k = 180.0 / 3.14159265358979323846;
    double Rp[9], tp[3], Rg[9], tg[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            Rp[3 * i + j] = (double)pred[12 * (size_t)g + 4 * i + j];
            Rg[3 * i + j] = (double)gt[(size_t)gt_stride * b + 4 * i + j];
        }
        tp[i] = (double)pred[12 * (size_t)g + 4 * i + 3];
        tg[i] = (double)gt[(size_t)gt_stride * b + 4 * i + 3];
    }
    // pred o gt^-1 = [Rp Rg^T | tp - (Rp Rg^T) tg]
    double Rc[9], tc[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Rc[3 * i + j] = (Rp[3 * i] * Rg[3 * j] + Rp[3 * i + 1] * Rg[3 * j + 1]) + Rp[3 * i + 2] * Rg[3 * j + 2];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) tc[i] = tp[i] - ((Rc[3 * i] * tg[0] + Rc[3 * i + 1] * tg[1]) + Rc[3 * i + 2] * tg[2]);
    double* o = out + 8 * (size_t)g;
    o[0] = acos(clamp1(0.5 * (((Rc[0] + Rc[4]) + Rc[8]) - 1.0))) * k;
    o[1] = sqrt((tc[0] * tc[0] + tc[1] * tc[1]) + tc[2] * tc[2]);
    // gt^-1 o pred = [Rg^T Rp | Rg^T (tp - tg)]: its trace, its translation
    double tr = 0.0, dt[3], ti[3];
#pragma unroll
    for (int i = 0; i < 3; i++) tr = tr + ((Rg[i] * Rp[i] + Rg[3 + i] * Rp[3 + i]) + Rg[6 + i] * Rp[6 + i]);
#pragma unroll
    for (int i = 0; i < 3; i++) dt[i] = tp[i] - tg[i];
#pragma unroll
    for (int i = 0; i < 3; i++) ti[i] = (Rg[i] * dt[0] + Rg[3 + i] * dt[1]) + Rg[6 + i] * dt[2];
    o[2] = acos(clamp1(0.5 * (tr - 1.0))) * k;
    o[3] = sqrt((ti[0] * ti[0] + ti[1] * ti[1]) + ti[2] * ti[2]);
    o[4] = ((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]) / 3.0;
    o[5] = ((fabs(dt[0]) + fabs(dt[1])) + fabs(dt[2])) / 3.0;
    double eg[3], ep[3], de[3];
    euler_xyz_deg(Rg, eg);
    euler_xyz_deg(Rp, ep);
#pragma unroll
    for (int i = 0; i < 3; i++) de[i] = eg[i] - ep[i];
    o[6] = ((de[0] * de[0] + de[1] * de[1]) + de[2] * de[2]) / 3.0;
    o[7] = ((fabs(de[0]) + fabs(de[1])) + fabs(de[2])) / 3.0;
    float* cm = composed + 12 * (size_t)g;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) cm[4 * i + j] = (float)Rc[3 * i + j];
        cm[4 * i + 3] = (float)tc[i];
    }
}

}  // namespace

extern "C" {

int regtr_nearest_lds_points(void) { return NR_TILE; }

int regtr_nearest(const float* q_xyz, const int* q_off, int n_q, const float* s_xyz, const int* s_off, int n_s, int n_clouds,
                  int max_q_len, const float* q_pose, const float* s_pose, float* d2, int* idx, void* stream)
{
    if (n_q < 0 || n_s < 0 || n_clouds < 0 || max_q_len < 0) return RG_ERR_ARG;
    if (n_q == 0 || n_clouds == 0 || max_q_len == 0) return RG_OK;
    if (n_clouds > 65535) return RG_ERR_ARG;                                   // (grid y)
    if (!q_xyz || !q_off || !s_off || !d2 || (n_s > 0 && !s_xyz)) return RG_ERR_ARG;
    const dim3 grid((unsigned)rg_cdiv(max_q_len, NR_QTILE), (unsigned)n_clouds);
    k_nearest<<<grid, NR_THREADS, 0, (hipStream_t)stream>>>(q_xyz, q_off, n_q, s_xyz, s_off, n_s, q_pose, s_pose, d2, idx);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_segment_mean(const float* v, const int* off, int n_clouds, int n, double* out, void* stream)
{
    if (n_clouds < 0 || n < 0) return RG_ERR_ARG;
    if (n_clouds == 0) return RG_OK;
    if (!off || !out || (n > 0 && !v)) return RG_ERR_ARG;
    k_segment_mean<<<n_clouds, SM_THREADS, 0, (hipStream_t)stream>>>(v, off, n, out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_pose_metrics(const float* pred, const float* gt, int gt_stride, int n_layers, int n_pairs, double* out, float* composed,
                       void* stream)
{
    if (n_layers < 0 || n_pairs < 0 || (gt_stride != 12 && gt_stride != 16)) return RG_ERR_ARG;
    const long long n = (long long)n_layers * n_pairs;
    if (n == 0) return RG_OK;
    if (n >= (1ll << 27)) return RG_ERR_ARG;
    if (!pred || !gt || !out || !composed) return RG_ERR_ARG;
    k_pose_metrics<<<rg_cdiv(n, 64), 64, 0, (hipStream_t)stream>>>(pred, gt, gt_stride, n_layers, n_pairs, out, composed);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
