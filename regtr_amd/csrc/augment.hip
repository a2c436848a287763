// The reference's 3DMatch training augmentation (data_loaders/__init__.py:18-23: RigidPerturb -> Jitter -> ShufflePoints -> RandomSwap,
// data_loaders/transforms.py) on packed device batches for gfx950, reproducible from (seed, step) with no host round trip.
//
// RANDOM NUMBERS -- one convention, restated in tests/augment_ref.py and regtr_amd/augment.py:
//   Philox4x32-10 (Salmon et al., SC'11) with
//     key     = (seed & 0xffffffff, seed >> 32)
//     counter = (index, cloud_or_pair, purpose, step)         purpose 0: pair draws, 1: shuffle keys, 2: jitter
//   a uniform is u = ((x >> 8) + 0.5) 2^-24 of one output word x, so 0 < u < 1; normals are Box-Muller pairs of two uniforms,
//   z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2), words (x0, x1) -> (z0, z1), (x2, x3) -> (z2, z3).
//   Pair draws of pair b (purpose 0), index = block:
//     block 0: x0, x1, x2 -> the perturbation's uniforms   small: phi = 2 pi u0, cos(theta) = 2 u1 - 1;  large: zyx Euler angles 2 pi u0..2
//     block 1: z0 -> the angle's normal, z1 z2 z3 -> the translation's normals (small only)
//     block 2: x0 -> perturb_source = u > 0.5, x1 -> swap = u > 0.5
//   Shuffle key of input row r of input cloud slot c (purpose 1): word x0 of counter (r, c, 1, step).
//   Jitter of OUTPUT row i of OUTPUT cloud slot c' (purpose 2): z0 z1 z2 of counter (i, c', 2, step).
//
// regtr_cloud_centroids  -- per-cloud mean, float64 sums in a fixed order (strided partial per lane, fixed tree), bit-reproducible.
// regtr_augment_draws    -- one thread per pair: the perturbation P (float64 trigonometry, rounded once to float32 as the reference's
//                           `.float()` does), its recentring about the centroid, the new ground-truth pose and the per-cloud transforms,
//                           composed in float32 rounded per operation in the reference's order (transforms.py:48-66,148, se3_torch.py:32-48).
// regtr_shuffle_keys     -- (cloud_slot << 32) | philox word per input row; the permutation is their stable ascending sort (the caller's
//                           radix sort), cloud c's output rows the first min(n_c, max_pts) of its sorted segment (ShufflePoints).
// regtr_augment_gather   -- the one pass over the points: gather, transform (rounded per operation like regtr_se3_transform), jitter, mask.
//
// No floating-point atomics, grid barriers, cooperative launches or spin-waits: every launch is independent, the stream orders them.
// Compiled with -ffp-contract=off (regtr_amd/build.py): the transforms are specified as rounded per operation.
#include "augment_common.h"      // Philox4x32-10, Box-Muller, the *_rn float32 transforms (shared with augment_modelnet.hip)

namespace {

constexpr int AUG_THREADS = 256;

// ---------------------------------------------------------------------------------------------------------------- centroids
__global__ __launch_bounds__(AUG_THREADS) void k_cloud_centroids(const float* __restrict__ xyz, const int* __restrict__ seg_off, int n,
                                                                 float* __restrict__ out)
{
    __shared__ double sh[3 * AUG_THREADS / RG_WAVE];
    const int c = blockIdx.x;
    int lo = seg_off[c], hi = seg_off[c + 1];
    lo = max(lo, 0); hi = min(hi, n);
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = lo + (int)threadIdx.x; i < hi; i += AUG_THREADS) {          // a lane's rows in ascending order
        s[0] += (double)xyz[3 * (size_t)i]; s[1] += (double)xyz[3 * (size_t)i + 1]; s[2] += (double)xyz[3 * (size_t)i + 2];
    }
#pragma unroll
    for (int d = 0; d < 3; d++) s[d] = rg_wave_sum(s[d]);                  // fixed xor tree
    if (rg_lane() == 0) {
#pragma unroll
        for (int d = 0; d < 3; d++) sh[3 * (threadIdx.x >> 6) + d] = s[d];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < AUG_THREADS / RG_WAVE; w++) t += sh[3 * w + threadIdx.x];      // waves in order
        out[3 * c + threadIdx.x] = hi > lo ? (float)(t / (double)(hi - lo)) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- pair draws
__global__ void k_augment_draws(const float* __restrict__ pose, int pose_stride, const float* __restrict__ centroids, int n_pairs,
                                uint32_t k0, uint32_t k1, uint32_t step, int mode, float std_, int do_swap, float* __restrict__ xform,
                                float* __restrict__ pose_out, int* __restrict__ flags)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_pairs) return;
    float G[12], P[12];
    const float I[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
#pragma unroll
    for (int e = 0; e < 12; e++) { G[e] = pose[(size_t)b * pose_stride + e]; P[e] = I[e]; }
    const Philox4 f = philox4x32_10(2u, (uint32_t)b, 0u, step, k0, k1);
    const int perturb_source = mode != 0 && (f.x[0] >> 8) >= (1u << 23);      // u > 0.5
    const int swap = do_swap && (f.x[1] >> 8) >= (1u << 23);

    if (mode != 0) {
        const Philox4 q = philox4x32_10(0u, (uint32_t)b, 0u, step, k0, k1);
        const double two_pi = 6.283185307179586476925;
        double R[9], t[3] = {0.0, 0.0, 0.0};
        if (mode == 1) {                                                      // small: so3.py:31-38,82-101, se3.py:38-44
            const Philox4 g = philox4x32_10(1u, (uint32_t)b, 0u, step, k0, k1);
            double z[4];
            box_muller_d(g.x[0], g.x[1], z[0], z[1]);
            box_muller_d(g.x[2], g.x[3], z[2], z[3]);
            const double phi = two_pi * uniform_d(q.x[0]), cth = 2.0 * uniform_d(q.x[1]) - 1.0;
            const double th = acos(cth);
            const double ax[3] = {sin(th) * cos(phi), sin(th) * sin(phi), cos(th)};
            const double ang = z[0] * ((double)std_ * 3.14159265358979323846 / sqrt(3.0));
            const double om[3] = {ax[0] * ang, ax[1] * ang, ax[2] * ang};
            const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
            if (theta <= 1e-8) {                                              // np.isclose(theta, 0): first-order Taylor
                const double T[9] = {1.0, -om[2], om[1], om[2], 1.0, -om[0], -om[1], om[0], 1.0};
#pragma unroll
                for (int e = 0; e < 9; e++) R[e] = T[e];
            } else {
                const double w[3] = {om[0] / theta, om[1] / theta, om[2] / theta};
                const double H[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
                const double s = sin(theta), c1 = 1.0 - cos(theta);
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const double h2 = H[3 * i] * H[j] + H[3 * i + 1] * H[3 + j] + H[3 * i + 2] * H[6 + j];
                        R[3 * i + j] = (i == j ? 1.0 : 0.0) + s * H[3 * i + j] + c1 * h2;
                    }
            }
            const double ts = (double)std_ / sqrt(3.0);
            t[0] = z[1] * ts; t[1] = z[2] * ts; t[2] = z[3] * ts;
        } else {                                                              // large: Rotation.from_euler('zyx', [a, b, c]) = Rx(c) Ry(b) Rz(a)
            const double a = two_pi * uniform_d(q.x[0]), bb = two_pi * uniform_d(q.x[1]), c = two_pi * uniform_d(q.x[2]);
            const double ca = cos(a), sa = sin(a), cb = cos(bb), sb = sin(bb), cc = cos(c), sc = sin(c);
            R[0] = cb * ca;                  R[1] = -cb * sa;                 R[2] = sb;
            R[3] = sc * sb * ca + cc * sa;   R[4] = -sc * sb * sa + cc * ca;  R[5] = -sc * cb;
            R[6] = -cc * sb * ca + sc * sa;  R[7] = cc * sb * sa + sc * ca;   R[8] = cc * cb;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int j = 0; j < 3; j++) P[4 * i + j] = (float)R[3 * i + j];
            P[4 * i + 3] = (float)t[i];
        }
        if (mode == 1) {                                                      // transforms.py:48-54: P <- C^-1 P C, C = [I | -centroid]
            const float* cen = centroids + 3 * (size_t)(perturb_source ? b : n_pairs + b);
            const float C[12] = {1.f, 0.f, 0.f, -cen[0], 0.f, 1.f, 0.f, -cen[1], 0.f, 0.f, 1.f, -cen[2]};
            float Ci[12];
            se3_inv_rn(C, Ci);
            se3_cat_rn(Ci, P, P);
            se3_cat_rn(P, C, P);
        }
        if (perturb_source) {                                                 // :57  pose <- pose o P^-1
            float Pi[12];
            se3_inv_rn(P, Pi);
            se3_cat_rn(G, Pi, G);
        } else {                                                              // :65  pose <- P o pose
            se3_cat_rn(P, G, G);
        }
    }
    if (swap) se3_inv_rn(G, G);                                               // :148
    const int slot = perturb_source ? b : n_pairs + b, other = perturb_source ? n_pairs + b : b;
#pragma unroll
    for (int e = 0; e < 12; e++) {
        xform[12 * (size_t)slot + e] = P[e];
        xform[12 * (size_t)other + e] = I[e];
        pose_out[12 * (size_t)b + e] = G[e];
    }
    flags[2 * b] = perturb_source;
    flags[2 * b + 1] = swap;
}

// ---------------------------------------------------------------------------------------------------------------- shuffle keys
__global__ void k_shuffle_keys(const int* __restrict__ seg_off, int n_clouds, int n, uint32_t k0, uint32_t k1, uint32_t step,
                               long long* __restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = rg_find_segment(seg_off, n_clouds, i);
    const Philox4 r = philox4x32_10((uint32_t)(i - seg_off[c]), (uint32_t)c, 1u, step, k0, k1);
    keys[i] = (long long)(((uint64_t)(uint32_t)c << 32) | r.x[0]);
}

// ---------------------------------------------------------------------------------------------------------------- gather
__global__ void k_augment_gather(const float* __restrict__ xyz, const unsigned char* __restrict__ mask, const int* __restrict__ in_off,
                                 int n_in, const long long* __restrict__ perm, const int* __restrict__ out_off,
                                 const int* __restrict__ in_slot, int n_clouds, int n_out, const float* __restrict__ xform, float noise,
                                 uint32_t k0, uint32_t k1, uint32_t step, float* __restrict__ out_xyz, unsigned char* __restrict__ out_mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const int co = rg_find_segment(out_off, n_clouds, i);                     // output cloud slot
    const int j = i - out_off[co];                                            // output row within it
    int ci = in_slot[co];
    ci = min(max(ci, 0), n_clouds - 1);
    const int lo = max(in_off[ci], 0), hi = min(in_off[ci + 1], n_in);
    if (hi <= lo) return;                                                     // (an empty input cloud has no output rows)
    const int row = min(max(lo + j, lo), hi - 1);                             // offsets of another layout cannot leave the cloud ...
    long long src = perm ? perm[row] : (long long)row;
    src = src < lo ? lo : (src >= hi ? hi - 1 : src);                         // ... nor can a permutation of one
    float p[3] = {xyz[3 * (size_t)src], xyz[3 * (size_t)src + 1], xyz[3 * (size_t)src + 2]};
    if (xform) {
        float T[12], o[3];
#pragma unroll
        for (int e = 0; e < 12; e++) T[e] = xform[12 * (size_t)ci + e];
        transform_rn(T, p[0], p[1], p[2], o);
        p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
    }
    if (noise != 0.f) {                                                       // (no `+ 0 z`: it would turn -0 into +0)
        const Philox4 r = philox4x32_10((uint32_t)j, (uint32_t)co, 2u, step, k0, k1);
        float z[4];
        box_muller_f(r.x[0], r.x[1], z[0], z[1]);
        box_muller_f(r.x[2], r.x[3], z[2], z[3]);
#pragma unroll
        for (int d = 0; d < 3; d++) p[d] = __fadd_rn(p[d], __fmul_rn(noise, z[d]));
    }
    out_xyz[3 * (size_t)i] = p[0]; out_xyz[3 * (size_t)i + 1] = p[1]; out_xyz[3 * (size_t)i + 2] = p[2];
    if (out_mask) out_mask[i] = mask[src];
}

}  // namespace

extern "C" {

int regtr_cloud_centroids(const float* xyz, const int* seg_off, int n_clouds, int n, float* out, void* stream)
{
    if (n_clouds < 0 || n < 0) return RG_ERR_ARG;
    if (n_clouds == 0) return RG_OK;
    if (!seg_off || !out || (n > 0 && !xyz)) return RG_ERR_ARG;
    k_cloud_centroids<<<n_clouds, AUG_THREADS, 0, (hipStream_t)stream>>>(xyz, seg_off, n, out);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_augment_draws(const float* pose, int pose_stride, const float* centroids, int n_pairs, unsigned long long seed,
                        unsigned int step, int perturb_mode, float perturb_std, int swap, float* xform, float* pose_out, int* flags,
                        void* stream)
{
    if (n_pairs < 0 || (pose_stride != 12 && pose_stride != 16) || perturb_mode < 0 || perturb_mode > 2) return RG_ERR_ARG;
    if (perturb_mode == 1 && !(perturb_std >= 0.f)) return RG_ERR_ARG;
    if (n_pairs == 0) return RG_OK;
    if (!pose || !xform || !pose_out || !flags || (perturb_mode == 1 && !centroids)) return RG_ERR_ARG;
    k_augment_draws<<<rg_cdiv(n_pairs, 64), 64, 0, (hipStream_t)stream>>>(pose, pose_stride, centroids, n_pairs, (uint32_t)seed,
                                                                         (uint32_t)(seed >> 32), step, perturb_mode, perturb_std,
                                                                         swap != 0, xform, pose_out, flags);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_shuffle_keys(const int* seg_off, int n_clouds, int n, unsigned long long seed, unsigned int step, long long* keys,
                       void* stream)
{
    if (n_clouds < 0 || n < 0) return RG_ERR_ARG;
    if (n == 0) return RG_OK;
    if (!seg_off || !keys || n_clouds < 1) return RG_ERR_ARG;
    k_shuffle_keys<<<rg_cdiv(n, AUG_THREADS), AUG_THREADS, 0, (hipStream_t)stream>>>(seg_off, n_clouds, n, (uint32_t)seed,
                                                                                   (uint32_t)(seed >> 32), step, keys);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_augment_gather(const float* xyz, const unsigned char* mask, const int* in_off, int n_in, const long long* perm,
                         const int* out_off, const int* in_slot, int n_clouds, int n_out, const float* xform, float noise,
                         unsigned long long seed, unsigned int step, float* out_xyz, unsigned char* out_mask, void* stream)
{
    if (n_clouds < 0 || n_in < 0 || n_out < 0 || n_out > n_in || !(noise == noise)) return RG_ERR_ARG;
    if (n_out == 0) return RG_OK;
    if (!xyz || !in_off || !out_off || !in_slot || !out_xyz || n_clouds < 1 || (out_mask && !mask)) return RG_ERR_ARG;
    k_augment_gather<<<rg_cdiv(n_out, AUG_THREADS), AUG_THREADS, 0, (hipStream_t)stream>>>(
        xyz, mask, in_off, n_in, perm, out_off, in_slot, n_clouds, n_out, xform, noise, (uint32_t)seed, (uint32_t)(seed >> 32), step,
        out_xyz, out_mask);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
