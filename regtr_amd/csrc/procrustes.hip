// Weighted Procrustes / Kabsch pose solve for gfx950: one workgroup per (pair, decoder layer) fuses
//   sigmoid(overlap logits) -> weight normalisation -> weighted centroids -> 3x3 covariance -> 3x3 SVD ->
//   det-corrected rotation + translation
// i.e. the pose assembly of /root/reference/src/models/regtr.py:185-203 and compute_rigid_transform of
// /root/reference/src/utils/se3_torch.py:108-154, which the reference runs as ~20 torch ops + torch.svd + a host
// assert per pair.  Correspondences in both directions are concatenated exactly as the reference does:
//   a = [src_kp ; tgt_corr]   b = [src_corr ; tgt_kp]   w = sigmoid([src_logit ; tgt_logit]).
// Reductions are float64 with a fixed tree (deterministic); the SVD is a one-sided Jacobi in float64 executed by
// one lane (9 numbers), singular values sorted descending so that "flip V[:,2]" (se3_torch.py:145-147) hits the
// smallest one as LAPACK's ordering does in the reference.
// k_procrustes_bwd is the backward of the same solve in closed form; both kernels recompute the pair's moments and rotation through the
// shared device functions below (pro_moments, pro_rotation), so nothing is saved between them.
#include "common.h"
#include "procrustes_solve.h"      // svd3, pro_rotation (shared with icp.hip)

namespace {

constexpr int PT = 256;

__device__ __forceinline__ double block_sum(double v, double* sh)
{
    v = rg_wave_sum(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if (rg_lane() == 0) sh[wave] = v;
    __syncthreads();
    double t = 0;
#pragma unroll
    for (int w = 0; w < PT / RG_WAVE; w++) t += sh[w];
    return t;
}

// One (pair, layer): the rows of the pair in the model's layout.
struct ProPair {
    const float *kp, *corr, *logit;   // kp [N_total, 3]; corr, logit: this layer's [N_total, 3], [N_total]
    int s0, t0, ns, n;                // first src row, first tgt row, src rows, src + tgt rows
};

__device__ __forceinline__ ProPair pro_pair(const float* kp, const float* corr, const float* logit, const int* seg_off, int B, int n_total,
                                            int b, int l)
{
    const int s0 = seg_off[b], s1 = seg_off[b + 1], t0 = seg_off[B + b], t1 = seg_off[B + b + 1];
    return ProPair{kp, corr + (size_t)l * n_total * 3, logit + (size_t)l * n_total, s0, t0, s1 - s0, (s1 - s0) + (t1 - t0)};
}

// point i of the pair: a = [src_kp ; tgt_corr], b = [src_corr ; tgt_kp], w = sigmoid([src ; tgt] logit); -> its row
__device__ __forceinline__ int pro_fetch(const ProPair& q, int i, float (&a)[3], float (&bb)[3], float& w)
{
    const bool is_src = i < q.ns;
    const int row = is_src ? q.s0 + i : q.t0 + (i - q.ns);
    const float* kpp = q.kp + 3 * (size_t)row;
    const float* cp = q.corr + 3 * (size_t)row;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        a[d] = is_src ? kpp[d] : cp[d];      // regtr.py:187-190
        bb[d] = is_src ? cp[d] : kpp[d];
    }
    w = 1.0f / (1.0f + expf(-q.logit[row]));   // torch.sigmoid, regtr.py:191-194
    return row;
}

// The three reduction passes of the pair, every thread of the workgroup: weight sum -> weighted centroids -> covariance.
struct ProMoments {
    double wsum;
    float denom, caf[3], cbf[3];
    double cov[9];
};

__device__ __forceinline__ void pro_moments(const ProPair& q, double* sh, ProMoments& m)
{
    const int n = q.n;
    // pass 1: sum of weights
    double wsum = 0;
    for (int i = threadIdx.x; i < n; i += PT) {
        float a[3], bb[3], w;
        pro_fetch(q, i, a, bb, w);
        wsum += w;
    }
    wsum = block_sum(wsum, sh);
    const float denom = fmaxf((float)wsum, 1e-6f);               // se3_torch.py:127-128 (_EPS)
    m.wsum = wsum;
    m.denom = denom;

    // pass 2: weighted centroids
    double ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < n; i += PT) {
        float a[3], bb[3], w;
        pro_fetch(q, i, a, bb, w);
        const float wn = w / denom;
#pragma unroll
        for (int d = 0; d < 3; d++) { ca[d] += (double)(a[d] * wn); cb[d] += (double)(bb[d] * wn); }
    }
#pragma unroll
    for (int d = 0; d < 3; d++) { ca[d] = block_sum(ca[d], sh); cb[d] = block_sum(cb[d], sh); }
    float caf[3], cbf[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { caf[d] = (float)ca[d]; cbf[d] = (float)cb[d]; }

    // pass 3: cov = sum (a - ca)(b - cb)^T wn                    se3_torch.py:131-133
    double cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += PT) {
        float a[3], bb[3], w;
        pro_fetch(q, i, a, bb, w);
        const float wn = w / denom;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) cov[3 * r + c] += (double)((a[r] - caf[r]) * ((bb[c] - cbf[c]) * wn));
    }
#pragma unroll
    for (int e = 0; e < 9; e++) m.cov[e] = block_sum(cov[e], sh);
#pragma unroll
    for (int d = 0; d < 3; d++) { m.caf[d] = caf[d]; m.cbf[d] = cbf[d]; }
}

struct ProArgs {
    const float* kp;      // [N_total, 3] coarsest-level points, stacked [src clouds..., tgt clouds...]
    const float* corr;    // [L, N_total, 3] predicted corresponding coordinates
    const float* logit;   // [L, N_total]   overlap logits
    const int* seg_off;   // [2B + 1]
    float* pose;          // [L, B, 3, 4]
    int B, n_total;
    int* status;          // optional: REGTR_STATUS_NONFINITE_POSE is OR-ed in when a pose comes out non-finite
};

__global__ void __launch_bounds__(PT) k_procrustes(ProArgs g)
{
    __shared__ double sh[PT / RG_WAVE];
    const int b = blockIdx.x, l = blockIdx.y;
    const ProPair q = pro_pair(g.kp, g.corr, g.logit, g.seg_off, g.B, g.n_total, b, l);
    ProMoments m;
    pro_moments(q, sh, m);

    if (threadIdx.x == 0) {
        double U[9], S[3], V[9], R[9];
        pro_rotation(m.cov, U, S, V, R);
        const float* caf = m.caf;
        const float* cbf = m.cbf;
        float* P = g.pose + ((size_t)l * g.B + b) * 12;
        bool bad = false;
        for (int r = 0; r < 3; r++) {
            const double t = -(R[3 * r] * caf[0] + R[3 * r + 1] * caf[1] + R[3 * r + 2] * caf[2]) + cbf[r];   // :151
            P[4 * r] = (float)R[3 * r]; P[4 * r + 1] = (float)R[3 * r + 1]; P[4 * r + 2] = (float)R[3 * r + 2];
            P[4 * r + 3] = (float)t;
            bad = bad || !(fabs(R[3 * r]) <= 2.0) || !(fabs(R[3 * r + 1]) <= 2.0) || !(fabs(R[3 * r + 2]) <= 2.0) || !(fabs(t) < 1e30);
        }
        // a NaN / Inf anywhere upstream (an f16 pair operand out of range that a ReLU or max swallowed on the way, a non-finite input
        // coordinate) ends here: R|t is the sum over every token of the pair
        if (bad && g.status) atomicOr(g.status, REGTR_STATUS_NONFINITE_POSE);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// The gradient of R|t with respect to a, b and w in closed form, without the derivative of an SVD.  With G_R | g_t = d_pose:
//   G = G_R - g_t ca^T,  dca = -R^T g_t,  dcb = g_t
//   A = (G R^T - R G^T) / 2,  A' = V^T A V,  lam = (S0, S1, d S2)
//   Y'_ij = -A'_ij / (lam_i + lam_j) (i != j),  dH = 2 R^T V Y' V^T = 2 U diag(1, 1, d) Y' V^T
//   da_i = wn_i (dH b'_i + dca),  db_i = wn_i (dH^T a'_i + dcb)
//   dwn_i = a'_i^T dH b'_i + a'_i . dca + b'_i . dcb      (a_i . dca + b_i . dcb less its constant g_t . t, which the mean below removes)
//   dw_i = (dwn_i - sum_j wn_j dwn_j) / W,  dlogit_i = dw_i w_i (1 - w_i)
// The forward's quantities are recomputed by the forward's own code (pro_moments, pro_rotation); w, wn and the centroids enter as the
// float32 values the forward rounded them to, everything else is float64.  Only sums lam_i + lam_j divide: equal singular values are
// harmless.  Where R is no differentiable function of the float32 inputs -- min (lam_i + lam_j) <= 2^-23 lam_0 (the zero covariance
// included), the weight sum at its 1e-6 clamp, an empty pair -- the pair's rows are exactly 0.
struct ProBwdArgs {
    const float *kp, *corr, *logit;
    const int* seg_off;
    const float* d_pose;   // [L, B, 3, 4]
    float* d_corr;         // [L, N_total, 3]
    float* d_logit;        // [L, N_total] | NULL
    float* d_kp;           // [L, N_total, 3] | NULL: per layer, the caller sums
    float* d_weight;       // [L, N_total] | NULL: dw_i, without the sigmoid's factor
    int B, n_total;
};

__global__ void __launch_bounds__(PT) k_procrustes_bwd(ProBwdArgs g)
{
    __shared__ double sh[PT / RG_WAVE];
    __shared__ double sm[15];      // dH (9), dca (3), dcb (3)
    __shared__ int s_zero;
    const int b = blockIdx.x, l = blockIdx.y;
    const ProPair q = pro_pair(g.kp, g.corr, g.logit, g.seg_off, g.B, g.n_total, b, l);
    const int n = q.n;
    ProMoments m;
    pro_moments(q, sh, m);

    if (threadIdx.x == 0) {
        double U[9], S[3], V[9], R[9];
        const double d = pro_rotation(m.cov, U, S, V, R);
        const double lam[3] = {S[0], S[1], d * S[2]};
        const double lmin = fmin(fmin(lam[0] + lam[1], lam[0] + lam[2]), lam[1] + lam[2]);
        const bool zero = !((float)m.wsum > 1e-6f) || !(lmin > 0x1p-23 * lam[0]);
        s_zero = zero;
        if (!zero) {
            const float* dp = g.d_pose + ((size_t)l * g.B + b) * 12;
            double G[9], gt[3];
            for (int r = 0; r < 3; r++) {
                gt[r] = dp[4 * r + 3];
                for (int c = 0; c < 3; c++) G[3 * r + c] = (double)dp[4 * r + c] - gt[r] * (double)m.caf[c];
            }
            double M[9], A[9], T[9], Ap[9], Y[9];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) M[3 * i + j] = G[3 * i] * R[3 * j] + G[3 * i + 1] * R[3 * j + 1] + G[3 * i + 2] * R[3 * j + 2];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) A[3 * i + j] = 0.5 * (M[3 * i + j] - M[3 * j + i]);
            for (int i = 0; i < 3; i++)      // T = A V
                for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * i] * V[j] + A[3 * i + 1] * V[3 + j] + A[3 * i + 2] * V[6 + j];
            for (int i = 0; i < 3; i++)      // A' = V^T T
                for (int j = 0; j < 3; j++) Ap[3 * i + j] = V[i] * T[j] + V[3 + i] * T[3 + j] + V[6 + i] * T[6 + j];
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) Y[3 * i + j] = i == j ? 0.0 : -Ap[3 * i + j] / (lam[i] + lam[j]);
            for (int i = 0; i < 3; i++)      // T = U diag(1, 1, d) Y'
                for (int j = 0; j < 3; j++) T[3 * i + j] = U[3 * i] * Y[j] + U[3 * i + 1] * Y[3 + j] + d * U[3 * i + 2] * Y[6 + j];
            for (int r = 0; r < 3; r++)      // dH = 2 T V^T
                for (int c = 0; c < 3; c++) sm[3 * r + c] = 2.0 * (T[3 * r] * V[3 * c] + T[3 * r + 1] * V[3 * c + 1] + T[3 * r + 2] * V[3 * c + 2]);
            for (int c = 0; c < 3; c++) {
                sm[9 + c] = -(R[c] * gt[0] + R[3 + c] * gt[1] + R[6 + c] * gt[2]);
                sm[12 + c] = gt[c];
            }
        }
    }
    __syncthreads();
    const bool zero = s_zero != 0;
    double dH[9], dca[3], dcb[3];
    if (!zero) {
#pragma unroll
        for (int e = 0; e < 9; e++) dH[e] = sm[e];
#pragma unroll
        for (int d = 0; d < 3; d++) { dca[d] = sm[9 + d]; dcb[d] = sm[12 + d]; }
    }

    // one point's share: wn, a', b', u = dH b', v = dH^T a', dwn
    auto point = [&](int i, float& w, double& wn, double (&u)[3], double (&v)[3], double& dwn) {
        float a[3], bb[3];
        const int row = pro_fetch(q, i, a, bb, w);
        wn = (double)(w / m.denom);
        double ap[3], bp[3];
#pragma unroll
        for (int d = 0; d < 3; d++) { ap[d] = (double)a[d] - (double)m.caf[d]; bp[d] = (double)bb[d] - (double)m.cbf[d]; }
        dwn = 0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            u[r] = dH[3 * r] * bp[0] + dH[3 * r + 1] * bp[1] + dH[3 * r + 2] * bp[2];
            v[r] = dH[r] * ap[0] + dH[3 + r] * ap[1] + dH[6 + r] * ap[2];
            dwn += ap[r] * u[r] + ap[r] * dca[r] + bp[r] * dcb[r];
        }
        return row;
    };

    // sum_j wn_j dwn_j, float64 in the fixed tree
    double mean = 0;
    if (!zero) {
        for (int i = threadIdx.x; i < n; i += PT) {
            float w;
            double wn, u[3], v[3], dwn;
            point(i, w, wn, u, v, dwn);
            mean += wn * dwn;
        }
    }
    mean = block_sum(mean, sh);

    // owner computes: every row of the pair is written once, by one thread
    const size_t lo = (size_t)l * g.n_total;
    for (int i = threadIdx.x; i < n; i += PT) {
        const bool is_src = i < q.ns;
        const size_t row = lo + (size_t)(is_src ? q.s0 + i : q.t0 + (i - q.ns));
        float da[3] = {0.f, 0.f, 0.f}, db[3] = {0.f, 0.f, 0.f}, dw = 0.f, dl = 0.f;
        if (!zero) {
            float w;
            double wn, u[3], v[3], dwn;
            point(i, w, wn, u, v, dwn);
#pragma unroll
            for (int d = 0; d < 3; d++) { da[d] = (float)(wn * (u[d] + dca[d])); db[d] = (float)(wn * (v[d] + dcb[d])); }
            const double dwd = (dwn - mean) / (double)m.denom;
            dw = (float)dwd;
            dl = (float)(dwd * ((double)w * (1.0 - (double)w)));
        }
        float* dc = g.d_corr + 3 * row;
#pragma unroll
        for (int d = 0; d < 3; d++) dc[d] = is_src ? db[d] : da[d];
        if (g.d_kp) {
            float* dk = g.d_kp + 3 * row;
#pragma unroll
            for (int d = 0; d < 3; d++) dk[d] = is_src ? da[d] : db[d];
        }
        if (g.d_logit) g.d_logit[row] = dl;
        if (g.d_weight) g.d_weight[row] = dw;
    }
}

}  // namespace

extern "C" {

int regtr_abi_version(void) { return REGTR_ABI_VERSION; }

int regtr_weighted_procrustes(const float* kp, const float* corr, const float* logit, const int* seg_off, int n_pairs,
                              int n_total, int n_layers, float* pose, int* status, void* stream)
{
    if (!kp || !corr || !logit || !seg_off || !pose || n_pairs < 1 || n_layers < 1 || n_total < 0) return RG_ERR_ARG;
    ProArgs g{kp, corr, logit, seg_off, pose, n_pairs, n_total, status};
    k_procrustes<<<dim3(n_pairs, n_layers), PT, 0, (hipStream_t)stream>>>(g);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_weighted_procrustes_bwd(const float* kp, const float* corr, const float* logit, const int* seg_off, int n_pairs, int n_total,
                                  int n_layers, const float* d_pose, float* d_corr, float* d_logit, float* d_kp, float* d_weight,
                                  void* stream)
{
    if (!kp || !corr || !logit || !seg_off || !d_pose || !d_corr || n_pairs < 1 || n_layers < 1 || n_total < 0) return RG_ERR_ARG;
    ProBwdArgs g{kp, corr, logit, seg_off, d_pose, d_corr, d_logit, d_kp, d_weight, n_pairs, n_total};
    k_procrustes_bwd<<<dim3(n_pairs, n_layers), PT, 0, (hipStream_t)stream>>>(g);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
