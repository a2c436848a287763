// Surface normals and point-to-plane ICP for gfx950 (no reference counterpart): the refinement of icp.hip with the residual measured
// along the target's normal, so that matches may slide along the planes an indoor scan mostly consists of.
//
//   k_estimate_normals     one thread per point: the 27-cell probe of the cloud's own grid, every neighbour q of the same cloud with
//                          float64 d2 = (dx dx + dy dy) + dz dz < radius^2 (the point itself included) adds its QUANTISED difference
//                          dq = rint((q - p) 2^s), radius 2^s <= 2^20, to int64 sums  n | sum dq (3) | sum dq dq^T (6, upper triangle).
//                          Integer sums do not depend on the order of a cell's entries (k_scatter_cells fills cells through an atomicAdd,
//                          in an order that differs between runs): the moments, and so the normals, are bit-reproducible.  Then, in
//                          float64, m = S1 / n, C = S2 / n - m m^T (one division and one product per entry, in that order), svd3(C):
//                          for a symmetric positive semi-definite C the singular values are the eigenvalues l2 >= l1 >= l0 and the last
//                          column of V is the normal, rounded to float32.  valid = n >= 3 and l1 > 2^-40 l2; else the normal is 0.
//   k_icp_plane_accumulate k_icp_accumulate's pass (the same chunking, float32 transform and match rule: idx, n and sum d2 are its bits)
//                          with, for a match whose target has a valid normal nrm, r = nrm . (y - q) and J = [y x nrm, nrm] in float64
//                          (y the transformed source point):  n | sum d2 | n_sys | sum J^T J (21, upper triangle by rows) | sum J^T r (6)
//                          per chunk into partial[b][c][30], in the fixed order of icp.hip (rows per thread, xor tree, waves in order).
//   k_icp_plane_solve      one wave per pair: the chunks in ascending order, stats and Open3D's stop rule as k_icp_solve; further stops:
//                          n_sys < 6, and a pivot <= 2^-23 of the LDL^T of the system scaled to unit diagonal (one wall fixes no pose).
//                          Else x = -(J^T J)^-1 J^T r, dT = (Rz(x2) Ry(x1) Rx(x0), x[3:6]) as Open3D composes it, pose64 <- dT pose64 on
//                          the float64 master pose (iteration 0 takes it from the float32 pose) and pose = its float32 rounding.
// A done pair is skipped by every later pass; its pose, pose64, stats and idx rows are never written again.  No atomics, no workspace.
#include "common.h"
#include "cellgrid.h"
#include "procrustes_solve.h"      // svd3
#include "augment_common.h"        // transform_rn: the float32 rigid transform rounded per operation

namespace {

constexpr int NRM_THREADS = 256;
constexpr int NRM_MOMENTS = 10;       // n, sum dq (3), sum dq dq^T (xx xy xz yy yz zz)
constexpr int PL_THREADS = 256;
constexpr int PL_ROWS = 1;            // rows per thread: PL_THREADS * PL_ROWS = regtr_icp_chunk()
constexpr int PL_SUMS = 30;           // n, sum d2, n_sys, J^T J upper (21), J^T r (6)
constexpr int PL_MAX_PAIRS = 65535;   // a launch's grid.y

struct NormalArgs {
    const float* xyz;       // [n, 3]
    const int* off;         // [C + 1]
    int n, C;
    GridView g;
    double r2, qscale;      // radius^2; 2^s
    float* normals;         // [n, 3]
    int* valid;             // [n]
    long long* moments;     // [n, 10] | NULL
};

__global__ void __launch_bounds__(NRM_THREADS) k_estimate_normals(NormalArgs a)
{
    const int i = blockIdx.x * NRM_THREADS + (int)threadIdx.x;
    if (i >= a.n) return;
    const int total = a.off[a.C];
    if (i >= total) {      // rows past the last cloud belong to none
        a.normals[3 * (size_t)i] = a.normals[3 * (size_t)i + 1] = a.normals[3 * (size_t)i + 2] = 0.f;
        a.valid[i] = 0;
        if (a.moments)
            for (int e = 0; e < NRM_MOMENTS; e++) a.moments[(size_t)i * NRM_MOMENTS + e] = 0;
        return;
    }
    const int c = rg_find_segment(a.off, a.C, i);
    const unsigned mask = rg_live_table(total) - 1u;
    const float px = a.xyz[3 * (size_t)i], py = a.xyz[3 * (size_t)i + 1], pz = a.xyz[3 * (size_t)i + 2];
    int64_t cx, cy, cz;
    cell_of(px, py, pz, a.g.inv_cs, cx, cy, cz);
    long long m[NRM_MOMENTS];
#pragma unroll
    for (int e = 0; e < NRM_MOMENTS; e++) m[e] = 0;
    for (int n = 0; n < 27; n++) {
        int cnt, start;
        slot_find(a.g.slots, mask, cell_key(cx + n % 3 - 1, cy + (n / 3) % 3 - 1, cz + n / 9 - 1), c, cnt, start);
        for (int t = 0; t < cnt; t++) {
            const float4 sp = a.g.sorted[start + t];
            const double dx = (double)sp.x - (double)px, dy = (double)sp.y - (double)py, dz = (double)sp.z - (double)pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 < a.r2)) continue;
            const long long qx = __double2ll_rn(dx * a.qscale), qy = __double2ll_rn(dy * a.qscale), qz = __double2ll_rn(dz * a.qscale);
            m[0] += 1;
            m[1] += qx; m[2] += qy; m[3] += qz;
            m[4] += qx * qx; m[5] += qx * qy; m[6] += qx * qz;
            m[7] += qy * qy; m[8] += qy * qz; m[9] += qz * qz;
        }
    }
    if (a.moments)
#pragma unroll
        for (int e = 0; e < NRM_MOMENTS; e++) a.moments[(size_t)i * NRM_MOMENTS + e] = m[e];
    float nrm[3] = {0.f, 0.f, 0.f};
    int ok = 0;
    if (m[0] >= 3) {
        const double n = (double)m[0];
        const double mx = (double)m[1] / n, my = (double)m[2] / n, mz = (double)m[3] / n;
        double C[9], U[9], S[3], V[9];
        C[0] = (double)m[4] / n - mx * mx; C[1] = (double)m[5] / n - mx * my; C[2] = (double)m[6] / n - mx * mz;
        C[4] = (double)m[7] / n - my * my; C[5] = (double)m[8] / n - my * mz; C[8] = (double)m[9] / n - mz * mz;
        C[3] = C[1]; C[6] = C[2]; C[7] = C[5];
        svd3(C, U, S, V);
        if (S[1] > 0x1p-40 * S[0]) {
            ok = 1;
            nrm[0] = (float)V[2]; nrm[1] = (float)V[5]; nrm[2] = (float)V[8];
        }
    }
    a.normals[3 * (size_t)i] = nrm[0]; a.normals[3 * (size_t)i + 1] = nrm[1]; a.normals[3 * (size_t)i + 2] = nrm[2];
    a.valid[i] = ok;
}

struct PlaneArgs {
    const float* src;       // [n_src, 3]
    const int* src_off;     // [B + 1]
    const int* tgt_off;     // [B + 1]
    const float* nrm;       // [n_tgt, 3]
    const int* nvalid;      // [n_tgt]
    int B, cpp;             // pairs; chunk slots per pair in partial
    GridView g;             // the targets' grid
    double r2;              // max_dist^2
    float* pose;            // [B, 12]
    double* pose64;         // [B, 12]
    int iter, stats_only;
    double rel_fitness, rel_rmse;
    double* stats;          // [B, 3]
    int* iters_run;         // [B]
    int* done;              // [B]
    int* idx;               // [n_src] | NULL
    double* partial;        // [B, cpp, PL_SUMS]
};

__global__ void __launch_bounds__(PL_THREADS) k_icp_plane_accumulate(PlaneArgs a)
{
    __shared__ double sh[PL_THREADS / RG_WAVE];
    const int b = blockIdx.y, c = blockIdx.x;
    const int s0 = a.src_off[b], s1 = a.src_off[b + 1];
    if ((long long)c * (PL_THREADS * PL_ROWS) >= (long long)(s1 - s0)) return;      // not a chunk of this pair
    if (a.iter > 0 && a.done[b]) return;                                            // (iteration 0 initialises done)
    const unsigned mask = rg_live_table(a.tgt_off[a.B]) - 1u;
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = a.pose[(size_t)b * 12 + e];

    static_assert(PL_SUMS == 3 + 21 + 6, "n, sum d2, n_sys, the upper triangle, the right-hand side");
    double m[PL_SUMS];
#pragma unroll
    for (int e = 0; e < PL_SUMS; e++) m[e] = 0.0;
    for (int k = 0; k < PL_ROWS; k++) {
        const int row = s0 + c * (PL_THREADS * PL_ROWS) + k * PL_THREADS + (int)threadIdx.x;
        if (row >= s1) break;
        float y[3];
        transform_rn(T, a.src[3 * (size_t)row], a.src[3 * (size_t)row + 1], a.src[3 * (size_t)row + 2], y);
        int64_t cx, cy, cz;
        cell_of(y[0], y[1], y[2], a.g.inv_cs, cx, cy, cz);
        // the match: k_icp_accumulate's rule and arithmetic (strict float64 nearest inside max_dist, ties to the lower index)
        double best = a.r2;
        int best_i = -1;
        float bq[3] = {0.f, 0.f, 0.f};
        for (int n = 0; n < 27; n++) {
            int cnt, start;
            slot_find(a.g.slots, mask, cell_key(cx + n % 3 - 1, cy + (n / 3) % 3 - 1, cz + n / 9 - 1), b, cnt, start);
            for (int t = 0; t < cnt; t++) {
                const float4 sp = a.g.sorted[start + t];
                const double dx = (double)y[0] - (double)sp.x, dy = (double)y[1] - (double)sp.y, dz = (double)y[2] - (double)sp.z;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const int i = __float_as_int(sp.w);
                if (d2 < best || (d2 == best && best_i >= 0 && i < best_i)) { best = d2; best_i = i; bq[0] = sp.x; bq[1] = sp.y; bq[2] = sp.z; }
            }
        }
        if (a.idx) a.idx[row] = best_i;
        if (best_i >= 0) {
            m[0] += 1.0;
            m[1] += best;
            if (a.nvalid[best_i]) {
                const double Y[3] = {(double)y[0], (double)y[1], (double)y[2]};
                const double N[3] = {(double)a.nrm[3 * (size_t)best_i], (double)a.nrm[3 * (size_t)best_i + 1], (double)a.nrm[3 * (size_t)best_i + 2]};
                const double r = (N[0] * (Y[0] - (double)bq[0]) + N[1] * (Y[1] - (double)bq[1])) + N[2] * (Y[2] - (double)bq[2]);
                const double J[6] = {Y[1] * N[2] - Y[2] * N[1], Y[2] * N[0] - Y[0] * N[2], Y[0] * N[1] - Y[1] * N[0], N[0], N[1], N[2]};
                m[2] += 1.0;
                int e = 3;
#pragma unroll
                for (int p = 0; p < 6; p++)
#pragma unroll
                    for (int q = p; q < 6; q++) m[e++] += J[p] * J[q];
#pragma unroll
                for (int p = 0; p < 6; p++) m[24 + p] += J[p] * r;
            }
        }
    }
    double* out = a.partial + ((size_t)b * a.cpp + c) * PL_SUMS;
#pragma unroll
    for (int e = 0; e < PL_SUMS; e++) {
        const double v = rg_block_sum<PL_THREADS>(m[e], sh);
        if (threadIdx.x == 0) out[e] = v;
    }
}

__global__ void __launch_bounds__(RG_WAVE) k_icp_plane_solve(PlaneArgs a)
{
    __shared__ double sm[PL_SUMS];
    const int b = blockIdx.x;
    if (a.iter > 0 && a.done[b]) return;
    const int n_src = a.src_off[b + 1] - a.src_off[b];
    const int chunks = (int)(((long long)n_src + PL_THREADS * PL_ROWS - 1) / (PL_THREADS * PL_ROWS));
    if (threadIdx.x < PL_SUMS) {       // lane e: sum e over the pair's chunks, ascending
        const double* w = a.partial + (size_t)b * a.cpp * PL_SUMS + threadIdx.x;
        double s = 0.0;
        for (int c = 0; c < chunks && c < a.cpp; c++) s += w[(size_t)c * PL_SUMS];
        sm[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;

    const double n = sm[0];
    const double fitness = n_src > 0 ? n / (double)n_src : 0.0;
    const double rmse = n > 0.0 ? sqrt(sm[1] / n) : 0.0;
    double* st = a.stats + 3 * (size_t)b;
    const double f_prev = st[0], r_prev = st[1];      // (read only when iter > 0: iteration 0 wrote them)
    st[0] = fitness; st[1] = rmse; st[2] = n;
    float* P = a.pose + 12 * (size_t)b;
    double* P64 = a.pose64 + 12 * (size_t)b;
    if (a.iter == 0)
        for (int e = 0; e < 12; e++) P64[e] = (double)P[e];
    if (a.stats_only) {
        if (a.iter == 0) { a.done[b] = 0; a.iters_run[b] = 0; }
        return;
    }
    bool stop = sm[2] < 6.0;
    for (int e = 0; e < 12; e++) stop = stop || !(fabsf(P[e]) <= 3.0e38f);      // a non-finite pose freezes the pair
    if (a.iter > 0) stop = stop || (fabs(fitness - f_prev) < a.rel_fitness && fabs(rmse - r_prev) < a.rel_rmse);
    double x[6];
    if (!stop) {
        // J^T J scaled to unit diagonal, LDL^T without pivoting (the matrix is positive semi-definite), pivots against 2^-23
        double A[6][6], D[6], z[6];
        int e = 3;
        for (int p = 0; p < 6; p++)
            for (int q = p; q < 6; q++) { A[p][q] = sm[e]; A[q][p] = sm[e]; e++; }
        for (int p = 0; p < 6; p++) {
            stop = stop || !(A[p][p] > 0.0);
            D[p] = 1.0 / sqrt(A[p][p]);
        }
        if (!stop) {
            for (int p = 0; p < 6; p++) {
                for (int q = 0; q < 6; q++) A[p][q] = (A[p][q] * D[p]) * D[q];
                z[p] = -(sm[24 + p] * D[p]);
            }
            // in place: the strict lower triangle becomes L, the diagonal the pivots
            for (int j = 0; j < 6 && !stop; j++) {
                double d = A[j][j];
                for (int k = 0; k < j; k++) d -= (A[j][k] * A[j][k]) * A[k][k];
                stop = !(d > 0x1p-23);
                A[j][j] = d;
                for (int i = j + 1; i < 6; i++) {
                    double s = A[i][j];
                    for (int k = 0; k < j; k++) s -= (A[i][k] * A[j][k]) * A[k][k];
                    A[i][j] = s / d;
                }
            }
        }
        if (!stop) {
            for (int i = 0; i < 6; i++)
                for (int k = 0; k < i; k++) z[i] -= A[i][k] * z[k];
            for (int i = 0; i < 6; i++) z[i] = z[i] / A[i][i];
            for (int i = 5; i >= 0; i--)
                for (int k = i + 1; k < 6; k++) z[i] -= A[k][i] * z[k];
            for (int i = 0; i < 6; i++) x[i] = z[i] * D[i];
        }
    }
    if (stop) {
        a.done[b] = 1;
        if (a.iter == 0) a.iters_run[b] = 0;
        return;
    }
    // dT = (Rz(x2) Ry(x1) Rx(x0), x[3:6]);  pose64 <- dT pose64
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    const double R[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                         sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                         -sb, cb * sa, cb * ca};
    double Q[12];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 4; c++) Q[4 * r + c] = (R[3 * r] * P64[c] + R[3 * r + 1] * P64[4 + c]) + R[3 * r + 2] * P64[8 + c];
        Q[4 * r + 3] += x[3 + r];
    }
    for (int e = 0; e < 12; e++) { P64[e] = Q[e]; P[e] = (float)Q[e]; }
    a.done[b] = 0;
    a.iters_run[b] = a.iter + 1;
}

inline bool misaligned(const void* p, size_t a) { return ((size_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" {

int regtr_icp_chunk(void);
size_t regtr_cellgrid_ws_bytes(int ns_cap, int n_clouds);

int regtr_estimate_normals(const float* xyz, const int* seg_off, int n, int n_clouds, double radius, float grid_radius, const void* grid_ws,
                           size_t grid_ws_bytes, float* normals, int* valid, long long* moments, void* stream)
{
    if (n < 0 || n_clouds < 1 || !(radius > 0.0) || !(radius < 1e30) || !(grid_radius > 0.f) || !((double)grid_radius * (1.0 + 1e-6) >= radius))
        return RG_ERR_ARG;
    if (!seg_off || !grid_ws || misaligned(seg_off, 4) || misaligned(grid_ws, 16) || misaligned(xyz, 4) || misaligned(normals, 4) ||
        misaligned(valid, 4) || misaligned(moments, 8) || (n > 0 && (!xyz || !normals || !valid)))
        return RG_ERR_ARG;
    if (grid_ws_bytes < regtr_cellgrid_ws_bytes(n, n_clouds)) return RG_ERR_WORKSPACE;
    if (n == 0) return RG_OK;
    int e;
    const double mant = frexp(radius, &e);       // radius = mant 2^e, 0.5 <= mant < 1: the largest s with radius 2^s <= 2^20
    NormalArgs a;
    a.xyz = xyz; a.off = seg_off; a.n = n; a.C = n_clouds;
    a.g = grid_view(carve_grid((void*)grid_ws, grid_ws_bytes, n), grid_radius);
    a.r2 = radius * radius;
    a.qscale = ldexp(1.0, (mant == 0.5 ? 21 : 20) - e);
    a.normals = normals; a.valid = valid; a.moments = moments;
    k_estimate_normals<<<rg_cdiv(n, NRM_THREADS), NRM_THREADS, 0, (hipStream_t)stream>>>(a);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

int regtr_icp_plane_step(const float* src_xyz, const int* src_off, int n_src, int max_src_len, const float* tgt_normals, const int* tgt_valid,
                         const int* tgt_off, int n_tgt, int n_pairs, double max_dist, float grid_radius, const void* grid_ws,
                         size_t grid_ws_bytes, float* pose, double* pose64, int iter, int stats_only, double rel_fitness, double rel_rmse,
                         double* stats, int* iters_run, int* done, int* idx, double* partial, void* stream)
{
    if (n_src < 0 || n_tgt < 0 || n_pairs < 1 || n_pairs > PL_MAX_PAIRS || max_src_len < 0 || max_src_len > n_src || iter < 0 ||
        !(max_dist > 0.0) || !(grid_radius > 0.f) || !((double)grid_radius * (1.0 + 1e-6) >= max_dist))
        return RG_ERR_ARG;
    if (!src_off || !tgt_off || !grid_ws || !pose || !pose64 || !stats || !iters_run || !done || !partial ||
        (n_src > 0 && (!src_xyz || max_src_len < 1)) || (n_tgt > 0 && (!tgt_normals || !tgt_valid)))
        return RG_ERR_ARG;
    if (misaligned(src_xyz, 4) || misaligned(src_off, 4) || misaligned(tgt_normals, 4) || misaligned(tgt_valid, 4) || misaligned(tgt_off, 4) ||
        misaligned(grid_ws, 16) || misaligned(pose, 4) || misaligned(pose64, 8) || misaligned(stats, 8) || misaligned(iters_run, 4) ||
        misaligned(done, 4) || misaligned(idx, 4) || misaligned(partial, 8))
        return RG_ERR_ARG;
    if (PL_THREADS * PL_ROWS != regtr_icp_chunk()) return RG_ERR_ARG;      // (the chunking is regtr_icp_step's)
    if (grid_ws_bytes < regtr_cellgrid_ws_bytes(n_tgt, n_pairs)) return RG_ERR_WORKSPACE;
    if (n_src == 0) return RG_OK;
    PlaneArgs a;
    a.src = src_xyz; a.src_off = src_off; a.tgt_off = tgt_off; a.nrm = tgt_normals; a.nvalid = tgt_valid;
    a.B = n_pairs; a.cpp = rg_cdiv(max_src_len, PL_THREADS * PL_ROWS);
    a.g = grid_view(carve_grid((void*)grid_ws, grid_ws_bytes, n_tgt > 0 ? n_tgt : 1), grid_radius);
    a.r2 = max_dist * max_dist;
    a.pose = pose; a.pose64 = pose64; a.iter = iter; a.stats_only = stats_only != 0;
    a.rel_fitness = rel_fitness; a.rel_rmse = rel_rmse;
    a.stats = stats; a.iters_run = iters_run; a.done = done; a.idx = idx; a.partial = partial;
    hipStream_t st = (hipStream_t)stream;
    k_icp_plane_accumulate<<<dim3(a.cpp, n_pairs), PL_THREADS, 0, st>>>(a);
    k_icp_plane_solve<<<n_pairs, RG_WAVE, 0, st>>>(a);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
