// Point-to-point ICP refinement and registration fitness for gfx950 (no reference counterpart): the polish of a coarse pose on the
// full-resolution clouds, and Open3D-style fitness / inlier_rmse of a pose without ground truth.
//
// One iteration = two launches, nothing waits for the host:
//   k_icp_accumulate  one fused pass over the source rows: transform by the pair's pose (float32, rounded per operation: the bits of
//                     regtr_se3_transform), nearest target row of the same pair inside max_dist through the targets' cell grid (float64
//                     d2 on the widened coordinates, ties to the lower index: k_nearest_in_radius's body), and the float64 moments of the
//                     matched rows  n | sum d2 | sum p (3) | sum q (3) | sum p q^T (9)  with p the ORIGINAL source point, so that the
//                     solve yields the absolute pose and nothing is composed over the iterations.
//                     A workgroup owns chunk c of pair b (ICP_CHUNK rows; the chunking is a function of the cloud lengths only); a thread
//                     adds its rows in row order, the xor tree joins a wave, the waves are added in order, and the result goes to
//                     ws[b][c][17].  No atomics: the sums are bit-reproducible.
//   k_icp_solve       one wave per pair: the pair's chunks in ascending order, fitness = n / n_src_b, inlier_rmse = sqrt(sum d2 / n),
//                     the stop rule, else centroids, cov = sum p q^T / n - pbar qbar^T, R by pro_rotation (the pose head's reflection
//                     rule), t = qbar - R pbar, rounded to float32 into pose.
// A pair that is done (converged, fewer than three matches, a degenerate covariance, a non-finite pose) is skipped by every later pass
// with a workgroup-uniform test; its pose, stats and idx rows are never written again.
// Every read is hashed or bounded by a count read from the grid: a source point far outside the targets finds 27 empty cells.
#include "common.h"
#include "cellgrid.h"
#include "procrustes_solve.h"
#include "augment_common.h"      // transform_rn: the float32 rigid transform rounded per operation

namespace {

constexpr int ICP_THREADS = 256;
constexpr int ICP_CHUNK = 256;       // source rows per workgroup (regtr_icp_chunk; regtr_amd/refine.py: CHUNK)
constexpr int ICP_ROWS = ICP_CHUNK / ICP_THREADS;
constexpr int ICP_MOMENTS = 17;      // n, sum d2, sum p (3), sum q (3), sum p q^T (9, row-major: p's component is the row)
constexpr int ICP_MAX_PAIRS = 65535;      // a launch's grid.y

static_assert(ICP_CHUNK % ICP_THREADS == 0, "a thread owns whole rows of its chunk");

struct IcpArgs {
    const float* src;       // [n_src, 3]
    const int* src_off;     // [B + 1]
    const int* tgt_off;     // [B + 1]
    int B, cpp;             // pairs; chunk slots per pair in ws
    GridView g;             // the targets' grid
    double r2;              // max_dist^2
    float* pose;            // [B, 12]
    int iter, stats_only;
    double rel_fitness, rel_rmse;
    double* stats;          // [B, 3]
    int* iters_run;         // [B]
    int* done;              // [B]
    int* idx;               // [n_src] | NULL
    double* d2;             // [n_src] | NULL
    double* ws;             // [B, cpp, ICP_MOMENTS]
};

__global__ void __launch_bounds__(ICP_THREADS) k_icp_accumulate(IcpArgs a)
{
    __shared__ double sh[ICP_THREADS / RG_WAVE];
    const int b = blockIdx.y, c = blockIdx.x;
    const int s0 = a.src_off[b], s1 = a.src_off[b + 1];
    if ((long long)c * ICP_CHUNK >= (long long)(s1 - s0)) return;      // not a chunk of this pair
    if (a.iter > 0 && a.done[b]) return;                               // (iteration 0 initialises done: nothing to read yet)
    const unsigned mask = rg_live_table(a.tgt_off[a.B]) - 1u;          // the table was built for every target row
    float T[12];
#pragma unroll
    for (int e = 0; e < 12; e++) T[e] = a.pose[(size_t)b * 12 + e];

    double m[ICP_MOMENTS];
#pragma unroll
    for (int e = 0; e < ICP_MOMENTS; e++) m[e] = 0.0;
    for (int k = 0; k < ICP_ROWS; k++) {
        const int row = s0 + c * ICP_CHUNK + k * ICP_THREADS + (int)threadIdx.x;
        if (row >= s1) break;
        const float px = a.src[3 * (size_t)row], py = a.src[3 * (size_t)row + 1], pz = a.src[3 * (size_t)row + 2];
        float y[3];
        transform_rn(T, px, py, pz, y);
        int64_t cx, cy, cz;
        cell_of(y[0], y[1], y[2], a.g.inv_cs, cx, cy, cz);
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
        if (a.d2) a.d2[row] = best_i >= 0 ? best : __builtin_huge_val();
        if (best_i >= 0) {
            const double p[3] = {(double)px, (double)py, (double)pz}, q[3] = {(double)bq[0], (double)bq[1], (double)bq[2]};
            m[0] += 1.0;
            m[1] += best;
#pragma unroll
            for (int d = 0; d < 3; d++) { m[2 + d] += p[d]; m[5 + d] += q[d]; }
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int cc = 0; cc < 3; cc++) m[8 + 3 * r + cc] += p[r] * q[cc];
        }
    }
    double* out = a.ws + ((size_t)b * a.cpp + c) * ICP_MOMENTS;
#pragma unroll
    for (int e = 0; e < ICP_MOMENTS; e++) {
        const double v = rg_block_sum<ICP_THREADS>(m[e], sh);
        if (threadIdx.x == 0) out[e] = v;
    }
}

__global__ void __launch_bounds__(RG_WAVE) k_icp_solve(IcpArgs a)
{
    __shared__ double sm[ICP_MOMENTS];
    const int b = blockIdx.x;
    if (a.iter > 0 && a.done[b]) return;
    const int n_src = a.src_off[b + 1] - a.src_off[b];
    const int chunks = (int)(((long long)n_src + ICP_CHUNK - 1) / ICP_CHUNK);
    if (threadIdx.x < ICP_MOMENTS) {       // lane e: moment e over the pair's chunks, ascending
        const double* w = a.ws + (size_t)b * a.cpp * ICP_MOMENTS + threadIdx.x;
        double s = 0.0;
        for (int c = 0; c < chunks && c < a.cpp; c++) s += w[(size_t)c * ICP_MOMENTS];
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
    if (a.stats_only) {
        if (a.iter == 0) { a.done[b] = 0; a.iters_run[b] = 0; }
        return;
    }
    float* P = a.pose + 12 * (size_t)b;
    bool stop = n < 3.0;
    for (int e = 0; e < 12; e++) stop = stop || !(fabsf(P[e]) <= 3.0e38f);      // a non-finite pose freezes the pair
    if (a.iter > 0) stop = stop || (fabs(fitness - f_prev) < a.rel_fitness && fabs(rmse - r_prev) < a.rel_rmse);
    double R[9], pb[3], qb[3];
    if (!stop) {
        double cov[9], U[9], S[3], V[9];
        for (int d = 0; d < 3; d++) { pb[d] = sm[2 + d] / n; qb[d] = sm[5 + d] / n; }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) cov[3 * r + c] = sm[8 + 3 * r + c] / n - pb[r] * qb[c];
        const double d = pro_rotation(cov, U, S, V, R);
        // the degeneracy test of k_procrustes_bwd: collinear or coincident matches fix no rotation
        const double lam[3] = {S[0], S[1], d * S[2]};
        const double lmin = fmin(fmin(lam[0] + lam[1], lam[0] + lam[2]), lam[1] + lam[2]);
        stop = !(lmin > 0x1p-23 * lam[0]);
    }
    if (stop) {
        a.done[b] = 1;
        if (a.iter == 0) a.iters_run[b] = 0;
        return;
    }
    for (int r = 0; r < 3; r++) {
        const double t = qb[r] - (R[3 * r] * pb[0] + R[3 * r + 1] * pb[1] + R[3 * r + 2] * pb[2]);
        P[4 * r] = (float)R[3 * r]; P[4 * r + 1] = (float)R[3 * r + 1]; P[4 * r + 2] = (float)R[3 * r + 2];
        P[4 * r + 3] = (float)t;
    }
    a.done[b] = 0;
    a.iters_run[b] = a.iter + 1;
}

}  // namespace

extern "C" {

int regtr_icp_chunk(void) { return ICP_CHUNK; }

size_t regtr_icp_ws_bytes(int n_pairs, int max_src_len)
{
    if (n_pairs < 0 || max_src_len < 0) return 0;
    const size_t cpp = (size_t)rg_cdiv(max_src_len > 0 ? max_src_len : 1, ICP_CHUNK);
    return rg_align_up((size_t)(n_pairs > 0 ? n_pairs : 1) * cpp * ICP_MOMENTS * sizeof(double), 256);
}

int regtr_icp_step(const float* src_xyz, const int* src_off, int n_src, int max_src_len, const int* tgt_off, int n_tgt, int n_pairs,
                   double max_dist, float grid_radius, const void* grid_ws, size_t grid_ws_bytes, float* pose, int iter, int stats_only,
                   double rel_fitness, double rel_rmse, double* stats, int* iters_run, int* done, int* idx, double* d2, void* ws,
                   size_t ws_bytes, void* stream)
{
    if (n_src < 0 || n_tgt < 0 || n_pairs < 0 || max_src_len < 0 || iter < 0 || n_pairs > ICP_MAX_PAIRS || max_src_len > n_src) return RG_ERR_ARG;
    if (n_pairs == 0 || n_src == 0) return RG_OK;
    if (!src_xyz || !src_off || !tgt_off || !grid_ws || !pose || !stats || !iters_run || !done || !ws || !(max_dist > 0.0) ||
        !(grid_radius > 0.f) || !((double)grid_radius * (1.0 + 1e-6) >= max_dist) || max_src_len < 1)
        return RG_ERR_ARG;
    if (grid_ws_bytes < regtr_cellgrid_ws_bytes(n_tgt, n_pairs) || ws_bytes < regtr_icp_ws_bytes(n_pairs, max_src_len)) return RG_ERR_WORKSPACE;
    IcpArgs a;
    a.src = src_xyz; a.src_off = src_off; a.tgt_off = tgt_off;
    a.B = n_pairs; a.cpp = rg_cdiv(max_src_len, ICP_CHUNK);
    a.g = grid_view(carve_grid((void*)grid_ws, grid_ws_bytes, n_tgt > 0 ? n_tgt : 1), grid_radius);
    a.r2 = max_dist * max_dist;
    a.pose = pose; a.iter = iter; a.stats_only = stats_only != 0;
    a.rel_fitness = rel_fitness; a.rel_rmse = rel_rmse;
    a.stats = stats; a.iters_run = iters_run; a.done = done; a.idx = idx; a.d2 = d2; a.ws = (double*)ws;
    hipStream_t st = (hipStream_t)stream;
    k_icp_accumulate<<<dim3(a.cpp, n_pairs), ICP_THREADS, 0, st>>>(a);
    k_icp_solve<<<n_pairs, RG_WAVE, 0, st>>>(a);
    RG_RETURN_IF_LAUNCH_FAILED();
    return RG_OK;
}

}  // extern "C"
