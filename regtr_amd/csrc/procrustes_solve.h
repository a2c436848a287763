// The 3x3 solve of a Procrustes / Kabsch fit in float64: the one-sided Jacobi SVD and the det-corrected rotation.  Shared by procrustes.hip
// (the weighted pose head and its backward) and icp.hip (the point-to-point refinement), so that both apply one reflection rule.
#pragma once
#include "common.h"

namespace {

// One-sided Jacobi SVD of a 3x3 matrix A (row-major): A = U diag(S) V^T, S descending.
__device__ void svd3(const double A[9], double U[9], double S[3], double V[9])
{
    double B[9];   // columns get rotated until mutually orthogonal: B = A V
    for (int i = 0; i < 9; i++) { B[i] = A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < 3; i++) {
                    alpha += B[3 * i + p] * B[3 * i + p];
                    beta += B[3 * i + q] * B[3 * i + q];
                    gamma += B[3 * i + p] * B[3 * i + q];
                }
                if (gamma == 0.0) continue;
                off = fmax(off, fabs(gamma) / sqrt(fmax(alpha * beta, 1e-300)));
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; i++) {
                    const double bp = B[3 * i + p], bq = B[3 * i + q];
                    B[3 * i + p] = c * bp - s * bq; B[3 * i + q] = s * bp + c * bq;
                    const double vp = V[3 * i + p], vq = V[3 * i + q];
                    V[3 * i + p] = c * vp - s * vq; V[3 * i + q] = s * vp + c * vq;
                }
            }
        if (off < 1e-15) break;
    }
    double n[3];
    for (int j = 0; j < 3; j++) n[j] = sqrt(B[j] * B[j] + B[3 + j] * B[3 + j] + B[6 + j] * B[6 + j]);
    int ord[3] = {0, 1, 2};   // sort columns by singular value, descending
    for (int a = 0; a < 2; a++)
        for (int b = a + 1; b < 3; b++)
            if (n[ord[b]] > n[ord[a]]) { int t = ord[a]; ord[a] = ord[b]; ord[b] = t; }
    double Vs[9];
    for (int j = 0; j < 3; j++) {
        S[j] = n[ord[j]];
        for (int i = 0; i < 3; i++) { Vs[3 * i + j] = V[3 * i + ord[j]]; U[3 * i + j] = B[3 * i + ord[j]]; }
    }
    for (int i = 0; i < 9; i++) V[i] = Vs[i];
    // normalise U; rebuild (near-)null directions so U stays orthonormal
    const double tiny = 1e-300 + 1e-14 * S[0];
    if (S[0] <= tiny) {
        // a zero covariance (one point, coincident points, all weights 0): U = V = I as LAPACK returns for a zero matrix, so that
        // R = I and t = cb - ca as in the reference.  Completing U from e0 would give a 90-degree turn about x instead.
        for (int i = 0; i < 9; i++) U[i] = V[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    for (int i = 0; i < 3; i++) U[3 * i] /= S[0];
    if (S[1] > tiny) for (int i = 0; i < 3; i++) U[3 * i + 1] /= S[1];
    else {   // any unit vector orthogonal to u0
        const double u0[3] = {U[0], U[3], U[6]};
        int m = fabs(u0[0]) < fabs(u0[1]) ? (fabs(u0[0]) < fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) < fabs(u0[2]) ? 1 : 2);
        double a[3] = {0, 0, 0};
        a[m] = 1.0;
        const double d = a[0] * u0[0] + a[1] * u0[1] + a[2] * u0[2];
        double e[3], nn = 0;
        for (int i = 0; i < 3; i++) { e[i] = a[i] - d * u0[i]; nn += e[i] * e[i]; }
        nn = sqrt(nn);
        for (int i = 0; i < 3; i++) U[3 * i + 1] = e[i] / nn;
    }
    {
        // third column: u2 = +-(u0 x u1), sign agreeing with A v2 (so that S[2] >= 0)
        const double u0[3] = {U[0], U[3], U[6]}, u1[3] = {U[1], U[4], U[7]};
        double c[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
        const double dot = c[0] * U[2] + c[1] * U[5] + c[2] * U[8];
        const double sg = dot < 0 ? -1.0 : 1.0;
        for (int i = 0; i < 3; i++) U[3 * i + 2] = sg * c[i];
    }
}

// cov = U S V^T -> R = V diag(1, 1, d) U^T with d = +1, or -1 when det(V U^T) <= 0 (flip V[:, 2]; se3_torch.py:143-148).  One lane.
__device__ __forceinline__ double pro_rotation(const double cov[9], double U[9], double S[3], double V[9], double R[9])
{
    svd3(cov, U, S, V);
    auto vut = [&](double sgn) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++)
                R[3 * r + c] = V[3 * r] * U[3 * c] + V[3 * r + 1] * U[3 * c + 1] + sgn * V[3 * r + 2] * U[3 * c + 2];
    };
    vut(1.0);
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                       R[2] * (R[3] * R[7] - R[4] * R[6]);
    double d = 1.0;
    if (!(det > 0)) { vut(-1.0); d = -1.0; }
    return d;
}

}  // namespace
