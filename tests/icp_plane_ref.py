"""Numpy restatement of regtr_amd.refine.estimate_normals and of point-to-plane ICP (csrc/icp_plane.hip), written from their definitions:
the oracle of tests/test_icp_plane_host.py and tests/test_gpu_icp_plane.py.  The transform and the match are tests/icp_ref.py's.

    qscale / moments     s = the largest integer with radius 2^s <= 2^20; per point the int64 sums n | sum dq (3) | sum dq dq^T (6) of
                         dq = rint((q - p) 2^s) over the points q of the cloud with float64 d2 = (dx dx + dy dy) + dz dz < radius^2
    covariance           m = S1 / n, C_ab = S2_ab / n - m_a m_b in float64 (one division, one product, one subtraction per entry)
    normals              np.linalg.eigh of C: l0 <= l1 <= l2, the eigenvector of l0 rounded to float32; valid = n >= 3 and l1 > 2^-40 l2
    plane_sums / solve   r = nrm . (y - q), J = [y x nrm, nrm], A = sum J^T J, g = sum J^T r; D = diag(A)^-1/2, LDL^T of D A D without
                         pivoting, stop on a pivot <= 2^-23, x = -D (D A D)^-1 D g
    compose              pose64 <- (Rz(x2) Ry(x1) Rx(x0), x[3:6]) pose64
    icp_plane            the loop with the stop rule, keeping every iteration's record
    step_bound           the DERIVED bound on one step's pose (below); normal_angle_bound / eigen_residual_bound for the normals

The normals' bounds.  The moments are integers: kernel and restatement agree exactly, and so does C (the same three float64 operations
per entry).  What differs is the eigen-solver: a backward-stable one returns the exact eigenvector of C + E, ||E|| <= c u ||C||, which
is within ||E|| / (l1 - l0) (radians, first order: Davis-Kahan) of C's own; both sides carry one, c = 32 each:
    angle <= 64 u64 l2 / (l1 - l0) + 2 sqrt(3) 2^-24                (the second term: both normals are rounded to float32 per entry)
    ||C n - l0 n|| <= 64 u64 ||C|| + 2^-23 ||C||                    (the float32 rounding of n moves C n by at most sqrt(3) 2^-24 ||C||)
Against unquantised doubles: with q = 2^-s, |dq q - d| <= q / 2 per axis, so a product of two differences moves by at most
2 radius q / 2 + q^2 / 4 and a covariance entry by dC = 4 radius q / 2 + q^2 / 2 (the mean of products and the product of means both
move); nine entries: angle <= 3 dC / (l1 - l0).

The bound of one step.  Both sides form A = sum J^T J and g = sum J^T r over the same matches with the same float64 J and r, in
different orders: entry (i, j) is within 2 (n + 8) u64 sum |J_i J_j| of the other side's (icp_ref: any order is within (n - 1) u of the
exact sum).  With D = diag(A)^-1/2, As = D A D (unit diagonal), gs = D g, z = -As^-1 gs and x = D z:
    E_ij = 2 (n + 8) u D_i D_j sum |J_i J_j|,  e_i = 2 (n + 8) u D_i sum |J_i r|
    ||dz|| <= (||e|| + ||E||_F ||z||) / lmin / (1 - ||E||_F / lmin) + 64 u (lmax / lmin) ||z||
(the standard perturbation bound of a linear system, lmin / lmax the extreme eigenvalues of the restatement's own As; the last term is
the backward error of two 6 x 6 LDL^T solves whose pivots exceed 2^-23), |dx_i| <= D_i ||dz||.  The rotation dR = Rz Ry Rx has
derivatives of at most 1 per angle and entry, so no entry moves by more than dth = |dx_0| + |dx_1| + |dx_2| + 16 u (the last for two
libraries' sin and cos).  The new pose Q = dT P then moves by
    |dQ_rc| <= dth sum_k |P_kc| + [c = 3] |dx_(3 + r)| + 8 u (sum_k |P_kc| + |x_(3 + r)|)
and its float32 rounding adds 2^-24 |Q_rc|.  Over a loop with equal matches the float64 master poses drift apart by the sum of the
steps' bounds (a rotation does not amplify what it is applied to); icp_plane accumulates that sum in `drift`.
Against the ground truth of targets that are ROUNDED images of the source rows (|q_i - (R p_i + t)| <= noise per axis): at the ground
truth every residual is at most |r_i| <= sqrt(3) (noise + dy), dy the rounding of the float32 transform, whatever the normal, and
z = -(Js^T Js)^-1 Js^T r (Js = J D, the stacked scaled Jacobian, whose pseudo-inverse has norm 1 / sqrt(lmin)) moves by at most
||r|| / sqrt(lmin) <= sqrt(n_sys) sqrt(3) (noise + dy) / sqrt(lmin); the linearisation adds the square of the last step,
2 ||x||^2 (1 + max |y|).
"""
import numpy as np

from tests import icp_ref as R

U64 = 2.0 ** -53
U32 = 2.0 ** -24
NSUMS = 30           # n | sum d2 | n_sys | 21 | 6 per chunk


def qscale(radius):
    """2^s, s the largest integer with radius 2^s <= 2^20."""
    m, e = np.frexp(float(radius))
    return float(np.ldexp(1.0, (21 if m == 0.5 else 20) - int(e)))


def neighbours(xyz, radius, block=256):
    """Per point the index arrays of the cloud's points with float64 d2 = (dx dx + dy dy) + dz dz < radius^2 (itself included)."""
    p = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    r2 = float(radius) * float(radius)
    cand = None
    if len(p) > 4000:      # candidates from a KD-tree, the decision by the stated arithmetic
        from scipy.spatial import cKDTree
        cand = cKDTree(p).query_ball_point(p, float(radius) * (1 + 1e-9))
    out = []
    for s in range(0, len(p), block):
        if cand is not None:
            for i in range(s, min(s + block, len(p))):
                j = np.sort(np.asarray(cand[i], dtype=np.int64))
                d = p[j] - p[i]
                out.append(j[(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] < r2])
            continue
        d = p[None, :, :] - p[s:s + block, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        out.extend(np.nonzero(row)[0] for row in d2 < r2)
    return out


def moments(xyz, radius, nbrs=None):
    """(N, 10) int64: n | sum dq (3) | sum dq dq^T (xx xy xz yy yz zz) of one cloud."""
    p = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    nbrs = neighbours(xyz, radius) if nbrs is None else nbrs
    sc = qscale(radius)
    m = np.zeros((len(p), 10), dtype=np.int64)
    for i, j in enumerate(nbrs):
        dq = np.rint((p[j] - p[i]) * sc).astype(np.int64)
        m[i, 0] = len(j)
        m[i, 1:4] = dq.sum(0)
        m[i, 4:] = [(dq[:, a] * dq[:, b]).sum() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return m


def covariance(m):
    """(N, 3, 3) float64 from the int64 moments: mean = S1 / n, C_ab = S2_ab / n - mean_a mean_b; zeros where n = 0."""
    n = np.maximum(m[:, 0], 1).astype(np.float64)
    mean = m[:, 1:4].astype(np.float64) / n[:, None]
    C = np.zeros((len(m), 3, 3))
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[:, a, b] = C[:, b, a] = m[:, 4 + k].astype(np.float64) / n - mean[:, a] * mean[:, b]
    return C


def normals(xyz, radius, nbrs=None):
    """One cloud -> dict(normals (N, 3) float32, valid (N,) int32, moments (N, 10) int64, C (N, 3, 3), lam (N, 3) ascending)."""
    m = moments(xyz, radius, nbrs)
    C = covariance(m)
    lam, vec = np.linalg.eigh(C)
    valid = (m[:, 0] >= 3) & (lam[:, 1] > 2.0 ** -40 * lam[:, 2])
    nrm = np.where(valid[:, None], vec[:, :, 0], 0.0).astype(np.float32)
    return {'normals': nrm, 'valid': valid.astype(np.int32), 'moments': m, 'C': C, 'lam': lam}


def angle(a, b):
    """The angle between the LINES along a and b ((n, 3) each), accurate near 0 (arccos of a dot product is not): atan2(|a x b|, |a . b|)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(-1)))


def normal_angle_bound(lam):
    with np.errstate(divide='ignore'):
        return 64 * U64 * lam[:, 2] / (lam[:, 1] - lam[:, 0]) + 2 * np.sqrt(3) * U32


def eigen_residual_bound(C):
    nC = np.linalg.norm(C, axis=(1, 2))
    return 64 * U64 * nC + 2.0 ** -23 * nC


def quantisation_angle_bound(lam, radius):
    """lam: eigenvalues of the quantised covariance (in quanta^2) -> the angle to the normal of unquantised doubles."""
    q = 1.0 / qscale(radius)
    dC = 4 * radius * q / 2 + q * q / 2
    with np.errstate(divide='ignore'):
        return 3 * dC / ((lam[:, 1] - lam[:, 0]) * q * q)


# ------------------------------------------------------------------------------------------------------------------ one step
def plane_sums(y, tgt, idx, d2, nrm, valid):
    """y (n, 3) float32 transformed source rows, idx / d2 their matches -> dict of the float64 sums and of the sums of magnitudes."""
    hit = idx >= 0
    use = hit.copy()
    use[hit] = np.asarray(valid)[idx[hit]] != 0
    Y = np.asarray(y, dtype=np.float32).astype(np.float64)[use]
    q = np.asarray(tgt, dtype=np.float32).astype(np.float64)[idx[use]] if use.any() else np.zeros((0, 3))
    N = np.asarray(nrm, dtype=np.float32).astype(np.float64)[idx[use]] if use.any() else np.zeros((0, 3))
    d = Y - q
    r = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2]
    J = np.concatenate([np.cross(Y, N), N], axis=1) if len(Y) else np.zeros((0, 6))
    return {'n': int(hit.sum()), 'sd2': float(d2[hit].sum()), 'n_sys': int(use.sum()), 'A': J.T @ J, 'g': J.T @ r,
            'Aabs': np.abs(J).T @ np.abs(J), 'gabs': np.abs(J).T @ np.abs(r),
            'ymax': float(np.abs(Y).max()) if len(Y) else 0.0}


def plane_solve(s):
    """-> dict(stop, x (6,) | None, D, As, pivots, lmin, lmax, z): stop on n_sys < 6, a non-positive diagonal, or a pivot <= 2^-23 of
    the LDL^T (no pivoting) of the system scaled to unit diagonal."""
    out = {'stop': True, 'x': None}
    if s['n_sys'] < 6 or not np.all(np.diag(s['A']) > 0):
        return out
    D = 1.0 / np.sqrt(np.diag(s['A']))
    As = (s['A'] * D[:, None]) * D[None, :]
    L, piv = np.eye(6), np.zeros(6)
    for j in range(6):
        piv[j] = As[j, j] - sum(L[j, k] * L[j, k] * piv[k] for k in range(j))
        if not piv[j] > 2.0 ** -23:
            out['pivots'] = piv[:j + 1]
            return out
        for i in range(j + 1, 6):
            L[i, j] = (As[i, j] - sum(L[i, k] * L[j, k] * piv[k] for k in range(j))) / piv[j]
    z = np.linalg.solve(L, -(s['g'] * D))
    z = np.linalg.solve(L.T, z / piv)
    ev = np.linalg.eigvalsh(As)
    return {'stop': False, 'x': z * D, 'z': z, 'D': D, 'As': As, 'pivots': piv, 'lmin': float(ev[0]), 'lmax': float(ev[-1])}


def delta(x):
    """(3, 4) float64: (Rz(x2) Ry(x1) Rx(x0), x[3:6]), Open3D's TransformVector6dToMatrix4d."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rm = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                   [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                   [-sb, cb * sa, cb * ca]])
    return np.concatenate([Rm, np.asarray(x[3:6], dtype=np.float64)[:, None]], axis=1)


def compose(dT, P):
    return np.concatenate([dT[:, :3] @ P[:, :3], (dT[:, :3] @ P[:, 3] + dT[:, 3])[:, None]], axis=1)


def step_bound(s, sol, P_prev, Q, target_noise=None, dy=0.0):
    """(3, 4): the derived bound (module docstring) on |float32 pose of the kernel - float64 pose Q of the restatement| for one step
    from the same master pose P_prev; with target_noise the bound against the ground truth instead (rounded-image targets)."""
    n, D = s['n_sys'], sol['D']
    k = 2 * (n + 8) * U64
    E = np.linalg.norm(k * s['Aabs'] * D[:, None] * D[None, :])
    e = k * s['gabs'] * D
    second = 0.0
    if target_noise is not None:
        second = 2 * float(sol['x'] @ sol['x']) * (1 + s['ymax'])
    zn = np.linalg.norm(sol['z'])
    dz = (np.linalg.norm(e) + E * zn) / sol['lmin'] / (1 - E / sol['lmin']) + 64 * U64 * sol['lmax'] / sol['lmin'] * zn
    if target_noise is not None:
        dz += np.sqrt(n) * np.sqrt(3) * (target_noise + dy) / np.sqrt(sol['lmin'])
    dx = D * dz + second
    dth = dx[:3].sum() + 16 * U64
    col = np.abs(P_prev).sum(0)
    b = dth * np.tile(col, (3, 1)) + 8 * U64 * (np.tile(col, (3, 1)))
    b[:, 3] += dx[3:] + 8 * U64 * np.abs(sol['x'][3:])
    return b + U32 * (np.abs(Q) + b)


def icp_plane(src, tgt, pose0, max_dist, nrm, valid, iters=30, rel_fitness=1e-6, rel_rmse=1e-6, margins=False, nearest=None):
    """One pair.  -> dict as icp_ref.icp, with pose64 the float64 master pose (None if never updated), last_s / last_sol / last_prev the
    sums, solve and master pose of the last update, drift (3, 4) the sum of the steps' bounds, and per pass k history[k] = dict(n, n_sys,
    fitness, rmse, idx, stop_margin, gap2 / gap_r minima with margins=True).  nearest: a replacement for icp_ref.nearest with its
    signature (kd_nearest for large clouds)."""
    src = np.asarray(src, dtype=np.float32)
    tgt = np.asarray(tgt, dtype=np.float32)
    pose = np.asarray(pose0, dtype=np.float32)[:3, :].copy()
    P64 = pose.astype(np.float64)
    out = {'pose64': None, 'history': [], 'iters_run': 0, 'last_s': None, 'last_sol': None, 'last_prev': None, 'drift': np.zeros((3, 4))}
    prev = None
    done = False
    for k in range(iters + 1):
        y = R.transform_f32(pose, src)
        with np.errstate(invalid='ignore', over='ignore'):
            res = (nearest or R.nearest)(y, tgt, max_dist, margins=margins)
        idx, d2 = res[0], res[1]
        s = plane_sums(y, tgt, idx, d2, nrm, valid)
        fit = s['n'] / len(src) if len(src) else 0.0
        rmse = float(np.sqrt(s['sd2'] / s['n'])) if s['n'] > 0 else 0.0
        rec = {'n': s['n'], 'n_sys': s['n_sys'], 'fitness': fit, 'rmse': rmse, 'idx': idx}
        if margins:
            rec['gap2'], rec['gap_r'] = (float(res[2].min()) if len(src) else np.inf), (float(res[3].min()) if len(src) else np.inf)
            rec['gap_rows'] = np.minimum(res[2], res[3])          # per row: how far its match is from another decision
        out.update(fitness=fit, inlier_rmse=rmse, n_inliers=s['n'], idx=idx, d2=d2)
        out['history'].append(rec)
        if k == iters:
            break
        stop = s['n_sys'] < 6 or not np.isfinite(pose).all()
        if k > 0:
            df, dr = abs(fit - prev[0]), abs(rmse - prev[1])
            rec['stop_margin'] = (abs(df - rel_fitness), abs(dr - rel_rmse))
            stop = stop or (df < rel_fitness and dr < rel_rmse)
        if not stop:
            sol = plane_solve(s)
            stop = sol['stop']
            rec['pivot_min'] = float(np.min(sol['pivots'])) if 'pivots' in sol else None
        if stop:
            done = True
            break
        Q = compose(delta(sol['x']), P64)
        out['drift'] = out['drift'] + step_bound(s, sol, P64, Q) - U32 * np.abs(Q)
        out.update(last_s=s, last_sol=sol, last_prev=P64, pose64=Q, iters_run=k + 1)
        P64 = Q
        pose = Q.astype(np.float32)
        prev = (fit, rmse)
    out['pose'], out['done'] = pose, done
    return out


def loop_bound(o):
    """(3, 4): the bound on |float32 pose of the kernel's loop - o['pose64']| when every pass made the restatement's matches."""
    return o['drift'] + U32 * (np.abs(o['pose64']) + o['drift'])


def kd_nearest(y, tgt, max_dist, margins=False):
    """icp_ref.nearest for large clouds, with its results: the eight nearest candidates from a KD-tree, every decision and margin by the
    stated float64 arithmetic on them (ties to the lower index; the second-best of all targets is among eight candidates)."""
    from scipy.spatial import cKDTree
    y64, t64 = np.asarray(y, dtype=np.float32).astype(np.float64), np.asarray(tgt, dtype=np.float32).astype(np.float64)
    assert len(t64) >= 8 and np.isfinite(y64).all()
    _, j = cKDTree(t64).query(y64, k=8)
    j = np.sort(j, axis=1)
    d = y64[:, None, :] - t64[j]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    k = np.argmin(d2, axis=1)
    best = d2[np.arange(len(k)), k]
    r2 = float(max_dist) * float(max_dist)
    hit = best < r2
    idx, d2o = np.where(hit, j[np.arange(len(k)), k], -1).astype(np.int32), np.where(hit, best, np.inf)
    if not margins:
        return idx, d2o
    part = np.partition(d2, 1, axis=1)
    return idx, d2o, np.where(part[:, 0] < r2, part[:, 1] - part[:, 0], np.inf), np.abs(best - r2)


# ------------------------------------------------------------------------------------------------------------------ test clouds
def plane_patch(nu, nv, spacing, seed, origin, eu, ev, jitter=0.3):
    """nu x nv float64 points on the plane origin + a eu + b ev, one per lattice cell, jittered inside the plane."""
    rng = np.random.RandomState(seed)
    a, b = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    ab = np.stack([a.ravel(), b.ravel()], 1) + 0.5 + rng.uniform(-jitter, jitter, size=(nu * nv, 2))
    return np.asarray(origin, dtype=np.float64) + spacing * (ab[:, :1] * np.asarray(eu, dtype=np.float64) + ab[:, 1:] * np.asarray(ev, dtype=np.float64))


def box_corner(n_side, spacing, seed, gt):
    """Three mutually orthogonal faces meeting in a corner.  -> src (float32), tgt = the float32-rounded images gt src in a shuffled
    order, perm (tgt row of source row i), noise = max |tgt[perm] - gt src| with src taken as its float32 values."""
    faces = [plane_patch(n_side, n_side, spacing, seed + 0, (0.2, -0.1, 0.3), (1, 0, 0), (0, 1, 0)),
             plane_patch(n_side, n_side, spacing, seed + 1, (0.2, -0.1, 0.3), (1, 0, 0), (0, 0, 1)),
             plane_patch(n_side, n_side, spacing, seed + 2, (0.2, -0.1, 0.3), (0, 1, 0), (0, 0, 1))]
    src = np.concatenate(faces).astype(np.float32)
    img64 = src.astype(np.float64) @ gt[:, :3].T + gt[:, 3]
    img = img64.astype(np.float32)
    order = np.random.RandomState(seed + 99).permutation(len(src))
    perm = np.empty(len(src), dtype=np.int64)
    perm[order] = np.arange(len(src))
    return src, img[order], perm, float(np.abs(img.astype(np.float64) - img64).max())
