"""Numpy restatement of regtr_amd.refine.icp (csrc/icp.hip), written from the definition of point-to-point ICP and of Open3D's
evaluate_registration: the oracle of tests/test_icp_host.py and tests/test_gpu_icp.py.

    transform_f32      y = ((r0 x + r1 y) + r2 z) + t, float32 rounded per operation (regtr_se3_transform's arithmetic)
    nearest            brute force, float64 on the widened float32 coordinates, d2 = (dx dx + dy dy) + dz dz, strict d2 < max_dist^2,
                       ties to the lower index; with the MARGINS that tell whether rounding could change a decision
    moments / solve    the float64 sums and the Kabsch fit through np.linalg.svd, the reflection on the smallest singular value
    icp                the loop with the stop rule, keeping every iteration's record
    pose_bound         the DERIVED bound on one solve's float32 pose against the float64 fit (below)

The bound.  The kernel and this file fit the same matched rows, the original source points p_i and their matches q_i, so a pose
depends on the iteration only through the matches: with equal matches the error of the final pose is the error of ONE solve.
  * Sums.  Both sides add n products of magnitude <= M = max |p_r q_c| (or max |p|, max |q|) in float64, in different orders.  Any
    order is within (n - 1) u M n of the exact sum, u = 2^-53; mean and covariance entries therefore differ by at most
    dcov = 2 (n + 8) u (M + max|p| max|q|)  (the products themselves and the centroid product add a few u M: the `+ 8`).
  * Rotation.  For cov = U diag(S) V^T and lam = (S0, S1, d S2), a perturbation E of cov turns the fitted rotation, to first order,
    by R (I + V Y V^T) with Y antisymmetric, Y_jk = -A_jk / (lam_j + lam_k), A = V^T (R E - E^T R^T) V -- the closed form that
    regtr_weighted_procrustes_bwd differentiates.  ||A||_F <= 2 ||E||_F, so ||Y||_F <= 2 ||E||_F / min (lam_j + lam_k), and no entry
    of R moves by more than ||Y||_F.  With ||E||_F <= 3 dcov (nine entries of at most dcov):
        c = 6 dcov / lmin,  lmin = min (lam_i + lam_j)              (the conditioning term, from this file's own singular values)
    The one-sided Jacobi SVD of the kernel and LAPACK's both return R to a few u / (lmin / S0); 64 u S0 / lmin is added for them.
  * Rounding to float32: |R_ij| <= 1 rounds by at most 2^-24 (1 + c), t_i by 2^-24 |t_i|.
  * Translation t = qbar - R pbar: |dt_i| <= c ||pbar||_1 + 4 u (|qbar| + |pbar|) + the rounding.
  * Noise in the targets (tgt rows that are ROUNDED images of the source rows, |q_i - (R p_i + t)| <= noise): a fit to them is not the
    ground truth; E gains noise * mean |p - pbar| per entry and t up to `noise`.  target_noise = 0 compares kernel and restatement.
So R is bounded by about one float32 rounding, 6e-8, plus c (1e-12 .. 1e-9 on the test clouds), per entry.
"""
import numpy as np

U64 = 2.0 ** -53
U32 = 2.0 ** -24


def transform_f32(pose, xyz):
    """pose (3, 4) or (12,), xyz (n, 3) float32 -> (n, 3) float32, rounded per operation."""
    T = np.asarray(pose, dtype=np.float32).reshape(3, 4)
    x, y, z = (np.asarray(xyz, dtype=np.float32)[:, k] for k in range(3))
    out = np.empty((len(x), 3), dtype=np.float32)
    for r in range(3):
        out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    assert out.dtype == np.float32
    return out


def nearest(y, tgt, max_dist, block=512, margins=False):
    """-> idx (n,) int32 (-1: empty ball), d2 (n,) float64 (inf: empty)[, gap2 (n,): second-best d2 minus best among ALL targets (inf
    with fewer than two, and where even the best is outside the ball: no match either way), gap_r (n,): |best d2 over all targets - max_dist^2|].  Ties: np.argmin keeps the first = lowest index."""
    y64, t64 = np.asarray(y, dtype=np.float32).astype(np.float64), np.asarray(tgt, dtype=np.float32).astype(np.float64)
    n, r2 = len(y64), float(max_dist) * float(max_dist)
    idx = np.full(n, -1, dtype=np.int32)
    d2o = np.full(n, np.inf)
    gap2, gap_r = np.full(n, np.inf), np.full(n, np.inf)
    if len(t64) == 0:
        return (idx, d2o, gap2, gap_r) if margins else (idx, d2o)
    for s in range(0, n, block):
        d = y64[s:s + block, None, :] - t64[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        with np.errstate(invalid='ignore'):
            j = np.argmin(np.where(np.isnan(d2), np.inf, d2), axis=1)
        best = d2[np.arange(len(j)), j]
        hit = best < r2            # (NaN compares false: a non-finite query matches nothing)
        idx[s:s + block] = np.where(hit, j, -1)
        d2o[s:s + block] = np.where(hit, best, np.inf)
        if margins:
            if d2.shape[1] > 1:
                part = np.partition(d2, 1, axis=1)
                gap2[s:s + block] = np.where(part[:, 0] < r2, part[:, 1] - part[:, 0], np.inf)
            gap_r[s:s + block] = np.abs(best - r2)
    return (idx, d2o, gap2, gap_r) if margins else (idx, d2o)


def moments(src, tgt, idx, d2):
    """float64: n, sum d2, sum p (3), sum q (3), sum p q^T (3, 3) over the matched rows; p the original source point."""
    hit = idx >= 0
    p = np.asarray(src, dtype=np.float32).astype(np.float64)[hit]
    q = np.asarray(tgt, dtype=np.float32).astype(np.float64)[idx[hit]] if hit.any() else np.zeros((0, 3))
    return {'n': int(hit.sum()), 'sd2': float(d2[hit].sum()), 'sp': p.sum(0), 'sq': q.sum(0), 'spq': p.T @ q,
            'pmax': float(np.abs(p).max()) if len(p) else 0.0, 'qmax': float(np.abs(q).max()) if len(q) else 0.0,
            'pdev': float(np.abs(p - p.mean(0)).mean()) if len(p) else 0.0,
            'pdmax': float(np.abs(p - p.mean(0)).max()) if len(p) else 0.0, 'qdmax': float(np.abs(q - q.mean(0)).max()) if len(q) else 0.0}


def stats_of(m, n_src):
    n = m['n']
    return (n / n_src if n_src > 0 else 0.0), (float(np.sqrt(m['sd2'] / n)) if n > 0 else 0.0)


def solve(m):
    """-> dict(pose (3, 4) float64, S (3,), d, lmin, degenerate): cov = sum p q^T / n - pbar qbar^T = U S V^T, R = V diag(1, 1, d) U^T,
    d = -1 when det(V U^T) <= 0; t = qbar - R pbar; degenerate when min (lam_i + lam_j) <= 2^-23 lam_0, lam = (S0, S1, d S2)."""
    n = m['n']
    pb, qb = m['sp'] / n, m['sq'] / n
    cov = m['spq'] / n - np.outer(pb, qb)
    Um, S, Vt = np.linalg.svd(cov)
    V = Vt.T
    d = 1.0 if np.linalg.det(V @ Um.T) > 0 else -1.0
    R = V @ np.diag([1.0, 1.0, d]) @ Um.T
    lam = np.array([S[0], S[1], d * S[2]])
    lmin = min(lam[0] + lam[1], lam[0] + lam[2], lam[1] + lam[2])
    return {'pose': np.concatenate([R, (qb - R @ pb)[:, None]], axis=1), 'S': S, 'd': d, 'lmin': lmin, 'pbar': pb, 'qbar': qb,
            'degenerate': not (lmin > 2.0 ** -23 * lam[0])}


def pose_bound(m, sol, target_noise=0.0):
    """(3, 4) float64: the derived bound (module docstring) on |float32 pose of the kernel - float64 pose of `sol`| per entry; with
    target_noise > 0 the bound against the ground truth of targets that are rounded images of the source rows."""
    n = m['n']
    M = m['pmax'] * m['qmax']
    dcov = 2 * (n + 8) * U64 * 2 * M + target_noise * m['pdev']
    c = 6 * dcov / sol['lmin'] + 64 * U64 * sol['S'][0] / sol['lmin']
    P = sol['pose']
    b = np.empty((3, 4))
    b[:, :3] = U32 * (1 + c) + c
    dt = c * np.abs(sol['pbar']).sum() + 4 * U64 * (np.abs(sol['qbar']).max() + np.abs(sol['pbar']).max()) + target_noise
    b[:, 3] = U32 * (np.abs(P[:, 3]) + dt) + dt
    return b


def composed_bound(m, sol):
    """(3, 4): the bound on |pose of the COMPOSED path - float64 pose of `sol`|.  That path fits the same matches through the pose head's
    kernel (regtr_weighted_procrustes), whose moments are float32 products summed in float64: wn = 1 / n, a centroid term a wn, the
    deviations a - ca and b - cb from centroids ROUNDED to float32, and (a - ca) ((b - cb) wn) each round once, u = 2^-24 relative.
    A covariance term therefore carries at most 5 u of itself, |a - ca| |b - cb| wn <= pdmax qdmax wn, and the rounded centroids
    shift every deviation by u |ca| or u |cb|: dcov32 = u (5 pdmax qdmax + pmax qdmax + qmax pdmax) (+ the float64 terms of pose_bound).
    The conditioning factor is pose_bound's; t = cb - R ca from the rounded centroids adds 2 u (|ca|_1 + |cb|_inf)."""
    dcov = U32 * (5 * m['pdmax'] * m['qdmax'] + m['pmax'] * m['qdmax'] + m['qmax'] * m['pdmax'])
    c = 6 * dcov / sol['lmin']
    b = pose_bound(m, sol)
    b[:, :3] += c
    b[:, 3] += c * np.abs(sol['pbar']).sum() + 2 * U32 * (np.abs(sol['pbar']).sum() + np.abs(sol['qbar']).max())
    return b


def match_margin_needed(src, pose, max_dist):
    """How far a one-ulp difference in every entry of a float32 pose can move a d2: the transformed point moves by at most
    dy = 2^-23 (max ||p||_1 + max |t|) per axis (each entry of R, at most 1, and of t off by one ulp, plus the three roundings of the
    sum), and d2 = |y - q|^2 with |y - q| < max_dist + sqrt(3) dy by 2 sqrt(3) dy (max_dist + sqrt(3) dy).  A decision whose margin
    (best against second-best d2, best d2 against max_dist^2) exceeds this is the same for both poses."""
    p = np.abs(np.asarray(src, dtype=np.float64))
    t = np.abs(np.asarray(pose, dtype=np.float64)[:3, 3]).max()
    dy = 2.0 ** -23 * ((p.sum(1).max() if len(p) else 0.0) + t) * 2
    return 2 * np.sqrt(3) * dy * (max_dist + np.sqrt(3) * dy)


def icp(src, tgt, pose0, max_dist, iters=30, rel_fitness=1e-6, rel_rmse=1e-6, margins=False):
    """One pair.  -> dict: pose (3, 4) float32 returned, pose64 (the float64 fit it was rounded from, None if never updated),
    fitness, inlier_rmse, n_inliers, iters_run, idx / d2 of the returned pose, history: per pass k the dict(n, fitness, rmse, idx,
    stop_margin = (| |dfit| - rel_fitness |, | |drmse| - rel_rmse |) for k > 0, gap2 / gap_r minima with margins=True), last_m / last_sol:
    moments and solve of the last update (for pose_bound)."""
    src = np.asarray(src, dtype=np.float32)
    tgt = np.asarray(tgt, dtype=np.float32)
    pose = np.asarray(pose0, dtype=np.float32)[:3, :].copy()
    out = {'pose64': None, 'history': [], 'iters_run': 0, 'last_m': None, 'last_sol': None}
    prev = None
    done = False
    for k in range(iters + 1):
        y = transform_f32(pose, src)
        with np.errstate(invalid='ignore', over='ignore'):
            res = nearest(y, tgt, max_dist, margins=margins)
        idx, d2 = res[0], res[1]
        m = moments(src, tgt, idx, d2)
        fit, rmse = stats_of(m, len(src))
        rec = {'n': m['n'], 'fitness': fit, 'rmse': rmse, 'idx': idx}
        if margins:
            rec['gap2'], rec['gap_r'] = (float(res[2].min()) if len(src) else np.inf), (float(res[3].min()) if len(src) else np.inf)
        out.update(fitness=fit, inlier_rmse=rmse, n_inliers=m['n'], idx=idx, d2=d2)
        out['history'].append(rec)
        if k == iters:
            break
        stop = m['n'] < 3 or not np.isfinite(pose).all()
        if k > 0:
            df, dr = abs(fit - prev[0]), abs(rmse - prev[1])
            rec['stop_margin'] = (abs(df - rel_fitness), abs(dr - rel_rmse))
            stop = stop or (df < rel_fitness and dr < rel_rmse)
        if not stop:
            sol = solve(m)
            stop = sol['degenerate']
        if stop:
            done = True
            break
        pose = sol['pose'].astype(np.float32)
        out.update(pose64=sol['pose'], last_m=m, last_sol=sol, iters_run=k + 1)
        prev = (fit, rmse)
    out['pose'], out['done'] = pose, done
    return out


# ------------------------------------------------------------------------------------------------------------------ test clouds
def rotation(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def pose_of(axis, deg, t):
    return np.concatenate([rotation(axis, deg), np.asarray(t, dtype=np.float64)[:, None]], axis=1)


def jittered_cloud(n, spacing, seed, jitter=0.3, origin=(0.0, 0.0, 0.0)):
    """n float32 points, one per cell of a cubic lattice (a random subset of the smallest cube of cells that holds n), each moved by up
    to jitter * spacing per axis: neighbours stay at least (1 - 2 jitter) spacing apart.  No two points coincide."""
    rng = np.random.RandomState(seed)
    side = int(np.ceil(max(n, 1) ** (1 / 3)))
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing='ij'), -1).reshape(-1, 3)
    cells = cells[rng.permutation(len(cells))[:n]]
    pts = (cells + 0.5 + rng.uniform(-jitter, jitter, size=(n, 3))) * spacing + np.asarray(origin)
    return pts.astype(np.float32)


def overlapping_pair(n, spacing, seed, gt, extra=0, jitter=0.3):
    """src: a jittered cloud; tgt: the float32-rounded images gt src of every source row, in a shuffled order, followed by `extra`
    points of a second cloud placed beyond the first (never nearer to an image than the images are to each other).  -> src, tgt,
    perm (tgt row of source row i), noise = max |tgt[perm] - gt src| (the rounding of the images)."""
    rng = np.random.RandomState(seed + 7919)
    src = jittered_cloud(n, spacing, seed, jitter)
    img64 = src.astype(np.float64) @ gt[:, :3].T + gt[:, 3]
    img = img64.astype(np.float32)
    order = rng.permutation(n)
    perm = np.empty(n, dtype=np.int64)
    perm[order] = np.arange(n)
    tgt = img[order]
    if extra:
        side = int(np.ceil(max(n, 1) ** (1 / 3)))
        far = jittered_cloud(extra, spacing, seed + 1, jitter, origin=((side + 3) * spacing, 0.0, 0.0)).astype(np.float64)
        tgt = np.concatenate([tgt, (far @ gt[:, :3].T + gt[:, 3]).astype(np.float32)])
    return src, tgt, perm, float(np.abs(img.astype(np.float64) - img64).max()) if n else 0.0


def perturbed(gt, axis, deg, dt):
    """gt composed with a small rotation about the origin-centred axis and a shift: (3, 4) float64."""
    R = rotation(axis, deg) @ gt[:, :3]
    return np.concatenate([R, (rotation(axis, deg) @ gt[:, 3] + np.asarray(dt))[:, None]], axis=1)


def pose_errors(pose, gt):
    """rotation error (degrees) and translation error of pose against gt, float64."""
    R = np.asarray(pose, dtype=np.float64)[:, :3] @ gt[:, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))
    return ang, float(np.linalg.norm(np.asarray(pose, dtype=np.float64)[:, 3] - gt[:, 3]))
