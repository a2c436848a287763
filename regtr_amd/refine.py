"""Pose refinement and registration fitness on the full-resolution clouds (csrc/icp.hip, csrc/icp_plane.hip; no reference counterpart).

    icp(src_list, tgt_list, pose0, max_dist, iters=30, ...)      point-to-point ICP from pose0: the polish of RegTR's coarse pose;
                                                                 method='point_to_plane': the residual along the target's normal
    estimate_normals(clouds, radius)                             per-point surface normals (bit-reproducible), Open3D's estimate_normals
    evaluate_registration(src_list, tgt_list, pose, max_dist)    Open3D-style fitness / inlier_rmse of a pose, no ground truth needed

One cell grid is built over the targets per call; every iteration is then one fused pass over the source rows and one per-pair solve
(regtr_icp_step), `iters + 1` steps enqueued on the current stream.  The stop rule runs on the device and nothing here synchronises.
`use_fused_icp(False)` routes the same iteration through the project's separate operators (ops.se3_transform, regtr_nearest_in_radius,
torch gathers and sums, se3.compute_rigid_transform): the A-B partner of tools/icp_bench.py and a second oracle for the tests.
"""
import collections
import math
import threading

import numpy as np
import torch

from . import _lib, ops, se3
from ._lib import bptr, check, dptr, iptr, ptr, stream

ICPResult = collections.namedtuple('ICPResult', 'pose fitness inlier_rmse n_inliers iters_run idx', defaults=(None,))

_route = threading.local()


def use_fused_icp(on=True):
    """A-B switch (thread-local): True (default) the fused kernels, False the composed form.  Returns the previous setting."""
    prev = getattr(_route, 'fused', True)
    _route.fused = bool(on)
    return prev


def __getattr__(name):
    if name == 'CHUNK':      # source rows per workgroup of the accumulate pass: a cloud of n rows has ceil(n / CHUNK) chunks
        return int(_lib.lib().regtr_icp_chunk())
    raise AttributeError(name)


def _pack(clouds, what):
    from .regtr import _packed_rows
    for c in clouds:
        if not isinstance(c, torch.Tensor) or c.device.type != 'cuda':
            raise RuntimeError(f'refine: {what} clouds must be GPU tensors (got {getattr(c, "device", type(c))}); there is no CPU fallback')
        if c.dim() != 2 or c.shape[1] != 3 or c.dtype is not torch.float32:
            raise RuntimeError(f'refine: {what} clouds must be (n, 3) float32, got {tuple(c.shape)} {c.dtype}')
    lens = [int(c.shape[0]) for c in clouds]
    xyz = _packed_rows(list(clouds)).contiguous()
    off = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    return xyz, torch.from_numpy(off).to(xyz.device, non_blocking=True), lens


def _pose12(pose, B, dev):
    if not isinstance(pose, torch.Tensor) or pose.device.type != 'cuda':
        raise RuntimeError(f'refine: the pose must be a GPU tensor (got {getattr(pose, "device", type(pose))}); there is no CPU fallback')
    if pose.dim() != 3 or pose.shape[0] != B or tuple(pose.shape[1:]) not in ((3, 4), (4, 4)):
        raise RuntimeError(f'refine: pose must be ({B}, 3, 4) or ({B}, 4, 4), got {tuple(pose.shape)}')
    return pose[:, :3, :].to(device=dev, dtype=torch.float32).reshape(B, 12).clone()      # refined in place; the caller's stays


METHODS = ('point_to_point', 'point_to_plane')


def estimate_normals(clouds, radius, return_moments=False):
    """Surface normals of (n, 3) float32 device clouds (regtr_estimate_normals): per point the eigenvector of the smallest eigenvalue of
    the covariance of the cloud's points closer than `radius` (strict; the point itself included), from exact integer moments, so two
    runs give the same bits.  -> (normals: list of (n, 3) float32, unit length or exactly 0, sign unspecified; valid: list of (n,) int32,
    0 with fewer than three neighbours or collinear ones[; moments: list of (n, 10) int64]): per-cloud views of packed tensors."""
    if not len(clouds) or not radius > 0:
        raise RuntimeError(f'refine.estimate_normals: at least one cloud and radius > 0 expected, got {len(clouds)}, {radius}')
    dev = clouds[0].device
    with _lib.on_device(dev):
        xyz, off, lens = _pack(clouds, 'the')
        r32 = float(np.float32(radius))
        r32 = r32 if r32 * (1 + 1e-6) >= radius else float(np.nextafter(np.float32(radius), np.float32(np.inf)))
        grid = ops.CellGrid(xyz, off, xyz.shape[0], r32) if xyz.shape[0] else None
        nrm, valid, mom = _normals_packed(xyz, off, grid, float(radius), r32, return_moments)
    cut = lambda t: list(torch.split(t, lens))
    return (cut(nrm), cut(valid), cut(mom)) if return_moments else (cut(nrm), cut(valid))


def _normals_packed(xyz, off, grid, radius, r32, want_moments=False):
    n, dev = xyz.shape[0], xyz.device
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.int32, device=dev)
    mom = torch.empty((n, 10), dtype=torch.int64, device=dev) if want_moments else None
    if n:
        check(_lib.lib().regtr_estimate_normals(ptr(xyz), iptr(off), n, off.numel() - 1, radius, r32, bptr(grid.ws), grid.nbytes, ptr(nrm),
                                                iptr(valid), mom.data_ptr() if want_moments else None, stream()), 'regtr_estimate_normals')
    return nrm, valid, mom


def icp(src_list, tgt_list, pose0, max_dist, iters=30, rel_fitness=1e-6, rel_rmse=1e-6, return_idx=False, method='point_to_point',
        tgt_normals=None, normal_radius=None):
    """ICP of B pairs; method 'point_to_point' (default) or 'point_to_plane' (the last paragraph).  Point to point:  src_list / tgt_list: (B) (n, 3) float32 device clouds, pose0 (B, 3, 4) or (B, 4, 4) with
    pose0 src ~ tgt, max_dist the correspondence distance.  Per iteration every source point, transformed by the pair's current pose,
    is matched to its nearest target point closer than max_dist (strict; float64 distances, ties to the lower index) and the pose is
    re-fitted to the matches of the ORIGINAL source points, so the result is the absolute pose.  A pair stops (Open3D's rule) when
    fitness and inlier_rmse both move by less than rel_fitness / rel_rmse between two iterations, and also with fewer than three
    matches, collinear matches or a non-finite pose; it then keeps its pose.
    Returns ICPResult(pose (B, 3, 4) f32, fitness (B,) f64 = matched / source points, inlier_rmse (B,) f64, n_inliers (B,) i32,
    iters_run (B,) i32 = pose updates applied[, idx (n_src,) i32: the packed match of every source row under the returned pose, -1 =
    none]) -- the stats are those of the returned pose; iters=0 is evaluate_registration.  Device tensors; nothing synchronises.
    method='point_to_plane' (regtr_icp_plane_step): the same matches, but every iteration minimises sum (n_q . (T y - q))^2 over the
    matches whose target q has a valid normal n_q, linearised as Open3D does, and composes the small motion onto a float64 master pose;
    a pair also stops with fewer than six such matches or a system that fixes no pose (one wall).  The targets' normals are estimated
    here with normal_radius (default max_dist) unless tgt_normals = (normals, valid), lists as estimate_normals returns them, is given."""
    if method not in METHODS:
        raise ValueError(f'refine.icp: method must be one of {METHODS}, got {method!r}')
    if len(src_list) != len(tgt_list) or not len(src_list):
        raise RuntimeError(f'refine.icp: as many source as target clouds, at least one (got {len(src_list)}, {len(tgt_list)})')
    if not max_dist > 0 or iters < 0:
        raise RuntimeError(f'refine.icp: max_dist > 0 and iters >= 0 expected, got {max_dist}, {iters}')
    B = len(src_list)
    dev = src_list[0].device
    with _lib.on_device(dev):
        src, s_off, s_len = _pack(src_list, 'source')
        tgt, t_off, _ = _pack(tgt_list, 'target')
        pose = _pose12(pose0, B, dev)
        r32 = float(np.float32(max_dist))      # the grid's radius, as overlap.nearest_in_radius builds it: r32 (1 + 1e-6) >= max_dist
        grid = ops.CellGrid(tgt, t_off, tgt.shape[0], r32)
        fused = getattr(_route, 'fused', True)
        if method == 'point_to_plane':
            nrm, valid = _target_normals(tgt, t_off, grid, r32, float(max_dist), tgt_normals, normal_radius)
            run = _icp_plane_fused if fused else _icp_plane_composed
            stats, iters_run, idx = run(src, s_off, s_len, tgt, t_off, grid, r32, nrm, valid, pose, float(max_dist), int(iters),
                                        float(rel_fitness), float(rel_rmse), return_idx)
            return ICPResult(pose.view(B, 3, 4), stats[:, 0], stats[:, 1], stats[:, 2].to(torch.int32), iters_run, idx)
        run = _icp_fused if fused else _icp_composed
        stats, iters_run, idx = run(src, s_off, s_len, tgt, t_off, grid, r32, pose, float(max_dist), int(iters), float(rel_fitness),
                                    float(rel_rmse), return_idx)
    return ICPResult(pose.view(B, 3, 4), stats[:, 0], stats[:, 1], stats[:, 2].to(torch.int32), iters_run, idx)


def evaluate_registration(src_list, tgt_list, pose, max_dist):
    """Open3D's evaluate_registration on the device: (fitness (B,) f64, inlier_rmse (B,) f64, n_inliers (B,) i32) of `pose`."""
    r = icp(src_list, tgt_list, pose, max_dist, iters=0)
    return r.fitness, r.inlier_rmse, r.n_inliers


def _icp_fused(src, s_off, s_len, tgt, t_off, grid, r32, pose, max_dist, iters, rel_fitness, rel_rmse, return_idx):
    L = _lib.lib()
    B, n_src, dev = len(s_len), src.shape[0], src.device
    max_len = max(s_len)
    new = torch.empty if n_src else torch.zeros       # (no source row: nothing is launched, the outputs are the empty fit's)
    stats = new((B, 3), dtype=torch.float64, device=dev)
    iters_run = new(B, dtype=torch.int32, device=dev)
    done = new(B, dtype=torch.int32, device=dev)
    idx = torch.empty(n_src, dtype=torch.int32, device=dev) if return_idx else None
    nb = L.regtr_icp_ws_bytes(B, max_len)
    ws = ops._ws(max(nb, 1), dev)
    for k in range(iters + 1):
        check(L.regtr_icp_step(ptr(src) if n_src else None, iptr(s_off), n_src, max_len, iptr(t_off), tgt.shape[0], B, max_dist, r32,
                               bptr(grid.ws), grid.nbytes, ptr(pose), k, int(k == iters), rel_fitness, rel_rmse, dptr(stats),
                               iptr(iters_run), iptr(done), iptr(idx) if n_src else None, None, bptr(ws), nb,
                               stream()), 'regtr_icp_step')
    return stats, iters_run, idx


def _sym3_eigvals(A):
    """Eigenvalues (descending) of symmetric (B, 3, 3) float64 matrices in closed form (elementwise torch: no solver library, no host
    wait)."""
    q = (A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]) / 3
    p1 = A[:, 0, 1] ** 2 + A[:, 0, 2] ** 2 + A[:, 1, 2] ** 2
    p2 = (A[:, 0, 0] - q) ** 2 + (A[:, 1, 1] - q) ** 2 + (A[:, 2, 2] - q) ** 2 + 2 * p1
    p = torch.sqrt(p2 / 6)
    ps = torch.where(p > 0, p, torch.ones_like(p))
    Bm = (A - q[:, None, None] * torch.eye(3, dtype=A.dtype, device=A.device)) / ps[:, None, None]
    r = (_det3(Bm) / 2).clamp(-1, 1)
    phi = torch.acos(r) / 3
    e0 = q + 2 * p * torch.cos(phi)
    e2 = q + 2 * p * torch.cos(phi + 2 * math.pi / 3)
    return torch.stack([e0, 3 * q - e0 - e2, e2], dim=1)


def _det3(M):
    return (M[:, 0, 0] * (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1]) - M[:, 0, 1] * (M[:, 1, 0] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 0])
            + M[:, 0, 2] * (M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0]))


def _icp_composed(src, s_off, s_len, tgt, t_off, grid, r32, pose, max_dist, iters, rel_fitness, rel_rmse, return_idx):
    """The same iteration from the project's separate operators; the stop rule as masked torch arithmetic, so it waits for nothing
    either.  Matches and counts are the fused path's bit for bit; the fit runs through the float32 moments of the pose head's kernel."""
    L = _lib.lib()
    B, n_src, dev = len(s_len), src.shape[0], src.device
    max_len = max(max(s_len), 1)
    lens = torch.tensor(s_len, dtype=torch.float64).to(dev, non_blocking=True)
    pair_of = torch.repeat_interleave(torch.arange(B), torch.tensor(s_len)).to(dev, non_blocking=True)
    col = torch.cat([torch.arange(n) for n in s_len]).to(dev, non_blocking=True) if n_src else pair_of
    stats = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    iters_run = torch.zeros(B, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    idx_keep = torch.full((n_src,), -1, dtype=torch.int32, device=dev)
    P = pose.view(B, 3, 4)
    for k in range(iters + 1):
        y = ops.se3_transform(src, s_off, P)
        idx = torch.empty(max(n_src, 1), dtype=torch.int32, device=dev)
        check(L.regtr_nearest_in_radius(ptr(y) if n_src else None, iptr(s_off), n_src, iptr(t_off), tgt.shape[0], B, max_dist, r32,
                                        bptr(grid.ws), grid.nbytes, iptr(idx), stream()), 'regtr_nearest_in_radius')
        idx = idx[:n_src]
        hit = idx >= 0
        q = tgt[idx.clamp(min=0).long()] if tgt.shape[0] else torch.zeros_like(src)
        d = y.double() - q.double()
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        w = hit.double()
        n = torch.zeros(B, dtype=torch.float64, device=dev).index_add_(0, pair_of, w)
        sd2 = torch.zeros(B, dtype=torch.float64, device=dev).index_add_(0, pair_of, d2 * w)
        fitness = torch.where(lens > 0, n / lens.clamp(min=1), torch.zeros_like(n))
        rmse = torch.where(n > 0, torch.sqrt(sd2 / n.clamp(min=1)), torch.zeros_like(n))
        live = ~done
        moved = (fitness - stats[:, 0]).abs().lt(rel_fitness) & (rmse - stats[:, 1]).abs().lt(rel_rmse) if k > 0 else torch.zeros_like(done)
        stats = torch.where(live[:, None], torch.stack([fitness, rmse, n], dim=1), stats)
        idx_keep = torch.where(live[pair_of], idx, idx_keep) if n_src else idx_keep
        if k == iters:
            break
        # the matched rows of every pair, padded to one length with weight 0
        a = torch.zeros((B, max_len, 3), dtype=torch.float32, device=dev)
        b = torch.zeros((B, max_len, 3), dtype=torch.float32, device=dev)
        wt = torch.zeros((B, max_len), dtype=torch.float32, device=dev)
        if n_src:
            a[pair_of, col] = src
            b[pair_of, col] = q
            wt[pair_of, col] = hit.float()
        fit = se3.compute_rigid_transform(a, b, wt)
        # degeneracy as the fused solve tests it: the singular values of the float64 covariance, the smallest signed by det
        wn = (wt.double() / n.clamp(min=1)[:, None])[:, :, None]
        ca, cb = (a.double() * wn).sum(1), (b.double() * wn).sum(1)
        cov = torch.einsum('bnr,bnc->brc', (a.double() - ca[:, None]) * wn, b.double() - cb[:, None])
        S = torch.sqrt(_sym3_eigvals(cov.transpose(1, 2) @ cov).clamp(min=0))
        lam2 = torch.where(_det3(cov) < 0, -S[:, 2], S[:, 2])
        lmin = torch.minimum(torch.minimum(S[:, 0] + S[:, 1], S[:, 0] + lam2), S[:, 1] + lam2)
        stop = (n < 3) | ~torch.isfinite(P).reshape(B, 12).all(dim=1) | moved | ~(lmin > 2.0 ** -23 * S[:, 0])
        step = live & ~stop
        P.copy_(torch.where(step[:, None, None], fit, P))
        iters_run = torch.where(step, torch.full_like(iters_run, k + 1), iters_run)
        done = done | stop
    return stats, iters_run, (idx_keep if return_idx else None)


# ------------------------------------------------------------------------------------------------ point to plane
def _target_normals(tgt, t_off, grid, r32, max_dist, given, normal_radius):
    """The packed targets' (normals (n, 3) f32, valid (n,) i32): the caller's, or estimated with normal_radius (default max_dist; the
    matching grid serves when its cells are wide enough, else one more grid is built)."""
    n = tgt.shape[0]
    if given is not None:
        nrm, valid = (_packed(list(g), n, w, dt) for g, w, dt in zip(given, ((3,), ()), (torch.float32, torch.int32)))
        return nrm, valid
    radius = max_dist if normal_radius is None else float(normal_radius)
    if not radius > 0:
        raise RuntimeError(f'refine.icp: normal_radius > 0 expected, got {normal_radius}')
    if n and not r32 * (1 + 1e-6) >= radius:
        r32 = float(np.float32(radius))
        r32 = r32 if r32 * (1 + 1e-6) >= radius else float(np.nextafter(np.float32(radius), np.float32(np.inf)))
        grid = ops.CellGrid(tgt, t_off, n, r32)
    nrm, valid, _ = _normals_packed(tgt, t_off, grid, radius, r32)
    return nrm, valid


def _packed(views, n, tail, dtype):
    from .regtr import _packed_rows
    t = _packed_rows(views).contiguous()
    if tuple(t.shape) != (n,) + tail or t.dtype is not dtype or t.device.type != 'cuda':
        raise RuntimeError(f'refine.icp: tgt_normals must be lists of device (n, 3) float32 normals and (n,) int32 valid flags of the target '
                           f'clouds, got {tuple(t.shape)} {t.dtype} on {t.device}')
    return t


def _icp_plane_fused(src, s_off, s_len, tgt, t_off, grid, r32, nrm, valid, pose, max_dist, iters, rel_fitness, rel_rmse, return_idx):
    L = _lib.lib()
    B, n_src, n_tgt, dev = len(s_len), src.shape[0], tgt.shape[0], src.device
    max_len = max(s_len)
    new = torch.empty if n_src else torch.zeros       # (no source row: nothing is launched, the outputs are the empty fit's)
    stats = new((B, 3), dtype=torch.float64, device=dev)
    iters_run = new(B, dtype=torch.int32, device=dev)
    done = new(B, dtype=torch.int32, device=dev)
    idx = torch.empty(n_src, dtype=torch.int32, device=dev) if return_idx else None
    chunk = int(L.regtr_icp_chunk())
    partial = ops._ws_as(B * max(-(-max_len // chunk), 1) * 30, torch.float64, dev)      # (B, chunks, 30): the header states the shape
    pose64 = ops._ws_as(B * 12, torch.float64, dev)
    for k in range(iters + 1):
        check(L.regtr_icp_plane_step(ptr(src) if n_src else None, iptr(s_off), n_src, max_len, ptr(nrm) if n_tgt else None,
                                     iptr(valid) if n_tgt else None, iptr(t_off), n_tgt, B, max_dist, r32, bptr(grid.ws), grid.nbytes,
                                     ptr(pose), dptr(pose64), k, int(k == iters), rel_fitness, rel_rmse, dptr(stats), iptr(iters_run),
                                     iptr(done), iptr(idx) if n_src else None, dptr(partial), stream()), 'regtr_icp_plane_step')
    return stats, iters_run, idx


def _ldl6_solve(A, g):
    """(B, 6, 6), (B, 6) float64 -> (x (B, 6) with A x = -g, ok (B,)): the system scaled to unit diagonal, LDL^T without pivoting unrolled
    in elementwise torch operations (no solver library, no host wait); ok is False where a diagonal entry is not positive or a pivot is
    <= 2^-23, and x is then meaningless."""
    diag = torch.diagonal(A, dim1=1, dim2=2)
    ok = (diag > 0).all(dim=1)
    D = 1.0 / torch.sqrt(torch.where(diag > 0, diag, torch.ones_like(diag)))
    As = (A * D[:, :, None]) * D[:, None, :]
    z = -(g * D)
    Lm = [[None] * 6 for _ in range(6)]
    piv = []
    for j in range(6):
        d = As[:, j, j]
        for k in range(j):
            d = d - (Lm[j][k] * Lm[j][k]) * piv[k]
        ok = ok & (d > 2.0 ** -23)
        d = torch.where(d > 2.0 ** -23, d, torch.ones_like(d))
        piv.append(d)
        for i in range(j + 1, 6):
            v = As[:, i, j]
            for k in range(j):
                v = v - (Lm[i][k] * Lm[j][k]) * piv[k]
            Lm[i][j] = v / d
    w = [z[:, i] for i in range(6)]
    for i in range(6):
        for k in range(i):
            w[i] = w[i] - Lm[i][k] * w[k]
    w = [w[i] / piv[i] for i in range(6)]
    for i in range(5, -1, -1):
        for k in range(i + 1, 6):
            w[i] = w[i] - Lm[k][i] * w[k]
    return torch.stack(w, dim=1) * D, ok


def _icp_plane_composed(src, s_off, s_len, tgt, t_off, grid, r32, nrm, valid, pose, max_dist, iters, rel_fitness, rel_rmse, return_idx):
    """The point-to-plane iteration from the project's separate operators (ops.se3_transform, regtr_nearest_in_radius) with torch float64
    sums and _ldl6_solve; the stop rule as masked torch arithmetic, so it waits for nothing either.  Matches and counts are the fused
    path's bit for bit; the sums run in another order."""
    L = _lib.lib()
    B, n_src, dev = len(s_len), src.shape[0], src.device
    lens = torch.tensor(s_len, dtype=torch.float64).to(dev, non_blocking=True)
    pair_of = torch.repeat_interleave(torch.arange(B), torch.tensor(s_len)).to(dev, non_blocking=True)
    stats = torch.zeros((B, 3), dtype=torch.float64, device=dev)
    iters_run = torch.zeros(B, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    idx_keep = torch.full((n_src,), -1, dtype=torch.int32, device=dev)
    P = pose.view(B, 3, 4)
    P64 = P.double()
    max_len = max(max(s_len), 1)
    col = torch.cat([torch.arange(n) for n in s_len]).to(dev, non_blocking=True) if n_src else pair_of
    iu = torch.triu_indices(6, 6).to(dev, non_blocking=True)
    for k in range(iters + 1):
        y = ops.se3_transform(src, s_off, P)
        idx = torch.empty(max(n_src, 1), dtype=torch.int32, device=dev)
        check(L.regtr_nearest_in_radius(ptr(y) if n_src else None, iptr(s_off), n_src, iptr(t_off), tgt.shape[0], B, max_dist, r32,
                                        bptr(grid.ws), grid.nbytes, iptr(idx), stream()), 'regtr_nearest_in_radius')
        idx = idx[:n_src]
        hit = idx >= 0
        j = idx.clamp(min=0).long()
        q = tgt[j] if tgt.shape[0] else torch.zeros_like(src)
        nq = nrm[j].double() if tgt.shape[0] else torch.zeros_like(src, dtype=torch.float64)
        use = (hit & (valid[j] != 0) if tgt.shape[0] else hit & False).double()
        Y = y.double()
        d = Y - q.double()
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        w = hit.double()
        r = (nq[:, 0] * d[:, 0] + nq[:, 1] * d[:, 1]) + nq[:, 2] * d[:, 2]
        J = torch.cat([torch.linalg.cross(Y, nq), nq], dim=1) * use[:, None]
        # every row's 30 terms (n | d2 | n_sys | the 21 upper products | J r), padded to one length per pair and summed per pair: a float64
        # index_add_ of 1.4 M rows onto 64 pairs would serialise on its atomics
        terms = torch.cat([w[:, None], (d2 * w)[:, None], use[:, None], J[:, iu[0]] * J[:, iu[1]], J * r[:, None]], dim=1)
        padded = torch.zeros((B, max_len, 30), dtype=torch.float64, device=dev)
        if n_src:
            padded[pair_of, col] = terms
        S = padded.sum(dim=1)
        n, sd2, n_sys, g = S[:, 0], S[:, 1], S[:, 2], S[:, 24:]
        A = torch.zeros((B, 6, 6), dtype=torch.float64, device=dev)
        A[:, iu[0], iu[1]] = S[:, 3:24]
        A[:, iu[1], iu[0]] = S[:, 3:24]
        fitness = torch.where(lens > 0, n / lens.clamp(min=1), torch.zeros_like(n))
        rmse = torch.where(n > 0, torch.sqrt(sd2 / n.clamp(min=1)), torch.zeros_like(n))
        live = ~done
        moved = (fitness - stats[:, 0]).abs().lt(rel_fitness) & (rmse - stats[:, 1]).abs().lt(rel_rmse) if k > 0 else torch.zeros_like(done)
        stats = torch.where(live[:, None], torch.stack([fitness, rmse, n], dim=1), stats)
        idx_keep = torch.where(live[pair_of], idx, idx_keep) if n_src else idx_keep
        if k == iters:
            break
        A = torch.where(torch.isfinite(A), A, torch.zeros_like(A))      # (a frozen pair's NaNs stay out of the arithmetic)
        x, ok = _ldl6_solve(A, torch.where(torch.isfinite(g), g, torch.zeros_like(g)))
        stop = (n_sys < 6) | ~torch.isfinite(P).reshape(B, 12).all(dim=1) | moved | ~ok
        step = live & ~stop
        x = torch.where(step[:, None], x, torch.zeros_like(x))
        ca, sa, cb, sb, cg, sg = torch.cos(x[:, 0]), torch.sin(x[:, 0]), torch.cos(x[:, 1]), torch.sin(x[:, 1]), torch.cos(x[:, 2]), torch.sin(x[:, 2])
        Rm = torch.stack([cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa, sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                          -sb, cb * sa, cb * ca], dim=1).view(B, 3, 3)
        Q = torch.cat([Rm @ P64[:, :, :3], Rm @ P64[:, :, 3:] + x[:, 3:, None]], dim=2)
        P64 = torch.where(step[:, None, None], Q, P64)
        P.copy_(torch.where(step[:, None, None], Q.float(), P))
        iters_run = torch.where(step, torch.full_like(iters_run, k + 1), iters_run)
        done = done | stop
    return stats, iters_run, (idx_keep if return_idx else None)
