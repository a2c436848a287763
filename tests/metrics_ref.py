"""Numpy restatements of csrc/metrics.hip (test infrastructure): `nearest` in float32 with exactly the kernel's arithmetic (bit for bit),
`pose_metrics` in float64 with the kernel's order of operations, `segment_mean`, `aggregate` (the reference's _aggregate_metrics) and
`chamfer` / `modelnet_metrics` composed of them."""
import numpy as np

F32 = np.float32


def transform_f32(T, x):
    """((r0 x + r1 y) + r2 z) + t per row, float32 rounded per operation.  T (3, 4) or (12,), x (n, 3)."""
    T = np.asarray(T, F32).reshape(3, 4)
    x = np.asarray(x, F32)
    return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], 1).astype(F32)


def nearest_cloud(q, s, chunk=512):
    """One cloud: (d2 float32 (nq,), idx int32 (nq,)).  d2 = (dx dx + dy dy) + dz dz in float32; the minimum by a strict < over the
    supports in ascending index (the first of equals; NaN never wins; no candidate below +inf: +inf, -1)."""
    q, s = np.asarray(q, F32), np.asarray(s, F32)
    d2 = np.full(len(q), np.inf, F32)
    idx = np.full(len(q), -1, np.int32)
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(0, len(q), chunk):
            d = q[a:a + chunk, None, :] - s[None, :, :]
            sq = d * d
            e = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(F32)
            e = np.where(np.isnan(e), F32(np.inf), e)                 # a NaN never satisfies d < best
            if e.shape[1] == 0:
                continue
            j = np.argmin(e, axis=1)                                   # first occurrence: the lowest index on ties
            m = e[np.arange(len(j)), j]
            won = m < np.inf
            d2[a:a + chunk] = np.where(won, m, F32(np.inf))
            idx[a:a + chunk] = np.where(won, j, -1)
    return d2, idx


def nearest(q_xyz, q_off, s_xyz, s_off, q_pose=None, s_pose=None):
    """Packed clouds, as ops.nearest."""
    d2 = np.empty(len(q_xyz), F32)
    idx = np.empty(len(q_xyz), np.int32)
    for c in range(len(q_off) - 1):
        q = np.asarray(q_xyz[q_off[c]:q_off[c + 1]], F32)
        s = np.asarray(s_xyz[s_off[c]:s_off[c + 1]], F32)
        if q_pose is not None:
            q = transform_f32(q_pose[c], q)
        if s_pose is not None:
            s = transform_f32(s_pose[c], s)
        d2[q_off[c]:q_off[c + 1]], idx[q_off[c]:q_off[c + 1]] = nearest_cloud(q, s)
    return d2, idx


def segment_mean(v, off):
    return np.array([np.asarray(v[off[c]:off[c + 1]], np.float64).mean() if off[c + 1] > off[c] else 0.0 for c in range(len(off) - 1)])


def _euler_xyz_deg(R):
    """Extrinsic xyz Euler angles (R = Rz(c) Ry(b) Rx(a)) in degrees, closed form; R (..., 3, 3) float64."""
    k = 180.0 / np.pi
    return np.stack([np.arctan2(R[..., 2, 1], R[..., 2, 2]) * k, -np.arcsin(np.clip(R[..., 2, 0], -1.0, 1.0)) * k,
                     np.arctan2(R[..., 1, 0], R[..., 0, 0]) * k], -1)


def pose_metrics(pred, gt):
    """pred (L, B, 3|4, 4) or (B, 3|4, 4), gt (B, 3|4, 4) (float32 values) -> (out (..., 8) float64, composed (..., 3, 4) float32), the
    kernel's order of operations: sums left to right in float64."""
    pred, gt = np.asarray(pred, F32).astype(np.float64)[..., :3, :], np.asarray(gt, F32).astype(np.float64)[..., :3, :]
    Rp, tp, Rg, tg = pred[..., :3], pred[..., 3], gt[..., :3], gt[..., 3]
    Rg, tg = np.broadcast_to(Rg, Rp.shape), np.broadcast_to(tg, tp.shape)
    k = 180.0 / np.pi
    Rc = np.empty_like(Rp)
    for i in range(3):
        for j in range(3):
            Rc[..., i, j] = (Rp[..., i, 0] * Rg[..., j, 0] + Rp[..., i, 1] * Rg[..., j, 1]) + Rp[..., i, 2] * Rg[..., j, 2]
    tc = np.stack([tp[..., i] - ((Rc[..., i, 0] * tg[..., 0] + Rc[..., i, 1] * tg[..., 1]) + Rc[..., i, 2] * tg[..., 2]) for i in range(3)], -1)
    out = np.empty(Rp.shape[:-2] + (8,))
    out[..., 0] = np.arccos(np.clip(0.5 * (((Rc[..., 0, 0] + Rc[..., 1, 1]) + Rc[..., 2, 2]) - 1.0), -1.0, 1.0)) * k
    out[..., 1] = np.sqrt((tc[..., 0] * tc[..., 0] + tc[..., 1] * tc[..., 1]) + tc[..., 2] * tc[..., 2])
    tr = 0.0
    for i in range(3):
        tr = tr + ((Rg[..., 0, i] * Rp[..., 0, i] + Rg[..., 1, i] * Rp[..., 1, i]) + Rg[..., 2, i] * Rp[..., 2, i])
    dt = tp - tg
    ti = np.stack([(Rg[..., 0, i] * dt[..., 0] + Rg[..., 1, i] * dt[..., 1]) + Rg[..., 2, i] * dt[..., 2] for i in range(3)], -1)
    out[..., 2] = np.arccos(np.clip(0.5 * (tr - 1.0), -1.0, 1.0)) * k
    out[..., 3] = np.sqrt((ti[..., 0] * ti[..., 0] + ti[..., 1] * ti[..., 1]) + ti[..., 2] * ti[..., 2])
    out[..., 4] = ((dt[..., 0] * dt[..., 0] + dt[..., 1] * dt[..., 1]) + dt[..., 2] * dt[..., 2]) / 3.0
    out[..., 5] = ((np.abs(dt[..., 0]) + np.abs(dt[..., 1])) + np.abs(dt[..., 2])) / 3.0
    de = _euler_xyz_deg(Rg) - _euler_xyz_deg(Rp)
    out[..., 6] = ((de[..., 0] * de[..., 0] + de[..., 1] * de[..., 1]) + de[..., 2] * de[..., 2]) / 3.0
    out[..., 7] = ((np.abs(de[..., 0]) + np.abs(de[..., 1])) + np.abs(de[..., 2])) / 3.0
    return out, np.concatenate([Rc, tc[..., None]], -1).astype(F32)


def compute_metrics(pred_pose, gt):
    """RegTR.compute_metrics: {'rot_err_deg', 'trans_err'} (L, B) float32."""
    out, _ = pose_metrics(pred_pose, gt)
    return {'rot_err_deg': out[..., 0].astype(F32), 'trans_err': out[..., 1].astype(F32)}


def chamfer(src, ref, raw, pred, gt):
    """metrics.chamfer: lists of clouds, pred / gt (B, 3|4, 4) -> (B,) float32."""
    _, comp = pose_metrics(pred, gt)
    pred = np.asarray(pred, F32)
    out = []
    for b in range(len(src)):
        d_src, _ = nearest_cloud(transform_f32(pred[b, :3], src[b][:, :3]), raw[b][:, :3])
        d_ref, _ = nearest_cloud(ref[b][:, :3], transform_f32(comp[b], raw[b][:, :3]))
        out.append(d_src.astype(np.float64).mean() + d_ref.astype(np.float64).mean())
    return np.asarray(out).astype(F32)


def modelnet_metrics(pred, gt, src, ref, raw):
    out, _ = pose_metrics(pred, gt)
    m = {k: out[..., c] for k, c in (('r_mse', 6), ('r_mae', 7), ('t_mse', 4), ('t_mae', 5), ('err_r_deg', 2), ('err_t', 3))}
    m['chamfer_dist'] = chamfer(src, ref, raw, pred, gt)
    return m


def aggregate(step_metrics, thresh_rot, thresh_trans):
    """generic_reg_model.py:211-250 on numpy arrays ((L, B_step) per key and step)."""
    cat = {k: np.concatenate([np.asarray(m[k]) for m in step_metrics], axis=1) for k in step_metrics[0]}
    rot, trans = cat['rot_err_deg'], cat['trans_err']
    out = {}
    L = rot.shape[0]
    for p in range(L):
        s = f'{p}' if p < L - 1 else 'final'
        out[f'rot_err_deg_{s}'] = rot[p].mean(dtype=rot.dtype)
        out[f'rot_err_{s}_hist'] = rot[p]
        out[f'trans_err_{s}'] = trans[p].mean(dtype=trans.dtype)
        out[f'trans_err_{s}_hist'] = trans[p]
        out[f'reg_success_{s}'] = np.logical_and(rot[p] < thresh_rot, trans[p] < thresh_trans).astype(F32).mean(dtype=F32)
    return out
