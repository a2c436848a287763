"""Generates tests/golden/procrustes_grads.npz: float64 autograd through the REAL reference compute_rigid_transform
(utils/se3_torch.py:108-154, loaded by file path as tools/make_golden_augment.py loads transforms.py) on float32-representable inputs.
Runs where the reference tree is present (oracle/ref_loader.py: REF_SRC); the fixture holds inputs, upstream gradients and the expected
gradients -- data only.

Two groups:
  * the model's layout, one launch: L = 2 decoder layers, pairs (n_src, n_tgt) = (5, 9), (300, 257), (64, 0), (130, 1) -- kp (N, 3),
    corr (L, N, 3), logit (L, N), seg_off (2B + 1,), d_pose (L, B, 3, 4) -> d_corr, d_logit, d_kp, d_weight, pose.  The pose assembly
    is the reference's (models/regtr.py:185-203: a = [src_kp ; tgt_corr], b = [src_corr ; tgt_kp], w = sigmoid([src ; tgt] logits)).
    Pair 2 is a reflected case (d = -1: its correspondences are a mirror image), pair 3 has coplanar points (S2 = 0 exactly).
  * the drop-in's layout: se3_a, se3_b (2, 3, 40, 3), se3_w (2, 3, 40) with exact 0 and 1 among the weights, se3_dT (2, 3, 3, 4) ->
    se3_da, se3_db, se3_dw, and se3_none_da, se3_none_db for weights=None.
For every recorded pair it asserts lam_0 / (lam_1 + lam_2) <= 10 and singular values at least 0.02 S0 apart: the reference's own SVD
backward (which divides by differences of squared singular values) is well conditioned there.

    python tools/make_golden_procrustes_grads.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_loader import REF_SRC      # noqa: E402

PAIRS = [(5, 9), (300, 257), (64, 0), (130, 1)]
LAYERS = 2
REFLECTED, COPLANAR = 2, 3
SIGMA = np.array([1.0, 0.8, 0.35])           # per-axis spread of the clouds: singular values ~ sigma^2 = 1, 0.64, 0.12


def load_se3():
    spec = importlib.util.spec_from_file_location('ref_se3_torch', os.path.join(REF_SRC, 'utils', 'se3_torch.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def check_conditioning(cov, what, want_d=None, want_s2_zero=False):
    u, s, vt = np.linalg.svd(cov)
    d = 1.0 if np.linalg.det(vt.T @ u.T) > 0 else -1.0
    lam = (s[0], s[1], d * s[2])
    assert lam[0] / (lam[1] + lam[2]) <= 10, (what, s, d)
    assert s[0] - s[1] >= 0.02 * s[0] and s[1] - s[2] >= 0.02 * s[0], (what, s)
    if want_d is not None:
        assert d == want_d, (what, d)
    if want_s2_zero:
        assert s[2] <= 1e-15 * s[0], (what, s)
    return s, d


def ref_cov(a, b, w):
    """The covariance compute_rigid_transform forms, in float64 (for the conditioning asserts only)."""
    wn = w / max(w.sum(), 1e-6)
    ca, cb = (a * wn[:, None]).sum(0), (b * wn[:, None]).sum(0)
    return (a - ca).T @ ((b - cb) * wn[:, None])


def model_group(se3, rng):
    B = len(PAIRS)
    lens = [p[0] for p in PAIRS] + [p[1] for p in PAIRS]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N = int(seg[-1])
    kp = np.zeros((N, 3))
    corr = np.zeros((LAYERS, N, 3))
    for p in range(B):
        s, t = slice(seg[p], seg[p + 1]), slice(seg[B + p], seg[B + p + 1])
        off = rng.uniform(-0.3, 0.3, 3)
        kp[s] = rng.standard_normal((lens[p], 3)) * SIGMA + off
        if p == COPLANAR:
            kp[s, 2] = 0.0
        for l in range(LAYERS):
            R, tr = rotation(rng), rng.uniform(-0.3, 0.3, 3)
            M = np.diag([1.0, 1.0, -1.0]) if p == REFLECTED else np.eye(3)
            corr[l, s] = (kp[s] * np.diag(M)) @ R.T + tr + 0.25 * rng.standard_normal((lens[p], 3))
            if l == 0:      # the tgt key points: images of src-like points, so that both halves describe one motion
                q = rng.standard_normal((lens[B + p], 3)) * SIGMA + off
                kp[t] = (q * np.diag(M)) @ R.T + tr
            back = ((kp[t] - tr) @ R) * np.diag(M) + 0.25 * rng.standard_normal((lens[B + p], 3))
            if p == COPLANAR:
                back[:, 2] = 0.0
            corr[l, t] = back
    logit = rng.uniform(-2, 2, (LAYERS, N))
    d_pose = rng.standard_normal((LAYERS, B, 3, 4))
    d_pose[..., 3] *= 0.25      # the translation's share of d_weight is a difference of two terms of the clouds' extent: kept below the rotation's
    kp, corr, logit, d_pose = f32(kp), f32(corr), f32(logit), f32(d_pose)

    kp_t = torch.from_numpy(kp).double().requires_grad_()
    corr_t = torch.from_numpy(corr).double().requires_grad_()
    logit_t = torch.from_numpy(logit).double().requires_grad_()
    pose = torch.zeros(LAYERS, B, 3, 4, dtype=torch.float64)
    d_weight = np.zeros((LAYERS, N))
    poses = []
    keep = []
    for l in range(LAYERS):
        for p in range(B):
            s, t = slice(seg[p], seg[p + 1]), slice(seg[B + p], seg[B + p + 1])
            a = torch.cat([kp_t[s], corr_t[l, t]])                         # regtr.py:187-190
            b = torch.cat([corr_t[l, s], kp_t[t]])
            w = torch.sigmoid(torch.cat([logit_t[l, s], logit_t[l, t]]))   # regtr.py:191-194
            w.retain_grad()
            keep.append((l, s, t, w))
            check_conditioning(ref_cov(a.detach().numpy(), b.detach().numpy(), w.detach().numpy()), ('model', l, p),
                               want_d=-1.0 if p == REFLECTED else 1.0, want_s2_zero=p == COPLANAR)
            poses.append(se3.compute_rigid_transform(a, b, w))
    pose = torch.stack(poses).reshape(LAYERS, B, 3, 4)
    (pose * torch.from_numpy(d_pose).double()).sum().backward()
    for l, s, t, w in keep:
        ns = s.stop - s.start
        d_weight[l, s], d_weight[l, t] = w.grad[:ns].numpy(), w.grad[ns:].numpy()
    # kp.grad sums the layers; the operator reports d_kp per layer: one backward per layer for it
    d_kp = np.zeros((LAYERS, N, 3))
    for l in range(LAYERS):
        kp_l = torch.from_numpy(kp).double().requires_grad_()
        tot = 0
        for p in range(B):
            s, t = slice(seg[p], seg[p + 1]), slice(seg[B + p], seg[B + p + 1])
            a = torch.cat([kp_l[s], corr_t[l, t].detach()])
            b = torch.cat([corr_t[l, s].detach(), kp_l[t]])
            w = torch.sigmoid(torch.cat([logit_t[l, s], logit_t[l, t]])).detach()
            tot = tot + (se3.compute_rigid_transform(a, b, w) * torch.from_numpy(d_pose[l, p]).double()).sum()
        tot.backward()
        d_kp[l] = kp_l.grad.numpy()
    assert np.allclose(d_kp.sum(0), kp_t.grad.numpy(), rtol=0, atol=1e-12 * np.abs(d_kp).max())
    return dict(kp=kp, corr=corr, logit=logit, seg_off=seg, d_pose=d_pose, pose=pose.detach().numpy(), d_corr=corr_t.grad.numpy(),
                d_logit=logit_t.grad.numpy(), d_kp=d_kp, d_weight=d_weight)


def se3_group(se3, rng):
    shape = (2, 3, 40)
    a = rng.standard_normal(shape + (3,)) * SIGMA + rng.uniform(-0.5, 0.5, (2, 3, 1, 3))
    b = np.zeros_like(a)
    for i in range(2):
        for j in range(3):
            R, tr = rotation(rng), rng.uniform(-1, 1, 3)
            b[i, j] = a[i, j] @ R.T + tr + 0.05 * rng.standard_normal((40, 3))
    w = rng.uniform(0.05, 0.95, shape)
    w[..., 3] = 0.0
    w[..., 17] = 1.0
    w[0, 1, 30:] = 0.0
    w[1, 2, :5] = 1.0
    dT = rng.standard_normal((2, 3, 3, 4))
    a, b, w, dT = f32(a), f32(b), f32(w), f32(dT)
    out = dict(se3_a=a, se3_b=b, se3_w=w, se3_dT=dT)
    for tag, use_w in (('', True), ('_none', False)):
        at, bt = torch.from_numpy(a).double().requires_grad_(), torch.from_numpy(b).double().requires_grad_()
        wt = torch.from_numpy(w).double().requires_grad_() if use_w else None
        for i in range(2):
            for j in range(3):
                wn = w[i, j].astype(np.float64) if use_w else np.full(40, 0.5)
                check_conditioning(ref_cov(a[i, j].astype(np.float64), b[i, j].astype(np.float64), wn), ('se3', tag, i, j), want_d=1.0)
        T = se3.compute_rigid_transform(at, bt, wt)
        (T * torch.from_numpy(dT).double()).sum().backward()
        out[f'se3{tag}_T'] = T.detach().numpy()
        out[f'se3{tag}_da'], out[f'se3{tag}_db'] = at.grad.numpy(), bt.grad.numpy()
        if use_w:
            out['se3_dw'] = wt.grad.numpy()
    return out


def main():
    se3 = load_se3()
    rng = np.random.default_rng(20250318)
    out = model_group(se3, rng)
    out.update(se3_group(se3, rng))
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    dst = os.path.join(ROOT, 'tests', 'golden', 'procrustes_grads.npz')
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
    main()
