"""RegTR.compute_loss and its kernels (csrc/losses.hip) on the GPU: regtr_infonce and regtr_loss_terms against float64 restatements,
compute_loss against the REAL reference's losses (tests/golden/losses_*.npz, tools/make_golden_losses.py), batch equivalences,
determinism, no host synchronisation, the batched GT masks and test.py --losses."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.util import ROOT, gold, load_cfg, seeded_sd

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
SIZES = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 394, 611, 2100]
R_P, R_N = 0.2, 0.4


# ---------------------------------------------------------------------------------------------------- float64 restatements
def _dist_f32(a, p):
    """d_ij = sqrt_rn(((dx^2 + dy^2) + dz^2)) in float32, rounded per operation (the kernel's arithmetic)."""
    d = a[:, None, :].astype(F32) - p[None, :, :].astype(F32)
    sq = d * d
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(F32)


def _transform_f32(T, x):
    """((R0 x + R1 y) + R2 z) + t per row, float32 rounded per operation."""
    T = T.astype(F32)
    cols = [((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)]
    return np.stack(cols, 1).astype(F32)


def _infonce_ref(A, P, ax, px, r_p, r_n):
    """Per row: (loss float64, mask, bound).  Decisions in the kernel's float32 distance arithmetic, logits / logsumexp in float64."""
    d = _dist_f32(ax, px)
    js = np.argmin(d, axis=1)                                   # first occurrence: the lowest j on exact ties
    rows = np.arange(len(A))
    dstar = d[rows, js]
    mask = dstar < F32(r_p)
    keep = ~(d < F32(r_n))
    keep[rows, js] = True
    l = A.astype(np.float64) @ P.astype(np.float64).T
    lm = np.where(keep, l, -np.inf)
    m = lm.max(1)
    lse = m + np.log(np.exp(lm - m[:, None]).sum(1))
    loss = lse - l[rows, js]
    D = A.shape[1]
    e = (D + 8) * U * (np.abs(A).astype(np.float64) @ np.abs(P).astype(np.float64).T).max(1)
    bound = 2 * e + 8 * U * (np.abs(lse) + np.abs(l[rows, js]) + np.log(keep.sum(1) + 1.0)) + 1e-6
    return loss, mask, bound


# ---------------------------------------------------------------------------------------------------- direct calls
def _lib():
    from regtr_amd import _lib as L
    return L.lib()


def _sentinel(n, pad=64):
    """NaN-filled buffer of n floats between two finite sentinel bands; returns (buffer, view)."""
    buf = torch.full((n + 2 * pad,), float('nan'), dtype=torch.float32, device='cuda')
    buf[:pad] = 12345.0
    buf[pad + n:] = -6789.0
    return buf, buf[pad:pad + n]


def _check_sentinel(buf, n, pad=64):
    h = buf.cpu().numpy()
    assert np.all(h[:pad] == 12345.0) and np.all(h[pad + n:] == -6789.0), 'write outside the output view'


def _run_infonce(A, P, ax, px, a_off, p_off, r_p, r_n, pose=None):
    """regtr_infonce on host arrays; outputs in sentinel-bounded NaN buffers.  -> (pair_out (B,2), row_loss, row_mask) numpy."""
    L = _lib()
    dev = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dtype=dt, device='cuda')
    B = len(a_off) - 1
    n_anc, D = A.shape
    n_pos = P.shape[0]
    max_anc = int(np.max(np.diff(a_off))) if B else 0
    tA, tP, tax, tpx = dev(A), dev(P), dev(ax), dev(px)
    ta, tp = dev(np.asarray(a_off, np.int32), torch.int32), dev(np.asarray(p_off, np.int32), torch.int32)
    tpose = dev(np.asarray(pose, F32).reshape(B, 12)) if pose is not None else None
    pb, po = _sentinel(2 * B)
    lb, lo = _sentinel(n_anc)
    mb, mo = _sentinel(n_anc)
    nb = L.regtr_infonce_ws_bytes(B, max_anc)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device='cuda')
    rc = L.regtr_infonce(tA.data_ptr(), D, tP.data_ptr(), D, tax.data_ptr(), tpx.data_ptr(), ta.data_ptr(), tp.data_ptr(), B, n_anc,
                         n_pos, max_anc, D, float(r_p), float(r_n), tpose.data_ptr() if tpose is not None else None, po.data_ptr(),
                         lo.data_ptr(), mo.data_ptr(), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, n in ((pb, 2 * B), (lb, n_anc), (mb, n_anc)):
        _check_sentinel(buf, n)
    return po.cpu().numpy().reshape(B, 2), lo.cpu().numpy(), mo.cpu().numpy()


def _make_pairs(rng, sizes, D, specials=True):
    """Ragged pairs: list of (A, P, ax, px); plus the special pairs (NaN pair, all-in-r_n pair, duplicated targets)."""
    out = []
    for ns, nt in sizes:
        side = max(0.6, 0.25 * (max(ns, nt) ** (1 / 3)))
        ax = rng.uniform(0, side, (ns, 3)).astype(F32)
        px = rng.uniform(0, side, (nt, 3)).astype(F32)
        out.append((rng.normal(0, 0.3, (ns, D)).astype(F32), rng.normal(0, 0.3, (nt, D)).astype(F32), ax, px))
    if specials:
        # no anchor within r_p: the pair's count is 0 (compute_loss: 0 / 0 = NaN, as in the reference)
        out.append((rng.normal(0, 0.3, (20, D)).astype(F32), rng.normal(0, 0.3, (30, D)).astype(F32),
                    rng.uniform(0, 1, (20, 3)).astype(F32) + F32(50), rng.uniform(0, 1, (30, 3)).astype(F32)))
        # every target within r_n of every anchor: only the positive is left, loss exactly 0
        out.append((rng.normal(0, 0.3, (17, D)).astype(F32), rng.normal(0, 0.3, (40, D)).astype(F32),
                    rng.uniform(0, 0.05, (17, 3)).astype(F32), rng.uniform(0, 0.05, (40, 3)).astype(F32)))
        # duplicated target points: the lowest index must be the positive
        base = rng.uniform(0, 1, (25, 3)).astype(F32)
        px = np.concatenate([base, base, base[::-1]]).astype(F32)
        out.append((rng.normal(0, 0.3, (33, D)).astype(F32), rng.normal(0, 0.3, (75, D)).astype(F32),
                    np.concatenate([base[:20], rng.uniform(0, 1, (13, 3)).astype(F32)]), px))
    return out


def _pack(pairs):
    A = np.concatenate([p[0] for p in pairs])
    P = np.concatenate([p[1] for p in pairs])
    ax = np.concatenate([p[2] for p in pairs])
    px = np.concatenate([p[3] for p in pairs])
    a_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(np.int32)
    p_off = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])]).astype(np.int32)
    return A, P, ax, px, a_off, p_off


@pytest.mark.parametrize('D', [64, 256, 512])
@pytest.mark.parametrize('layout', ['sizes', 'ragged64'])
def test_infonce_vs_float64(D, layout):
    rng = np.random.default_rng(D + (0 if layout == 'sizes' else 1))
    if layout == 'sizes':
        sizes = [(SIZES[i], SIZES[(7 * i + 3) % len(SIZES)]) for i in range(len(SIZES))] + [(SIZES[i], SIZES[i]) for i in range(0, 15, 2)]
    else:
        sizes = [(int(rng.integers(1, 420)), int(rng.integers(1, 420))) for _ in range(61)]
    pairs = _make_pairs(rng, sizes, D)
    A, P, ax, px, a_off, p_off = _pack(pairs)
    po, rl, rm = _run_infonce(A, P, ax, px, a_off, p_off, R_P, R_N)
    worst = 0.0
    for b, (Ab, Pb, axb, pxb) in enumerate(pairs):
        loss, mask, bound = _infonce_ref(Ab, Pb, axb, pxb, R_P, R_N)
        sl = slice(a_off[b], a_off[b + 1])
        assert np.array_equal(rm[sl], mask.astype(F32)), f'pair {b}: mask'
        err = np.abs(rl[sl].astype(np.float64) - loss)
        assert np.all(err <= bound), (b, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        assert po[b, 1] == mask.sum(), b
        s_ref = loss[mask].sum()
        assert abs(po[b, 0] - s_ref) <= bound[mask].sum() + 4 * U * np.abs(loss[mask]).sum() * len(loss) + 1e-5, b
    nan_pair, zero_pair = len(pairs) - 3, len(pairs) - 2
    assert po[nan_pair, 1] == 0 and po[nan_pair, 0] == 0
    assert np.all(rl[a_off[zero_pair]:a_off[zero_pair + 1]] == 0.0)
    print(f'infonce D={D} {layout}: {len(pairs)} pairs, worst err/bound {worst:.3f}')


def test_infonce_pose_applied_on_load():
    rng = np.random.default_rng(3)
    pairs = _make_pairs(rng, [(70, 90), (33, 129)], 256, specials=False)
    A, P, ax, px, a_off, p_off = _pack(pairs)
    c, s = np.cos(0.4), np.sin(0.4)
    poses = np.stack([np.array([[c, -s, 0, 0.1], [s, c, 0, -0.2], [0, 0, 1, 0.05]]), np.eye(4)[:3]]).astype(F32)
    po, rl, rm = _run_infonce(A, P, ax, px, a_off, p_off, R_P, R_N, pose=poses)
    axw = np.concatenate([_transform_f32(poses[b], pairs[b][2]) for b in range(2)])
    po2, rl2, rm2 = _run_infonce(A, P, axw, px, a_off, p_off, R_P, R_N)
    assert np.array_equal(po, po2) and np.array_equal(rl, rl2) and np.array_equal(rm, rm2)


def test_infonce_deterministic():
    rng = np.random.default_rng(9)
    pairs = _make_pairs(rng, [(394, 400)] * 8 + [(611, 129)], 256)
    args = _pack(pairs)
    a = _run_infonce(*args, R_P, R_N)
    b = _run_infonce(*args, R_P, R_N)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _loss_terms_ref(logit, gt, kp, warped, seg, poses):
    B = len(poses)
    out = np.zeros((B, 5))
    for b in range(B):
        T = poses[b].astype(F32)[:3]
        Ti = np.zeros((3, 4), F32)
        Ti[:, :3] = T[:, :3].T
        for r in range(3):
            Ti[r, 3] = -(((T[0, r] * T[0, 3]) + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
        for side, (lo, hi), M in ((0, (seg[b], seg[b + 1]), T), (1, (seg[B + b], seg[B + b + 1]), Ti)):
            x, y = logit[lo:hi].astype(np.float64), gt[lo:hi].astype(np.float64)
            out[b, 0] += (np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).sum()
            w3 = _transform_f32(M, kp[lo:hi])
            e = np.abs(warped[lo:hi] - w3).astype(F32)
            err = ((e[:, 0] + e[:, 1]) + e[:, 2]).astype(F32)
            out[b, 1 + 2 * side] += (gt[lo:hi] * err).astype(F32).astype(np.float64).sum()
            out[b, 2 + 2 * side] += gt[lo:hi].astype(np.float64).sum()
    return out


def test_loss_terms_vs_float64():
    from regtr_amd import ops
    rng = np.random.default_rng(4)
    lens_s, lens_t = [1, 64, 300, 0, 17], [5, 129, 250, 40, 0]
    B = len(lens_s)
    lens = lens_s + lens_t
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    N = int(seg[-1])
    logit = rng.normal(0, 3, N).astype(F32)
    logit[::7] = 80.0
    logit[3::7] = -80.0                                        # BCE stability: exp(80) overflows a naive form
    gt = rng.uniform(0, 1, N).astype(F32)
    gt[::5] = 0.0
    gt[seg[2]:seg[3]] = 0.0                                    # pair 2's src: all-zero weights (the clamp path)
    gt[seg[B + 2]:seg[B + 3]] = 0.0
    kp = rng.uniform(-2, 2, (N, 3)).astype(F32)
    warped = (kp + rng.normal(0, 0.1, (N, 3))).astype(F32)
    c, s = np.cos(0.7), np.sin(0.7)
    poses = np.stack([np.array([[c, -s, 0, 0.3 * b], [s, c, 0, -0.1], [0, 0, 1, 0.2], [0, 0, 0, 1]]) for b in range(B)]).astype(F32)
    ref = _loss_terms_ref(logit, gt, kp, warped, seg, poses)
    d = lambda x: torch.from_numpy(x).cuda()
    for P in (poses, poses[:, :3]):
        got = ops.loss_terms(d(logit), d(gt), d(kp), d(warped), d(seg), d(np.ascontiguousarray(P))).cpu().numpy().astype(np.float64)
        tol = 1e-6 * np.abs(ref) + 1e-5
        assert np.all(np.abs(got - ref) <= tol), np.abs(got - ref).max()
    assert got[2, 2] == 0.0 and np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------- compute_loss vs the reference
def _clouds(case):
    """The input clouds of a loss golden: those of the forward golden of the same name (tools/make_golden_losses.py reads them there)."""
    f = gold(case)
    if case == '3dmatch_crop_b2':
        return [f['src_0'], f['src_1']], [f['tgt_0'], f['tgt_1']]
    return [f['src']], [f['tgt']]


def _golden_batch(g, case, dev='cuda'):
    B = int(g['n_pairs'])
    srcs, tgts = _clouds(case)
    assert len(srcs) == B
    return (srcs, tgts,
            {'pose': torch.from_numpy(g['pose']).to(dev), 'src_overlap': [torch.from_numpy(g[f'src_mask_{b}']).to(dev) for b in range(B)],
             'tgt_overlap': [torch.from_numpy(g[f'tgt_mask_{b}']).to(dev) for b in range(B)]})


def _loss_weights(shape, seed):
    """tools/make_golden_losses.py loss_weights: N(0, 0.1) from torch's CPU generator, W then W_un."""
    gen = torch.Generator().manual_seed(int(seed))
    return torch.randn(shape, generator=gen) * 0.1, torch.randn(shape, generator=gen) * 0.1


def _model(cfg, g):
    from regtr_amd import RegTR
    sd = seeded_sd(cfg)
    sd['feature_criterion.W'], sd['feature_criterion_un.W'] = _loss_weights(tuple(sd['feature_criterion.W'].shape), g['w_seed'])
    m = RegTR(cfg)
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _forward(model, srcs, tgts, extra):
    batch = {'src_xyz': [torch.from_numpy(s).cuda() for s in srcs], 'tgt_xyz': [torch.from_numpy(t).cuda() for t in tgts]}
    pred = model(batch)
    batch.update(extra)
    return pred, batch


def _ref_pred(g, pred, L=6):
    """pred with the reference's own coarsest-level key points, correspondences and overlap logits (layer 5 of the decoder outputs) in
    place of this forward's; the features stay this forward's (parity mode: within 1e-4 of the reference's)."""
    B = int(g['n_pairs'])
    t = lambda x: torch.from_numpy(x).cuda()
    def layered(k, b):
        x = t(g[f'{k}_{b}'])
        full = torch.zeros((L,) + tuple(x.shape), dtype=torch.float32, device='cuda')
        full[5] = x
        return full
    out = dict(pred)
    for k in ('src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
        out[k] = [layered(k, b) for b in range(B)]
    for k in ('src_kp', 'tgt_kp'):
        out[k] = tuple(t(g[f'{k}_{b}']) for b in range(B))
    return out


CASES = [('3dmatch_crop_b2', '3dmatch'), ('3dmatch_kitchen', '3dmatch'), ('modelnet_630', 'modelnet')]


@pytest.mark.parametrize('case,cfgn', CASES)
def test_compute_loss_vs_reference_golden(case, cfgn):
    """compute_loss on the reference's key points / correspondences / overlap logits and this project's parity-mode features
    (parity-mode pyramid: the reference's pools for the GT pyramid): every key within 1e-5 relative of the reference with exact
    distances, and of the stock reference within the recorded decision gap."""
    g = gold(f'losses_{case}')
    cfg = load_cfg(cfgn)
    cfg.update({'kpconv_ref_row_order': True})
    model = _model(cfg, g)
    srcs, tgts, extra = _golden_batch(g, case)
    pred, batch = _forward(model, srcs, tgts, extra)
    for b in range(int(g['n_pairs'])):
        assert np.array_equal(pred['src_kp'][b].cpu().numpy(), g[f'src_kp_{b}'])
        assert np.array_equal(pred['tgt_kp'][b].cpu().numpy(), g[f'tgt_kp_{b}'])
    got = model.compute_loss(_ref_pred(g, pred), batch)
    gap = int(g['decision_rows'])
    rep = {}
    for k, v in got.items():
        v = float(v)
        ex, st = float(g[f'exact_{k}']), float(g[f'ref_{k}'])
        rep[k] = (v, ex, abs(v - ex) / max(abs(ex), 1e-12))
        assert abs(v - ex) <= 1e-5 * max(abs(ex), 1.0), (k, v, ex)
        # stock cdist: `gap` rows decide differently; with none, the two reference values are equal and so is the bound
        assert abs(v - st) <= 1e-5 * max(abs(st), 1.0) + gap * 50.0 / max(int(g['anchor_rows']), 1) * max(abs(st), 1.0), (k, v, st)
    print(case, 'parity, reference kp / corr / logits:', {k: f'{r[2]:.1e}' for k, r in rep.items()}, 'decision gap rows', gap)


@pytest.mark.parametrize('case,cfgn', CASES)
@pytest.mark.parametrize('parity', [True, False])
def test_compute_loss_own_forward_vs_reference(case, cfgn, parity):
    """compute_loss on this project's own forward (parity and default mode) against the reference's losses; the gap is the forward's."""
    g = gold(f'losses_{case}')
    cfg = load_cfg(cfgn)
    cfg.update({'kpconv_ref_row_order': parity})
    model = _model(cfg, g)
    srcs, tgts, extra = _golden_batch(g, case)
    pred, batch = _forward(model, srcs, tgts, extra)
    got = model.compute_loss(pred, batch)
    rel = {k: abs(float(v) - float(g[f'exact_{k}'])) / max(abs(float(g[f'exact_{k}'])), 1e-12) for k, v in got.items()}
    print(case, 'parity' if parity else 'default', 'own forward, rel err:', {k: f'{v:.1e}' for k, v in rel.items()})
    tol = 1e-3 if parity else 5e-2
    for k, v in rel.items():
        assert v <= tol, (k, v)


def test_per_pair_equals_single_pair_forwards_and_is_deterministic():
    case = '3dmatch_crop_b2'
    g = gold(f'losses_{case}')
    cfg = load_cfg('3dmatch')
    model = _model(cfg, g)
    srcs, tgts, extra = _golden_batch(g, case)
    pred, batch = _forward(model, srcs, tgts, extra)
    per = model.compute_loss(pred, batch, per_pair=True)
    again = model.compute_loss(pred, batch, per_pair=True)
    for k in per:
        assert per[k].shape == (2,) and torch.equal(per[k], again[k]), k
    full = model.compute_loss(pred, batch)
    full2 = model.compute_loss(pred, batch)
    for k in full:
        assert torch.equal(full[k], full2[k]), k
    for b in range(2):
        p1, b1 = _forward(model, [srcs[b]], [tgts[b]], {'pose': extra['pose'][b:b + 1], 'src_overlap': [extra['src_overlap'][b]],
                                                         'tgt_overlap': [extra['tgt_overlap'][b]]})
        one = model.compute_loss(p1, b1)
        for k in one:
            a, c = float(per[k][b]), float(one[k])
            assert abs(a - c) <= 1e-5 * max(abs(c), 1.0), (b, k, a, c)


def test_nan_pair_makes_total_nan():
    """The reference's 0 / 0: a pair without an anchor inside r_p gives a NaN feature term, and total = sum(w * term) is NaN."""
    case = '3dmatch_crop_b2'
    g = gold(f'losses_{case}')
    cfg = load_cfg('3dmatch')
    model = _model(cfg, g)
    srcs, tgts, extra = _golden_batch(g, case)
    extra['pose'] = extra['pose'].clone()
    extra['pose'][1, :, 3] += 100.0                            # pair 1's anchors land far from every target
    pred, batch = _forward(model, srcs, tgts, extra)
    per = model.compute_loss(pred, batch, per_pair=True)
    assert torch.isnan(per['feature_5'][1]) and torch.isnan(per['feature_un'][1]) and torch.isnan(per['total'][1])
    assert torch.isfinite(per['total'][0])
    full = model.compute_loss(pred, batch)
    assert torch.isnan(full['feature_5']) and torch.isnan(full['total']) and torch.isfinite(full['overlap_5'])


def test_compute_loss_no_host_sync():
    case = '3dmatch_crop_b2'
    g = gold(f'losses_{case}')
    cfg = load_cfg('3dmatch')
    model = _model(cfg, g)
    srcs, tgts, extra = _golden_batch(g, case)
    pred, batch = _forward(model, srcs, tgts, extra)
    model.compute_loss(pred, batch)                            # weight preparation (once per weight version)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = model.compute_loss(pred, batch)
        out_pp = model.compute_loss(pred, batch, per_pair=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(out['total'])
    # the mode does trip on this build: a device -> host read inside it raises
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            float(out['total'])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out_pp['total'].shape == (2,)


# ---------------------------------------------------------------------------------------------------- GT masks
def test_compute_overlap_masks_equal_per_pair():
    from regtr_amd import ops
    from regtr_amd.overlap import compute_overlap, compute_overlap_masks
    rng = np.random.default_rng(21)
    g = gold('overlap_pairs')
    srcs, tgts, radii = [], [], []
    for i in range(int(g['n_cases'])):
        srcs.append(g[f'src_{i}']); tgts.append(g[f'tgt_{i}']); radii.append(float(g[f'radius_{i}']))
    for n in (0, 1, 5, 700, 3000):                              # ragged synthetic, an empty cloud included
        srcs.append(rng.uniform(0, 1, (n, 3)).astype(F32)); tgts.append(rng.uniform(0, 1, (max(n // 2, 1), 3)).astype(F32))
    c, s = np.cos(0.2), np.sin(0.2)
    poses = np.stack([np.array([[c, -s, 0, 0.01 * k], [s, c, 0, 0], [0, 0, 1, -0.01]]) for k in range(len(srcs))]).astype(F32)
    for radius in (0.0375, 0.05):
        sm, tm = compute_overlap_masks([torch.from_numpy(x).cuda() for x in srcs], [torch.from_numpy(x).cuda() for x in tgts],
                                       torch.from_numpy(poses), radius)
        for k in range(len(srcs)):
            seg = torch.tensor([0, len(srcs[k])], dtype=torch.int32, device='cuda')
            sw = ops.se3_transform(torch.from_numpy(srcs[k]).cuda(), seg, torch.from_numpy(poses[k:k + 1]).cuda()) if len(srcs[k]) else \
                torch.zeros((0, 3), device='cuda')
            assert np.array_equal(sw.cpu().numpy(), _transform_f32(poses[k], srcs[k]) if len(srcs[k]) else np.zeros((0, 3), F32))
            if len(srcs[k]) == 0:
                assert sm[k].numel() == 0 and not tm[k].any().item()
                continue
            hs, ht, _ = compute_overlap(sw, torch.from_numpy(tgts[k]).cuda(), radius)
            assert np.array_equal(sm[k].cpu().numpy(), hs) and np.array_equal(tm[k].cpu().numpy(), ht), (radius, k)


# ---------------------------------------------------------------------------------------------------- test.py --losses
def _run_test_py(tmp, args):
    cmd = [sys.executable, os.path.join(ROOT, 'test.py'), '--config', os.path.join(ROOT, 'regtr_amd', 'conf', '3dmatch.yaml'),
           '--logdir', str(tmp), '--name', 'x'] + args
    r = subprocess.run(cmd, cwd=str(tmp), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout + r.stderr


def _est_logs(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            if f == 'est.log':
                with open(os.path.join(d, f), 'rb') as fh:
                    out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_test_py_losses(tmp_path):
    """test.py --synthetic 128 --batch 64 --losses --dev (seeded checkpoint): exit 0, a [Losses] line equal to the mean of B = 1
    compute_loss over the same pairs (1e-5), and est.log byte for byte that of the run without --losses."""
    from regtr_amd import RegTR
    from regtr_amd.harness import SyntheticPairs
    from regtr_amd.overlap import compute_overlap_masks
    cfg = load_cfg('3dmatch')
    sd = seeded_sd(cfg)
    gen = torch.Generator().manual_seed(7)
    for k in ('feature_criterion.W', 'feature_criterion_un.W'):
        sd[k] = torch.randn(sd[k].shape, generator=gen) * 0.01
    ckpt = tmp_path / 'model.pth'
    torch.save({'state_dict': sd}, str(ckpt))
    a, b = tmp_path / 'a' / 'run', tmp_path / 'b' / 'run'          # --dev logs to ../logdev: one per run
    a.mkdir(parents=True); b.mkdir(parents=True)
    common = ['--synthetic', '128', '--batch', '64', '--dev', '--resume', str(ckpt)]
    log_a = _run_test_py(a, common + ['--losses'])
    log_b = _run_test_py(b, common)
    line = [l for l in log_a.splitlines() if '[Losses]' in l]
    assert line and not any('[Losses]' in l for l in log_b.splitlines()), log_a[-2000:]
    kv = [x.split(':') for x in line[-1].split('[Losses]')[1].split('(')[0].split(',')]
    vals = {k.strip(): float(v) for k, v in kv}
    assert list(vals) == ['overlap_5', 'feature_5', 'feature_un', 'corr_5', 'total'], vals
    ea, eb = _est_logs(a.parent / 'logdev'), _est_logs(b.parent / 'logdev')
    assert ea and ea == eb, 'est.log differs with --losses'
    model = RegTR(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    pairs = SyntheticPairs(128, points=20000)
    acc = {k: 0.0 for k in vals}
    for i in range(128):
        it = pairs[i]
        s_, t_ = torch.from_numpy(it['src_xyz']).cuda(), torch.from_numpy(it['tgt_xyz']).cuda()
        pose = torch.from_numpy(it['pose'][None]).cuda()
        sm, tm = compute_overlap_masks([s_], [t_], pose, cfg.overlap_radius)
        batch = {'src_xyz': [s_], 'tgt_xyz': [t_]}
        pred = model(batch)
        batch.update({'pose': pose, 'src_overlap': sm, 'tgt_overlap': tm})
        for k, v in model.compute_loss(pred, batch).items():
            acc[k] += float(v) / 128
    print('test.py --losses:', vals, 'B = 1 mean:', acc)
    for k in vals:
        assert abs(vals[k] - acc[k]) <= 1e-5 * max(abs(acc[k]), 1.0), (k, vals[k], acc[k])


def test_run_test_losses_equal_mean_of_single_pair_losses():
    """harness.run_test(losses=True) with two replicas and B = 4 == the mean of B = 1 compute_loss over the same pairs (1e-5)."""
    from regtr_amd import harness
    from regtr_amd.overlap import compute_overlap_masks
    from regtr_amd.workload import replicate
    cfg = load_cfg('3dmatch')
    sd = seeded_sd(cfg)
    gen = torch.Generator().manual_seed(5)
    for k in ('feature_criterion.W', 'feature_criterion_un.W'):
        sd[k] = torch.randn(sd[k].shape, generator=gen) * 0.01
    from regtr_amd import RegTR
    model = RegTR(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    pairs = harness.SyntheticPairs(8, points=3000)
    models = replicate(model, cfg, 2, torch.device('cuda'))
    _, _, timing = harness.run_test(models, pairs, 4, torch.device('cuda'), losses=True)
    got = timing['losses']
    acc = {}
    for i in range(8):
        it = pairs[i]
        s, t = torch.from_numpy(it['src_xyz']).cuda(), torch.from_numpy(it['tgt_xyz']).cuda()
        pose = torch.from_numpy(it['pose'][None]).cuda()
        sm, tm = compute_overlap_masks([s], [t], pose, cfg.overlap_radius)
        batch = {'src_xyz': [s], 'tgt_xyz': [t]}
        pred = model(batch)
        batch.update({'pose': pose, 'src_overlap': sm, 'tgt_overlap': tm})
        for k, v in model.compute_loss(pred, batch).items():
            acc[k] = acc.get(k, 0.0) + float(v) / 8
    assert list(got) == list(acc)
    for k in acc:
        assert abs(got[k] - acc[k]) <= 1e-5 * max(abs(acc[k]), 1.0), (k, got[k], acc[k])
