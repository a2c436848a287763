"""The training-loss drop-ins (regtr_amd/losses.py) and their kernels on the GPU: losses and gradients against the REAL reference's
autograd (tests/golden/loss_grads_*.npz), the InfoNCE gradients against a float64 restatement with float32 error bounds over ragged
layouts, bit-identity with compute_loss's forward path, determinism, no host synchronisation, and a short AdamW optimisation."""
import numpy as np
import pytest
import torch

from tests import loss_grads_ref as R
from tests.test_gpu_losses import SIZES, _make_pairs
from tests.util import gold

pytestmark = pytest.mark.gpu

F32 = np.float32
R_P, R_N = 0.2, 0.4
CASES = ['3dmatch_crop_b2', '3dmatch_kitchen', 'modelnet_630']


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.requires_grad_() if grad else t


def _run_infonce(pairs, W, r_p=R_P, r_n=R_N):
    from regtr_amd.losses import InfoNCELossFull
    m = InfoNCELossFull(W.shape[0], r_p, r_n).cuda()
    with torch.no_grad():
        m.W.copy_(_t(W))
    fa = [_t(p[0], True) for p in pairs]
    fg = [_t(p[1], True) for p in pairs]
    loss = m(fa, fg, [_t(p[2]) for p in pairs], [_t(p[3]) for p in pairs])
    loss.backward()
    torch.cuda.synchronize()
    return (float(loss.detach()), [x.grad.cpu().numpy() for x in fa], [x.grad.cpu().numpy() for x in fg], m.W.grad.cpu().numpy())


@pytest.mark.parametrize('case', CASES)
def test_drop_ins_vs_reference_golden(case):
    from regtr_amd.losses import CorrCriterion
    g = gold(f'loss_grads_{case}')
    lg = gold(f'losses_{case}')
    B, D = int(g['n_pairs']), int(g['D'])
    src_kp = [lg[f'src_kp_{b}'] for b in range(B)]
    tgt_kp = [lg[f'tgt_kp_{b}'] for b in range(B)]
    src, tgt, W, w = R.draw_inputs([len(x) for x in src_kp], [len(x) for x in tgt_kp], D, int(g['feat_seed']))
    pairs = [(src[b].numpy(), tgt[b].numpy(), g[f'anc_xyz_{b}'], tgt_kp[b]) for b in range(B)]
    loss, dA, dG, dW = _run_infonce(pairs, W.numpy(), float(g['r_p']), float(g['r_n']))
    ref = float(g['loss_feat'])
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)
    rep = []
    for b in range(B):
        for got, r in ((dA[b], g[f'dA_{b}']), (dG[b], g[f'dG_{b}'])):
            err = np.abs(got - r).max() / np.abs(r).max()
            rep.append(err)
            assert err <= 1e-4, (b, err)
    err = np.abs(dW - g['dW']).max() / np.abs(g['dW']).max()
    assert err <= 1e-4 and np.all(np.tril(dW, -1) == 0), err
    # CorrCriterion on the reference's own correspondences
    crit = CorrCriterion('mae')
    wp = [_t(lg[f'src_kp_warped_{b}'], True) for b in range(B)]
    lc = crit([_t(x) for x in src_kp], wp, _t(lg['pose']), [x.cuda() for x in w])
    lc.backward()
    assert abs(float(lc) - float(g['loss_corr'])) <= 1e-5 * abs(float(g['loss_corr']))
    for b in range(B):
        r = g[f'dwarped_{b}']
        assert np.abs(wp[b].grad.cpu().numpy() - r).max() <= 1e-6 * np.abs(r).max(), b
    print(case, f'loss rel {abs(loss - ref) / abs(ref):.1e}, feature grads worst rel {max(rep):.1e}, dW rel {err:.1e}')


def infonce_grads_case(rng, sizes, D):
    """InfoNCELossFull forward + backward on ragged pairs of these sizes plus _make_pairs' three special pairs, against the float64
    restatement under its bounds: masks, lowest-index ties, exact zeros for the NaN pair, a strictly lower-triangular zero dW.
    -> (number of pairs, worst err / bound).  Shared with tests/test_gpu_bwd_routes.py (the other D instantiations)."""
    from regtr_amd import ops
    pairs = _make_pairs(rng, sizes, D)                    # + the NaN pair, the all-within-r_n pair, duplicated targets
    W = (rng.normal(0, 0.1, (D, D)) / np.sqrt(D / 64)).astype(F32)
    loss, dA, dG, dW = _run_infonce(pairs, W)
    assert np.isnan(loss)                                  # the NaN pair: 0 / 0 in the mean, as in the reference
    # the kernel's own decisions (float32 distances) -- the restatement uses them with float64 arithmetic
    A = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    G = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    off = lambda k: torch.tensor(np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])]), dtype=torch.int32).cuda()
    Wt = np.triu(W)
    P = ops.gemm(G, torch.from_numpy((Wt + Wt.T).astype(F32)).cuda())
    _, lse, idx, rm = ops.infonce_rows(A, P, _t(np.concatenate([p[2] for p in pairs])), _t(np.concatenate([p[3] for p in pairs])),
                                       off(0), off(1), max(len(p[0]) for p in pairs), R_P, R_N)
    idx, rm = idx.cpu().numpy(), rm.cpu().numpy()
    a_off = off(0).cpu().numpy()
    p_off = off(1).cpu().numpy()
    dec = []
    for b, p in enumerate(pairs):
        i_r, m_r, allowed = R.decisions(p[2], p[3], R_P, R_N)
        sl = slice(a_off[b], a_off[b + 1])
        assert np.array_equal(idx[sl] - p_off[b], i_r) and np.array_equal(rm[sl] != 0, m_r), b   # lowest-j ties, masks
        dec.append((i_r, m_r, allowed))
    _, rA, rG, rW, bA, bG, bW = R.infonce_grads([p[0] for p in pairs], [p[1] for p in pairs], W, dec, bounds=True)
    worst = 0.0
    for b in range(len(pairs)):
        for got, r, bd in ((dA[b], rA[b], bA[b]), (dG[b], rG[b], bG[b])):
            q = np.abs(got - r) / (bd + 1e-30)
            assert np.all(q <= 1.0), (b, float(q.max()))
            worst = max(worst, float(q.max()))
    q = np.abs(dW - rW) / (bW + 1e-30)
    assert np.all(q <= 1.0), float(q.max())
    worst = max(worst, float(q.max()))
    nan_pair, zero_pair = len(pairs) - 3, len(pairs) - 2
    assert np.all(dA[nan_pair] == 0) and np.all(dG[nan_pair] == 0)          # exactly 0, as torch autograd of an empty mask
    assert np.all(np.tril(dW, -1) == 0)
    return len(pairs), worst


@pytest.mark.parametrize('D', [64, 256, 512])
@pytest.mark.parametrize('layout', ['sizes', 'ragged'])
def test_infonce_grads_vs_float64(D, layout):
    rng = np.random.default_rng(100 + D + (0 if layout == 'sizes' else 1))
    if layout == 'sizes':
        sizes = [(SIZES[i], SIZES[(7 * i + 3) % len(SIZES)]) for i in range(len(SIZES) - 1)] + [(1, 1), (1, 40), (40, 1)]
    else:
        sizes = [(int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(13)]
    n_pairs, worst = infonce_grads_case(rng, sizes, D)
    print(f'infonce grads D={D} {layout}: {n_pairs} pairs, worst err/bound {worst:.3f}')


def test_forward_bit_identical_to_compute_loss_path():
    """The drop-in's value equals compute_loss's feature term (ops.infonce on G W_sym with the pose applied on load) bit for bit."""
    from regtr_amd import ops
    from regtr_amd.losses import InfoNCELossFull
    rng = np.random.default_rng(5)
    pairs = _make_pairs(rng, [(394, 400), (120, 77), (33, 129)], 256, specials=False)
    B = len(pairs)
    c, s = np.cos(0.4), np.sin(0.4)
    poses = np.stack([np.array([[c, -s, 0, 0.1 * b], [s, c, 0, -0.2], [0, 0, 1, 0.05]]) for b in range(B)]).astype(F32)
    m = InfoNCELossFull(256, R_P, R_N).cuda()
    seg = torch.tensor(np.concatenate([[0], np.cumsum([len(p[2]) for p in pairs])]), dtype=torch.int32).cuda()
    ax = _t(np.concatenate([p[2] for p in pairs]))
    ax_t = ops.se3_transform(ax, seg, _t(poses))
    anc = list(torch.split(ax_t, [len(p[2]) for p in pairs]))
    with torch.no_grad():
        got = m([_t(p[0]) for p in pairs], [_t(p[1]) for p in pairs], anc, [_t(p[3]) for p in pairs])
        A = _t(np.concatenate([p[0] for p in pairs]))
        G = _t(np.concatenate([p[1] for p in pairs]))
        w = torch.triu(m.W)
        P = ops.gemm(G, (w + w.t()).contiguous())
        p_seg = torch.tensor(np.concatenate([[0], np.cumsum([len(p[3]) for p in pairs])]), dtype=torch.int32).cuda()
        out = ops.infonce(A, P, ax, _t(np.concatenate([p[3] for p in pairs])), seg, p_seg, max(len(p[0]) for p in pairs), R_P, R_N,
                          anc_pose=_t(poses.reshape(B, 12)))
        ref = (out[:, 0] / out[:, 1]).mean()
    assert torch.isfinite(ref) and torch.equal(got, ref)


def _kitchen_like(seed=7, D=256):
    rng = np.random.default_rng(seed)
    return _make_pairs(rng, [(410, 339), (394, 400), (611, 129)], D, specials=True), rng


def test_grads_bit_reproducible():
    pairs, rng = _kitchen_like()
    W = rng.normal(0, 0.1, (256, 256)).astype(F32)
    a = _run_infonce(pairs, W)
    b = _run_infonce(pairs, W)
    for x, y in zip(a[1] + a[2] + [a[3]], b[1] + b[2] + [b[3]]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_double_backward_refused():
    from regtr_amd.losses import CorrCriterion, InfoNCELossFull
    pairs, _ = _kitchen_like()
    m = InfoNCELossFull(256, R_P, R_N).cuda()
    fa = [_t(p[0], True) for p in pairs[:2]]
    loss = m(fa, [_t(p[1]) for p in pairs[:2]], [_t(p[2]) for p in pairs[:2]], [_t(p[3]) for p in pairs[:2]])
    (gA,) = torch.autograd.grad(loss, fa[0], create_graph=True)
    with pytest.raises(RuntimeError):
        gA.sum().backward()
    kp = [_t(pairs[0][2])]
    wp = [_t(pairs[0][2] + F32(0.01), True)]
    lc = CorrCriterion()(kp, wp, _t(np.eye(4, dtype=F32)[:3][None]), [torch.ones(len(pairs[0][2]), device='cuda')])
    (gw,) = torch.autograd.grad(lc, wp[0], create_graph=True)
    with pytest.raises(RuntimeError):
        gw.sum().backward()


def test_no_host_sync():
    from regtr_amd.losses import CorrCriterion, InfoNCELossFull
    pairs, _ = _kitchen_like()
    m = InfoNCELossFull(256, R_P, R_N).cuda()
    crit = CorrCriterion()
    fa = [_t(p[0], True) for p in pairs]
    fg = [_t(p[1], True) for p in pairs]
    ax, px = [_t(p[2]) for p in pairs], [_t(p[3]) for p in pairs]
    wp = [_t(p[2] + F32(0.01), True) for p in pairs]
    pose = _t(np.stack([np.eye(4, dtype=F32)[:3]] * len(pairs)))
    wts = [torch.rand(len(p[2]), device='cuda') for p in pairs]

    def step():
        total = m(fa[:-3] + fa[-2:], fg[:-3] + fg[-2:], ax[:-3] + ax[-2:], px[:-3] + px[-2:]) + crit(ax, wp, pose, wts)
        total.backward()
        return total
    step()                                                  # first-call preparation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        total = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(total) and torch.isfinite(m.W.grad).all()


def _restated_losses(A, G, W, dec, ax_list, warped, kp, T, w):
    """Float64 torch restatement (the same decisions) of the two drop-ins' values, differentiable."""
    Wt = torch.triu(W)
    Ws = Wt + Wt.t()
    per = []
    for b in range(len(A)):
        idx, mask, allowed = (torch.from_numpy(x).to(A[b].device) for x in dec[b])
        l = A[b] @ (G[b] @ Ws).t()
        lm = l.masked_fill(~allowed, float('-inf'))
        li = torch.logsumexp(lm, -1) - l.gather(1, idx[:, None]).squeeze(1)
        per.append(li[mask].sum() / mask.sum())
    feat = torch.stack(per).mean()
    e = torch.cat([warped[b] - (kp[b] @ T[b][:, :3].t() + T[b][:, 3]) for b in range(len(kp))])
    ww = torch.cat(w)
    corr = (ww * e.abs().sum(-1)).sum() / ww.sum().clamp_min(1e-6)
    return feat, corr


def test_adamw_tracks_float64_restatement():
    from regtr_amd.losses import CorrCriterion, InfoNCELossFull
    pairs, rng = _kitchen_like(11, 64)
    pairs = pairs[:3] + pairs[-2:]                          # no NaN pair: a finite loss to optimise
    dec = [R.decisions(p[2], p[3], R_P, R_N) for p in pairs]
    dec = [(i.astype(np.int64), m, a) for i, m, a in dec]
    T = np.stack([np.eye(4, dtype=F32)[:3]] * len(pairs))
    T[:, :, 3] = rng.normal(0, 0.1, (len(pairs), 3))
    kp = [p[2] for p in pairs]
    warped0 = [(x + rng.normal(0, 0.05, x.shape)).astype(F32) for x in kp]
    w = [rng.uniform(0, 1, len(x)).astype(F32) for x in kp]
    W0 = rng.normal(0, 0.1, (64, 64)).astype(F32)

    m = InfoNCELossFull(64, R_P, R_N).cuda()
    with torch.no_grad():
        m.W.copy_(_t(W0))
    crit = CorrCriterion()
    fa = [torch.nn.Parameter(_t(p[0])) for p in pairs]
    fg = [torch.nn.Parameter(_t(p[1])) for p in pairs]
    wp = [torch.nn.Parameter(_t(x)) for x in warped0]
    opt = torch.optim.AdamW([m.W, *fa, *fg, *wp], lr=1e-2)
    dd = lambda x: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(x)).double().cuda())
    W64, fa64, fg64, wp64 = dd(W0), [dd(p[0]) for p in pairs], [dd(p[1]) for p in pairs], [dd(x) for x in warped0]
    opt64 = torch.optim.AdamW([W64, *fa64, *fg64, *wp64], lr=1e-2)
    ax, px = [_t(p[2]) for p in pairs], [_t(p[3]) for p in pairs]
    kp64 = [torch.from_numpy(x).double().cuda() for x in kp]
    T64 = torch.from_numpy(T).double().cuda()
    w64 = [torch.from_numpy(x).double().cuda() for x in w]
    hist, hist64 = [], []
    for _ in range(30):
        opt.zero_grad()
        lf = m(fa, fg, ax, px)
        lc = crit([_t(x) for x in kp], wp, _t(T), [_t(x) for x in w])
        (lf + lc).backward()
        opt.step()
        opt64.zero_grad()
        f64, c64 = _restated_losses(fa64, fg64, W64, dec, ax, wp64, kp64, T64, w64)
        (f64 + c64).backward()
        opt64.step()
        hist.append((float(lf), float(lc)))
        hist64.append((float(f64), float(c64)))
    h, h64 = np.array(hist), np.array(hist64)
    assert np.all(np.abs(h - h64) <= 2e-3 * np.abs(h64) + 1e-5), np.abs(h - h64).max()
    assert h[-1, 0] < 0.5 * h[0, 0] and h[-1, 1] < h[0, 1]
    print('AdamW 30 steps: feature', h[0, 0], '->', h[-1, 0], 'corr', h[0, 1], '->', h[-1, 1],
          'worst rel gap', float((np.abs(h - h64) / np.abs(h64)).max()))
