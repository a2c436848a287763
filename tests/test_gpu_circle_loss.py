"""CircleLossFull on the GPU (regtr_amd/losses.py, csrc/circle_loss.hip): the drop-in against the REAL reference's float64 autograd
(tests/golden/circle_loss_*.npz), against the float64 restatement under its derived float32 bounds over ragged pairs that cross every
tile edge (owned rows: 32, streamed columns: 64, feature chunks: 64) and the special pairs, bit-identity with RegTR.compute_loss,
determinism, no host synchronisation, refusals, and the model's training / validation steps under `feature_loss_type: circle`."""
import numpy as np
import pytest
import torch

from tests import circle_loss_ref as R
from tests.test_circle_loss_host import BAD, CASES, circle_call, golden_inputs
from tests.util import gold, load_cfg, seeded_sd

pytestmark = pytest.mark.gpu

F32 = np.float32
R_P, R_N = 0.25, 0.5            # exactly representable: the grid pair below puts coordinate distances ON both radii
# CL_TR = 32 owned rows, CL_TC = 64 streamed columns; either side of a pair is rows in one pass and columns in the other
EDGE_SIZES = [(1, 1), (1, 70), (70, 1), (31, 65), (32, 64), (33, 63), (63, 33), (64, 32), (65, 31), (127, 129), (129, 127), (200, 97)]


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.requires_grad_() if grad else t


def _feat(rng, n, D, lo=0.3, hi=1.3):
    """Unit directions scaled by U(lo, hi) / sqrt(2): feature distances about both margins."""
    v = rng.normal(0, 1, (n, D))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * rng.uniform(lo, hi, (n, 1)) / np.sqrt(2.0)).astype(F32)


def _pair(rng, ns, nt, D, side=None):
    side = side or max(0.7, 0.3 * (max(ns, nt) ** (1 / 3)))
    return (_feat(rng, ns, D), _feat(rng, nt, D), rng.uniform(0, side, (ns, 3)).astype(F32), rng.uniform(0, side, (nt, 3)).astype(F32))


def _special_pairs(rng, D):
    """name -> pair; see test_grads_vs_float64 for what each must give."""
    sp = {}
    a, g, ax, px = _pair(rng, 40, 70, D)
    sp['no_pos'] = (a, g, ax, (px + F32(10.0)).astype(F32))                    # nothing inside r_p
    sp['no_neg'] = _pair(rng, 40, 70, D, side=0.1)                             # everything inside r_p, nothing beyond r_n
    # rows selected, no column: ONE anchor with a positive in column 0 and negatives in columns 2..; no column holds a pos and a neg
    px1 = np.zeros((9, 3), F32)
    px1[0, 0] = 0.125
    px1[1, 0] = 0.375                                                          # between the radii: neither
    px1[2:, 0] = 1.0
    sp['rows_only'] = (_feat(rng, 1, D), _feat(rng, 9, D), np.zeros((1, 3), F32), px1)
    # a 0.25 lattice: coordinate distances exactly r_p = 0.25 and exactly r_n = 0.5 -> neither positive nor negative (both strict)
    gx = np.array([[i * 0.25, j * 0.25, 0.0] for i in range(5) for j in range(5)], F32)
    sp['grid'] = (_feat(rng, 25, D), _feat(rng, 25, D), gx, (gx + F32([0.0, 0.0, 0.125])).astype(F32)[::-1].copy())
    sp['grid_on'] = (_feat(rng, 25, D), _feat(rng, 25, D), gx, gx.copy())
    # duplicate features: d = sqrt(1e-12) = 1e-6, finite gradients, zero weight on those positives
    a, g, ax, px = _pair(rng, 50, 45, D)
    g[:20] = a[:20]
    px[:20] = ax[:20]
    sp['duplicates'] = (a, g, ax, px)
    # feature distances around 12: tp up to s * 11.9^2 ~ 1.4e3, exponents far beyond float32's exp range without the max subtraction
    _, _, ax, px = _pair(rng, 45, 50, D)
    sp['far'] = ((_feat(rng, 45, D, 1.25, 1.35) * F32(13.0)).astype(F32), (_feat(rng, 50, D) * F32(0.2)).astype(F32), ax, px)
    return sp


def _run(pairs, r_p=R_P, r_n=R_N, crit=None):
    from regtr_amd.losses import CircleLossFull
    m = crit or CircleLossFull('euclidean', r_p=r_p, r_n=r_n)
    fa = [_t(p[0], True) for p in pairs]
    fg = [_t(p[1], True) for p in pairs]
    loss = m(fa, fg, [_t(p[2]) for p in pairs], [_t(p[3]) for p in pairs])
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), [x.grad.cpu().numpy() for x in fa], [x.grad.cpu().numpy() for x in fg]


def _stats(pairs, r_p=R_P, r_n=R_N):
    """ops.circle_rows on the packed pairs -> (pair_out, anc_sel, pos_sel) numpy."""
    from regtr_amd import ops
    cat = lambda k: _t(np.concatenate([p[k] for p in pairs]))
    off = lambda k: torch.tensor(np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])]), dtype=torch.int32).cuda()
    out, _, a_sel, _, p_sel = ops.circle_rows(cat(0), cat(1), cat(2), cat(3), off(0), off(1), max(len(p[0]) for p in pairs),
                                              max(len(p[1]) for p in pairs), r_p, r_n)
    return out.cpu().numpy(), a_sel.cpu().numpy(), p_sel.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- the feature's own test
def test_circle_is_served():
    """Fails without the feature: the import, and compute_loss / training_step on a circle config (NotImplementedError before)."""
    from regtr_amd.losses import CircleLossFull          # noqa: F401
    s = _model_setup()
    b = s['batch']()
    with torch.no_grad():
        pred = s['model'](b)
        losses = s['model'].compute_loss(pred, b)
    assert list(losses) == s['model'].loss_keys() and all(torch.isfinite(v) for v in losses.values())


# ---------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize('case', CASES)
def test_drop_in_vs_reference_golden(case):
    g, pairs = golden_inputs(case)
    loss, dA, dG = _run(pairs, float(g['r_p']), float(g['r_n']))
    ref = float(g['loss'])
    print(case, f'loss {loss:.8f} vs {ref:.8f}: rel {abs(loss - ref) / abs(ref):.1e}')
    rep = []
    for b in range(len(pairs)):
        for got, r in ((dA[b], g[f'dA_{b}']), (dG[b], g[f'dG_{b}'])):
            rep.append(float(np.abs(got - r).max() / np.abs(r).max()))
    print(case, 'gradients, worst error / max per tensor:', ' '.join(f'{e:.1e}' for e in rep))
    out, _, _ = _stats(pairs, float(g['r_p']), float(g['r_n']))
    assert list(out[:, 1]) == list(g['n_rows']) and list(out[:, 3]) == list(g['n_cols'])
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)
    assert max(rep) <= 1e-4, rep


# ---------------------------------------------------------------------------------------------------- float64 restatement
def grads_case(pairs, names, r_p=R_P, r_n=R_N):
    """Forward + backward on `pairs` against the restatement under its bounds; the selection flags and counts exactly.
    -> worst err / bound."""
    loss, dA, dG = _run(pairs, r_p, r_n)
    msk = [R.masks(p[2], p[3], r_p, r_n) for p in pairs]
    ref, per, rA, rG, cnt, bper, bA, bG = R.circle([p[0] for p in pairs], [p[1] for p in pairs], msk, bounds=True)
    out, a_sel, p_sel = _stats(pairs, r_p, r_n)
    a_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])])
    p_off = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])])
    worst = 0.0
    for b, p in enumerate(pairs):
        pos, neg = msk[b]
        assert np.array_equal(a_sel[a_off[b]:a_off[b + 1]] != 0, pos.any(1) & neg.any(1)), names[b]
        assert np.array_equal(p_sel[p_off[b]:p_off[b + 1]] != 0, pos.any(0) & neg.any(0)), names[b]
        assert (int(out[b, 1]), int(out[b, 3])) == cnt[b], names[b]
        got = (out[b, 0] / out[b, 1] + out[b, 2] / out[b, 3]) / 2 if min(cnt[b]) > 0 else np.nan
        if np.isnan(per[b]):
            assert min(cnt[b]) == 0 and np.all(dA[b] == 0) and np.all(dG[b] == 0), names[b]       # exactly 0
            continue
        q = abs(got - per[b]) / bper[b]
        print(f'  {names[b]}: pair loss {got:.7f} (float64 {per[b]:.7f}) err / bound {q:.3f}')
        assert q <= 1.0, (names[b], got, per[b], bper[b])
        worst = max(worst, q)
        for got_g, r, bd in ((dA[b], rA[b], bA[b]), (dG[b], rG[b], bG[b])):
            assert np.all(np.isfinite(got_g)), names[b]
            q = np.abs(got_g - r) / (bd + 1e-30)
            worst = max(worst, float(q.max()))
            assert np.all(q <= 1.0), (names[b], float(q.max()))
    assert np.isnan(loss) == bool(np.isnan(ref))
    if not np.isnan(ref):
        assert abs(loss - ref) <= float(np.mean(bper)) + 8 * R.U * abs(ref)
    return worst, msk, (rA, rG)


def test_grads_vs_float64_edges_and_specials():
    rng = np.random.default_rng(41)
    D = 64
    sp = _special_pairs(rng, D)
    pairs = [_pair(rng, ns, nt, D) for ns, nt in EDGE_SIZES] + list(sp.values())
    names = [f'{ns}x{nt}' for ns, nt in EDGE_SIZES] + list(sp)
    worst, msk, (rA, rG) = grads_case(pairs, names)
    at = {n: i for i, n in enumerate(names)}
    cnt = lambda n: (int((msk[at[n]][0].any(1) & msk[at[n]][1].any(1)).sum()), int((msk[at[n]][0].any(0) & msk[at[n]][1].any(0)).sum()))
    # what the special pairs are built to be (grads_case has checked: NaN pairs give exactly zero rows)
    assert not msk[at['no_pos']][0].any() and msk[at['no_pos']][1].all() and cnt('no_pos') == (0, 0)
    assert msk[at['no_neg']][0].all() and not msk[at['no_neg']][1].any() and cnt('no_neg') == (0, 0)
    assert cnt('rows_only') == (1, 0)
    pos, neg = msk[at['grid_on']]
    gx = pairs[at['grid_on']][2].astype(np.float64)
    dd = np.linalg.norm(gx[:, None] - gx[None], axis=-1)
    assert (dd == 0.25).sum() >= 40 and (dd == 0.5).sum() >= 30                    # distances ON the radii ...
    assert not pos[dd == 0.25].any() and not neg[dd == 0.5].any() and pos[dd == 0].all() and neg[dd > 0.5].all()      # ... are neither
    assert min(cnt('grid_on')) > 0 and min(cnt('grid')) > 0
    a, g = pairs[at['duplicates']][0].astype(np.float64), pairs[at['duplicates']][1].astype(np.float64)
    assert np.all(a[:20] == g[:20]) and msk[at['duplicates']][0][np.arange(20), np.arange(20)].all() and min(cnt('duplicates')) > 0
    a, g = pairs[at['far']][0].astype(np.float64), pairs[at['far']][1].astype(np.float64)
    dfar = np.linalg.norm(a[:, None] - g[None], axis=-1)
    assert 11.0 < dfar.min() and dfar.max() < 13.0 and min(cnt('far')) > 0 and msk[at['far']][0].any()
    assert np.abs(rA[at['far']]).max() > 0
    assert min(min(cnt(f'{ns}x{nt}')) for ns, nt in EDGE_SIZES[3:]) > 0
    print(f'circle grads D={D}: {len(pairs)} pairs, worst err / bound {worst:.3f}')


@pytest.mark.parametrize('D', [128, 192, 256, 320, 384, 448, 512])
def test_grads_vs_float64_every_width(D):
    """Every D instantiation on two pairs whose sizes cross the row and the column tile."""
    rng = np.random.default_rng(50 + D)
    sizes = [(33, 65), (129, 31)]
    pairs = [_pair(rng, ns, nt, D) for ns, nt in sizes]
    worst, msk, _ = grads_case(pairs, [f'{a}x{b}' for a, b in sizes])
    print(f'circle grads D={D}: worst err / bound {worst:.3f}')


# ---------------------------------------------------------------------------------------------------- consistency, behaviour
def test_forward_bit_identical_to_compute_loss_path():
    """The drop-in's value equals compute_loss's feature term (ops.circle_rows on the packed tokens, the pose applied on load)."""
    from regtr_amd import ops
    from regtr_amd.losses import CircleLossFull
    rng = np.random.default_rng(5)
    pairs = [_pair(rng, ns, nt, 256) for ns, nt in [(394, 400), (120, 77), (33, 129)]]
    B = len(pairs)
    c, s = np.cos(0.4), np.sin(0.4)
    poses = np.stack([np.array([[c, -s, 0, 0.1 * b], [s, c, 0, -0.2], [0, 0, 1, 0.05]]) for b in range(B)]).astype(F32)
    m = CircleLossFull('euclidean', r_p=R_P, r_n=R_N)
    n_src = [len(p[0]) for p in pairs]
    lens = n_src + [len(p[1]) for p in pairs]
    seg_c = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
    feats = _t(np.concatenate([p[0] for p in pairs] + [p[1] for p in pairs]))
    xyz = _t(np.concatenate([p[2] for p in pairs] + [p[3] for p in pairs]))
    ax_t = ops.se3_transform(xyz[:sum(n_src)].contiguous(), seg_c[:B + 1].contiguous(), _t(poses))
    with torch.no_grad():
        got = m([_t(p[0]) for p in pairs], [_t(p[1]) for p in pairs], list(torch.split(ax_t, n_src)), [_t(p[3]) for p in pairs])
        out = ops.circle_rows(feats, feats, xyz, xyz, seg_c[:B + 1], seg_c[B:], max(n_src), max(lens[B:]), R_P, R_N, m.params(),
                              anc_pose=_t(poses.reshape(B, 12)))[0]
        ref = ((out[:, 0] / out[:, 1] + out[:, 2] / out[:, 3]) / 2).mean()
    assert torch.isfinite(ref) and torch.equal(got, ref)


def _kitchen_like(seed=7, D=256):
    rng = np.random.default_rng(seed)
    return [_pair(rng, ns, nt, D) for ns, nt in [(410, 339), (394, 400), (611, 129)]]


def test_grads_bit_reproducible():
    pairs = _kitchen_like()
    a, b = _run(pairs), _run(pairs)
    assert a[0] == b[0] and np.isfinite(a[0])
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.abs(x).max() > 0


def test_no_host_sync():
    from regtr_amd.losses import CircleLossFull
    pairs = _kitchen_like()
    m = CircleLossFull('euclidean', r_p=R_P, r_n=R_N)
    fa = [_t(p[0], True) for p in pairs]
    fg = [_t(p[1], True) for p in pairs]
    ax, px = [_t(p[2]) for p in pairs], [_t(p[3]) for p in pairs]

    def step():
        total = m(fa, fg, ax, px)
        total.backward()
        return total
    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        total = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(total) and all(torch.isfinite(x.grad).all() for x in fa + fg)


def test_refusals():
    from regtr_amd.losses import CircleLossFull
    pairs = _kitchen_like(D=64)[:2]
    m = CircleLossFull('euclidean', r_p=R_P, r_n=R_N)
    fa = [_t(p[0], True) for p in pairs]
    args = lambda: ([_t(p[1]) for p in pairs], [_t(p[2]) for p in pairs], [_t(p[3]) for p in pairs])
    loss = m(fa, *args())
    (gA,) = torch.autograd.grad(loss, fa[0], create_graph=True)
    with pytest.raises(RuntimeError):
        gA.sum().backward()                                  # double backward
    fg, ax, px = args()
    with pytest.raises(NotImplementedError, match='cosine'):
        CircleLossFull(r_p=R_P, r_n=R_N)(fa, fg, ax, px)
    with pytest.raises(RuntimeError):
        m(fa, fg, [x.clone().requires_grad_() for x in ax], px)
    with pytest.raises(RuntimeError):
        m([x.double() for x in fa], fg, ax, px)
    with pytest.raises(RuntimeError):
        m([x.cpu() for x in fa], fg, ax, px)
    with pytest.raises(RuntimeError):
        m([fa[0][:0], fa[1]], fg, [ax[0][:0], ax[1]], px)    # an empty cloud
    # the attributes are read at every call
    base = float(m(fa, fg, ax, px))
    m.log_scale, m.neg_margin, m.neg_optimal = 4.0, 1.1, 1.2
    msk = [R.masks(p[2], p[3], R_P, R_N) for p in pairs]
    ref = R.circle([p[0] for p in pairs], [p[1] for p in pairs], msk, params=m.params())[0]
    got = float(m(fa, fg, ax, px))
    assert abs(got - ref) <= 1e-5 * abs(ref) and abs(got - base) > 1e-3
    # argument errors: a status, nothing launched (the pointers are never dereferenced)
    for bwd in (False, True):
        for kw in BAD:
            assert circle_call(bwd, **kw) == -2, kw
    assert circle_call(True, mean_div=0.0) == -2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the model
_shared = {}
CASE = '3dmatch_crop_b2'


def _model_setup():
    if _shared:
        return _shared
    from regtr_amd import RegTR
    from tests.test_gpu_losses import _golden_batch
    g = gold(f'losses_{CASE}')
    cfg = load_cfg('3dmatch')
    cfg.update({'feature_loss_type': 'circle'})
    cfg.wt_feature_un = 0.05
    model = RegTR(cfg)
    model.load_state_dict(seeded_sd(cfg), strict=True)
    model = model.cuda().eval()
    srcs, tgts, extra = _golden_batch(g, CASE)

    def batch():
        b = {'src_xyz': [torch.from_numpy(s).cuda() for s in srcs], 'tgt_xyz': [torch.from_numpy(t).cuda() for t in tgts]}
        b.update(extra)
        return b
    _shared.update(model=model, batch=batch, cfg=cfg)
    return _shared


def test_compute_loss_per_pair_and_drop_in():
    """compute_loss's feature terms: bit-equal to CircleLossFull.forward on the same tokens; per_pair=True averages to the scalar."""
    from regtr_amd import ops
    s = _model_setup()
    model, b = s['model'], s['batch']()
    with torch.no_grad():
        pred = model(b)
        scalar = model.compute_loss(pred, b)
        per = model.compute_loss(pred, b, per_pair=True)
        B = len(pred['src_kp'])
        n_src = [int(x.shape[0]) for x in pred['src_kp']]
        seg = torch.tensor(np.concatenate([[0], np.cumsum(n_src)]), dtype=torch.int32).cuda()
        pose = torch.stack(list(b['pose'])) if isinstance(b['pose'], (list, tuple)) else b['pose']
        pose = pose.to(device='cuda', dtype=torch.float32).contiguous()
        anc = ops.se3_transform(torch.cat(list(pred['src_kp'])).contiguous(), seg, pose)
        crit = model.feature_criterion
        for key, fs, ft in ([(f'feature_{i}', [f[i] for f in pred['src_feat']], [f[i] for f in pred['tgt_feat']])
                             for i in s['cfg'].feature_loss_on] + [('feature_un', list(pred['src_feat_un']), list(pred['tgt_feat_un']))]):
            got = crit([f.contiguous() for f in fs], [f.contiguous() for f in ft], list(torch.split(anc, n_src)), list(pred['tgt_kp']))
            assert torch.isfinite(got) and torch.equal(got, scalar[key]), key
    for k in [k for k in scalar if k.startswith('feature')]:
        assert per[k].shape == (B,) and abs(float(per[k].mean()) - float(scalar[k])) <= 1e-6 * max(abs(float(scalar[k])), 1.0), k


def test_training_and_validation_steps():
    s = _model_setup()
    model = s['model']
    last = f'feature_{model.cfg.num_encoder_layers - 1}'
    params = model.trainable_parameters(backbone=True)
    state = [p.detach().clone() for p in model.parameters()]
    try:
        for p in model.parameters():
            p.grad = None
        pred, losses = model.training_step(s['batch'](), train_backbone=True)
        assert list(losses) == model.loss_keys() and last in losses
        assert all(torch.isfinite(v) for v in losses.values())
        losses['total'].backward()
        for p in params:
            assert p.grad is not None and torch.isfinite(p.grad).all()
        assert any(p.grad.abs().max() > 0 for p in params)
        with torch.no_grad():
            vl, vm = model.validation_step(s['batch'](), 0)
        assert list(vl) == list(losses) and all(torch.isfinite(v) for v in vl.values())
        opt = torch.optim.AdamW(params, lr=1e-4)
        hist = []
        for _ in range(6):                                   # the value before each of five steps, and after the last
            opt.zero_grad()
            _, losses = model.training_step(s['batch'](), train_backbone=True)
            hist.append(float(losses[last].detach()))
            if len(hist) == 6:
                break
            losses['total'].backward()
            opt.step()
        print(f'{last} over five AdamW steps:', ' '.join(f'{h:.5f}' for h in hist))
        assert all(np.isfinite(hist)) and hist[-1] < hist[0]
    finally:
        with torch.no_grad():
            for p, st in zip(model.parameters(), state):
                p.copy_(st)
