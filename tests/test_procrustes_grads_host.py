"""CPU: the weighted Procrustes backward's restatement (tests/procrustes_grads_ref.py) against the reference's own float64 autograd
(tests/golden/procrustes_grads.npz, tools/make_golden_procrustes_grads.py), its error bound against moved weights, the C ABI of the new
entry, the opt-in pose term's keys, and the refusal of CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

from tests import procrustes_grads_ref as R
from tests.util import ROOT, gold, load_cfg

OUTS = ('d_corr', 'd_logit', 'd_kp', 'd_weight')


def _model(g, **kw):
    return R.model_backward(g['kp'], g['corr'], g['logit'], g['seg_off'], g['d_pose'], **kw)


def _rel(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def _se3_restated(g, tag, roundings):
    a, b, dT = g['se3_a'], g['se3_b'], g['se3_dT']
    da, db, dw = np.zeros(a.shape), np.zeros(a.shape), np.zeros(a.shape[:-1])
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            w = g['se3_w'][i, j] if tag == '' else np.full(a.shape[2], 0.5, np.float32)
            da[i, j], db[i, j], _, dw[i, j], info = R.pair_backward(a[i, j], b[i, j], dT[i, j], w=w, roundings=roundings)
            assert not info['zeroed']
    return da, db, dw


@pytest.mark.parametrize('roundings,tol', [(False, 1e-9), (True, 1e-4)])
def test_restatement_vs_reference_autograd(roundings, tol):
    g = gold('procrustes_grads')
    out, infos = _model(g, roundings=roundings)
    errs = {k: _rel(out[k], g[k]) for k in OUTS}
    for tag in ('', '_none'):
        da, db, dw = _se3_restated(g, tag, roundings)
        errs[f'se3{tag}_da'], errs[f'se3{tag}_db'] = _rel(da, g[f'se3{tag}_da']), _rel(db, g[f'se3{tag}_db'])
        if tag == '':
            errs['se3_dw'] = _rel(dw, g['se3_dw'])
            assert np.isfinite(dw).all() and (g['se3_w'] == 0).any() and (g['se3_w'] == 1).any()
    print(f'restatement (float32 roundings {roundings}) vs the reference autograd, error / tensor maximum:', {k: f'{v:.2e}' for k, v in errs.items()})
    assert max(errs.values()) <= tol, errs
    ds = [[i['d'] for i in row] for row in infos]
    assert all(row[2] == -1.0 and row[0] == row[1] == row[3] == 1.0 for row in ds)          # pair 2 is the reflected case
    assert all(row[3]['S'][2] <= 1e-6 * row[3]['S'][0] for row in infos)                    # pair 3 is coplanar
    assert not any(i['zeroed'] for row in infos for i in row)


def test_bound_covers_a_moved_weight_and_is_not_vacuous():
    """The bound's first term is one float32 ulp on each w_i: moving every w_i of the restatement by an ulp (all up, all down, random
    signs) must stay inside it; and on the golden inputs it is at most 1e-5 of every output's maximum."""
    g = gold('procrustes_grads')
    ref, infos = _model(g)
    bound = R.pair_bounds(ref, infos)
    for k in OUTS:
        assert bound[k].max() <= 1e-5 * np.abs(ref[k]).max(), (k, bound[k].max() / np.abs(ref[k]).max())
    rng = np.random.default_rng(5)
    worst = 0.0
    for ul in (np.ones(g['logit'].shape, np.int32), -np.ones(g['logit'].shape, np.int32), rng.integers(-1, 2, g['logit'].shape)):
        out, _ = _model(g, w_ulps=ul)
        for k in OUTS:
            m = bound[k] > 0
            worst = max(worst, float((np.abs(out[k] - ref[k])[m] / bound[k][m]).max()))
    print(f'one ulp on every weight: worst change / bound {worst:.3f}')
    assert worst <= 1.0


def test_zero_gradient_rule_of_the_restatement():
    rng = np.random.default_rng(3)
    dp = rng.standard_normal((3, 4))
    a = rng.standard_normal((12, 3))
    line = np.outer(np.linspace(-1, 1, 12), [1.0, 2.0, -1.0])
    cases = {'one point': (a[:1], a[:1] + 1, np.zeros(1)), 'collinear': (line, line + 0.5, np.zeros(12)),
             'coincident': (np.ones((12, 3)), a, np.zeros(12)), 'clamp': (a, a + 0.1, np.full(12, -40.0)),
             'empty': (a[:0], a[:0], np.zeros(0))}
    for name, (x, y, lg) in cases.items():
        da, db, dl, dw, info = R.pair_backward(x.astype(np.float32), y.astype(np.float32), dp, logit=lg.astype(np.float32))
        assert info['zeroed'] and not da.any() and not db.any() and not dl.any() and not dw.any(), name
    _, _, _, _, info = R.pair_backward(a.astype(np.float32), (a @ np.diag([1.0, 0.9, 0.8])).astype(np.float32), dp, logit=np.zeros(12, np.float32))
    assert not info['zeroed']


def _cube():
    """The corners of a cube under a rigid motion, equal weights: S0 = S1 = S2, where the derivative of an SVD does not exist and the
    closed form (which divides by sums only) does."""
    a = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)]) * 0.5 + np.array([0.25, -0.5, 0.125])
    c, s = np.cos(0.75), np.sin(0.75)
    b = a @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]).T + np.array([0.5, 0.25, -0.125])
    return a, b, np.zeros(8), np.random.default_rng(9).standard_normal((3, 4))


def test_equal_singular_values_against_finite_differences():
    a, b, lg, dp = _cube()
    da, db, dl, dw, info = R.pair_backward(a, b, dp, logit=lg, roundings=False)
    assert not info['zeroed'] and info['S'][0] - info['S'][2] <= 1e-12 * info['S'][0] and abs(info['kappa'] - 0.5) <= 1e-9

    def value(a_, b_, lg_):
        f = R.pair_forward(a_, b_, lg_, roundings=False)
        return float((f['R'] * dp[:, :3]).sum() + ((f['cb'] - f['R'] @ f['ca']) * dp[:, 3]).sum())
    h = 1e-6
    worst = 0.0
    for which, grad in ((0, da), (1, db), (2, dl)):
        for idx in np.ndindex(grad.shape):
            args = [a.copy(), b.copy(), lg.copy()]
            args[which][idx] += h
            up = value(*args)
            args[which][idx] -= 2 * h
            fd = (up - value(*args)) / (2 * h)
            worst = max(worst, abs(fd - grad[idx]))
    scale = max(np.abs(da).max(), np.abs(db).max(), np.abs(dl).max())
    print(f'cube (S0 = S1 = S2): closed form vs central differences, worst {worst / scale:.2e} of the largest entry')
    assert worst <= 1e-7 * scale


def test_header_and_binding():
    from regtr_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    m = re.search(r'^int regtr_weighted_procrustes_bwd\(([^;]*)\);', hdr, re.M)
    assert m and len(m.group(1).split(',')) == 13
    assert 'regtr_weighted_procrustes_bwd ' in hdr.split('#ifndef REGTR_HIP_H')[0]                   # the mapping table at the top
    res, args = _lib.SIGNATURES['regtr_weighted_procrustes_bwd']
    assert len(args) == 13 and res is _lib._I
    assert re.search(r'#define\s+REGTR_ABI_VERSION\s+11\b', hdr) and _lib.ABI_VERSION == 11
    assert 'procrustes.hip' in build.SOURCES and callable(ops.weighted_procrustes_bwd)
    src = open(os.path.join(ROOT, 'regtr_amd', 'csrc', 'procrustes.hip')).read()
    assert 'atomicAdd' not in src and 'asm' not in src.replace('assembly', '')
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(_lib.lib(), 'regtr_weighted_procrustes_bwd')


def test_pose_term_keys():
    from regtr_amd import RegTR
    from regtr_amd.regtr import loss_weight_dict
    for name in ('3dmatch', 'modelnet'):
        cfg = load_cfg(name)
        last = cfg.num_encoder_layers - 1
        base = RegTR(cfg)
        keys0, wd0, layers0 = base.loss_keys(), loss_weight_dict(cfg), base.head_layers()
        assert not any(k.startswith('pose') for k in keys0) and not any(k.startswith('pose') for k in wd0)
        cfg.wt_pose = 0
        zero = RegTR(cfg)
        assert zero.loss_keys() == keys0 and loss_weight_dict(cfg) == wd0 and zero.head_layers() == layers0
        cfg.wt_pose = 0.5
        on = RegTR(cfg)
        assert on.loss_keys() == keys0[:-1] + [f'pose_{last}', 'total']
        wd = loss_weight_dict(cfg)
        assert wd.pop(f'pose_{last}') == 0.5 and wd == wd0
        assert on.head_layers() == sorted(set(layers0) | {last})
        # the last layer enters head_layers() through the pose term alone
        cfg.overlap_loss_on, cfg.corr_loss_on = [0], [0]
        assert RegTR(cfg).head_layers() == [0, last]
        cfg.wt_pose = 0
        assert RegTR(cfg).head_layers() == [0]


def test_pose_tensor_reads_like_the_gradient_free_pose_it_replaces():
    from regtr_amd.head_grad import PoseTensor
    x = torch.arange(24, dtype=torch.float32).reshape(1, 2, 3, 4).requires_grad_()
    p = (x * 2).as_subclass(PoseTensor)
    assert p.grad_fn is not None and torch.equal(p.detach(), x.detach() * 2)
    assert np.array_equal(p[0].cpu().numpy(), 2 * x.detach().numpy()[0]) and np.array_equal(np.asarray(p), 2 * x.detach().numpy())
    (p * p).sum().backward()
    assert torch.equal(x.grad, 8 * x.detach())


def test_cpu_tensors_are_refused():
    from regtr_amd import head_grad, losses, ops, se3
    kp, corr, logit = torch.zeros(4, 3), torch.zeros(1, 4, 3, requires_grad=True), torch.zeros(1, 4)
    seg = torch.tensor([0, 4, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        head_grad.procrustes_forward_grad(kp, corr, logit, seg, 1)
    with pytest.raises(RuntimeError):
        ops.weighted_procrustes_bwd(kp, corr.detach(), logit, seg, 1, torch.zeros(1, 1, 3, 4))
    with pytest.raises(RuntimeError):
        se3.compute_rigid_transform(torch.rand(5, 3, requires_grad=True), torch.rand(5, 3))
    with pytest.raises(RuntimeError):
        losses.PoseCriterion()(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
