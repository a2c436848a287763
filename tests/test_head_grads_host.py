"""CPU: the float64 restatement tests/head_grads_ref.py against the stored results of the real reference modules
(tests/golden/head_grads_<case>.npz) and against torch's float64 autograd of the same arithmetic; its kernel bounds; and the new
entry points' presence in the header, the binding table and the build list."""
import os
import re

import numpy as np
import pytest
import torch

from tests import head_grads_ref as HR
from tests.util import ROOT

REL = 1e-9
_cache = {}


def _full(name):
    if name not in _cache:
        _cache[name] = (HR.draw_full_case(name), HR.full(HR.draw_full_case(name)))
    return _cache[name]


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize('name', list(HR.FULL_CASES))
def test_restatement_agrees_with_the_reference_modules(name):
    c, r = _full(name)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', f'head_grads_{name}.npz'))
    assert int(g['decision_rows']) == 0, 'the float32 anchors decide differently in float64 distances'
    assert float(g['relu_margin']) >= HR.RELU_MARGIN and abs(HR.relu_margin(c) - float(g['relu_margin'])) <= 1e-6 * float(g['relu_margin'])
    assert int(g['seed']) == c['seed'] and list(g['src_lens']) == c['src'] and list(g['tgt_lens']) == c['tgt']
    st, rows = int(g['row_step']), g['w_rows']
    for k in ('overlap', 'feature', 'feature_un', 'corr', 'total'):
        assert abs(float(r['losses'][k]) - float(g['loss/' + k])) <= REL * abs(float(g['loss/' + k])), k
    assert _rel(r['corr'][::st], g['corr']) <= REL and _rel(r['logit'][::st], g['logit']) <= REL
    assert _rel(r['d_feats_un'][::st], g['d_feats_un']) <= REL
    names = [k[2:] for k in g.files if k.startswith('g/')]
    assert set(names) == set(r['grads']), 'a gradient tensor of the reference is missing from the restatement (or the reverse)'
    for k in names:
        got = r['grads'][k]
        got = got if got.dim() == 1 or got.shape[0] <= 3 else got[rows]
        assert _rel(got, g['g/' + k]) <= REL, (k, _rel(got, g['g/' + k]))
    # the modules' state_dict names are RegTR's
    from regtr_amd import RegTR
    from tests.util import load_cfg
    sd = RegTR(load_cfg('3dmatch')).state_dict()
    assert all(k in sd for k in g['sd_keys'] if not k.startswith('transformer_encoder.layers.') or int(k.split('.')[2]) < 6)


def test_head_backward_agrees_with_autograd():
    c = HR.draw_head_case('ragged')
    r = HR.run_head_case(c)
    P = {k: v.double().requires_grad_() for k, v in c['sd'].items()}
    f = c['feats'].double().reshape(-1, c['D']).requires_grad_()
    corr, logit, _ = HR.head_fwd(P, f)
    ((corr * c['d_corr'].double().reshape(-1, 3)).sum() + (logit * c['d_logit'].double().reshape(-1)).sum()).backward()
    assert _rel(r['df'].reshape(-1, c['D']), f.grad) <= 1e-12
    for k, p in P.items():
        assert _rel(r['grads'][k], p.grad) <= 1e-12, k


def test_bce_agrees_with_torch():
    gen = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(50, generator=gen, dtype=torch.float64) * 4, torch.tensor([100.0, -100.0, 0.0], dtype=torch.float64)])
    y = torch.rand(53, generator=gen, dtype=torch.float64)
    y[:2], y[-1] = torch.tensor([0.0, 1.0]), 1.0
    xa = x.clone().requires_grad_()
    want = torch.nn.BCEWithLogitsLoss()(xa, y)
    want.backward()
    val, grad = HR.bce(x, y)
    assert abs(float(val) - float(want.detach())) <= 1e-14 * abs(float(want.detach())) and _rel(grad, xa.grad) <= 1e-13
    k = HR.bce_logits_bwd(x.numpy(), y.numpy(), 0.7)
    assert _rel(k['d'], 0.7 * xa.grad.numpy()) <= 1e-13 and np.all(k['b_d'] > 0)


def test_full_backward_agrees_with_autograd():
    """The manual backward of the whole chain against torch's float64 autograd of the same forward (the small case)."""
    name = '3dmatch_crop_b2'
    c, r = _full(name)
    leaves = {}

    def leaf(key, v):
        leaves[key] = torch.as_tensor(v).double().clone().requires_grad_()
        return leaves[key]
    Wp, bp = leaf('feat_proj.weight', c['sd_proj']['weight']), leaf('feat_proj.bias', c['sd_proj']['bias'])
    Ph = {k: leaf('correspondence_decoder.' + k, v) for k, v in c['sd_head'].items()}
    W, Wu = leaf('feature_criterion.W', c['W']), leaf('feature_criterion_un.W', c['W_un'])
    fu = leaf('feats_un', c['feats_un'])
    sd_enc = {k: leaf('transformer_encoder.' + k, v) for k, v in c['sd_enc'].items()}
    B, L, seg, wt = c['B'], c['L'], c['seg'], c['wt']
    cut = lambda x, lo: [x[int(seg[lo + b]):int(seg[lo + b + 1])] for b in range(B)]
    x = fu @ Wp.T + bp
    y = x
    for li in range(L):
        y, _ = HR.R.layer_fwd(HR.R._sub(sd_enc, f'layers.{li}.'), y, None, seg, c['kv_self'], c['kv_cross'], c['H'])
    last, _ = HR.R.ln_fwd(y, sd_enc['norm.weight'], sd_enc['norm.bias'])
    corr, logit, _ = HR.head_fwd(Ph, last)
    dec = HR.decisions(c)
    gt, T = c['gt'].double(), torch.from_numpy(c['pose']).double()
    kp = lambda ks: [torch.from_numpy(k).double() for k in ks]
    total = (wt['overlap'] * HR.bce(logit, gt)[0] + wt['feature'] * HR.infonce(cut(last, 0), cut(last, B), W, dec)[0]
             + wt['feature_un'] * HR.infonce(cut(x, 0), cut(x, B), Wu, dec)[0]
             + wt['corr'] * (HR.corr_l1(kp(c['src_kp']), cut(corr, 0), T, cut(gt, 0))[0]
                             + HR.corr_l1(kp(c['tgt_kp']), cut(corr, B), HR.se3_inv(T), cut(gt, B))[0]))
    assert c['pe'] is None and abs(float(total) - float(r['losses']['total'])) <= 1e-12 * abs(float(total))
    total.backward()
    assert _rel(r['d_feats_un'], fu.grad) <= 1e-10
    for k, g in r['grads'].items():
        # the final norm serves the last layer only here (the other layers' outputs carry no loss): autograd sees the same
        assert leaves[k].grad is not None and _rel(g, leaves[k].grad) <= 1e-10, (k, _rel(g, leaves[k].grad))


@pytest.mark.parametrize('sides', ['both', 'corr', 'logit'])
def test_kernel_bounds_are_positive_where_the_reference_is_nonzero(sides):
    rng = np.random.default_rng(9)
    for m, D in ((5, 64), (257, 256)):
        h2 = np.maximum(rng.normal(0, 1, (m, D)), 0).astype(np.float32)
        f, w4, wc = (rng.normal(0, 1, s).astype(np.float32) for s in ((m, D), (3, D), (D,)))
        dc = rng.normal(0, 1, (m, 3)).astype(np.float32) if sides != 'logit' else None
        dl = rng.normal(0, 1, m).astype(np.float32) if sides != 'corr' else None
        r = HR.head_tail_bwd(dc, dl, h2, f, w4, wc)
        for k in ('g2', 'r', 'dw4', 'db4', 'dwc', 'dbc', 'db2'):
            assert r[k].shape == r['b_' + k].shape and np.all(r['b_' + k][r[k] != 0] > 0), k
            if (dc is None and k in ('g2', 'dw4', 'db4', 'db2')) or (dl is None and k in ('r', 'dwc', 'dbc')):
                assert not r[k].any() and not r['b_' + k].any(), k
        assert np.all(r['g2'][h2 <= 0] == 0)
        # the bounds are first order in U: far below the flat bar
        for k in ('dw4', 'dwc', 'db2'):
            if r[k].any():
                assert r['b_' + k].max() <= 1e-4 * np.abs(r[k]).max(), k


def test_entry_points_exported_declared_and_bound():
    import ctypes
    from regtr_amd import _lib as L
    from regtr_amd import build, head_grad, losses, ops
    from regtr_amd.regtr import CorrespondenceDecoder, CorrespondenceRegressor, RegTR
    lib = ctypes.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    table = hdr.split('#ifndef REGTR_HIP_H')[0]
    for name in ('regtr_head_tail_bwd', 'regtr_head_tail_bwd_ws_bytes', 'regtr_bce_logits_bwd'):
        assert hasattr(lib, name) and name in L.SIGNATURES and f'{name}(' in hdr, name
        if not name.endswith('_ws_bytes'):
            assert name + ' ' in table, name                   # the mapping table at the top
    assert int(re.search(r'#define REGTR_ABI_VERSION (\d+)', hdr).group(1)) == L.ABI_VERSION
    assert 'head_bwd.hip' in build.SOURCES
    assert callable(ops.head_tail_bwd) and callable(ops.bce_logits_bwd) and callable(head_grad.stack_forward_grad)
    assert callable(CorrespondenceRegressor.forward_grad) and callable(CorrespondenceDecoder.forward_grad)
    assert callable(losses.OverlapCriterion) and all(callable(getattr(RegTR, n)) for n in
                                                     ('forward_grad', 'compute_loss_grad', 'trainable_parameters', 'training_step'))
    # refusals that need no GPU: nothing is launched for a refused argument list
    lib.regtr_head_tail_bwd_ws_bytes.restype = ctypes.c_size_t
    assert lib.regtr_head_tail_bwd_ws_bytes(100, 64) == 4 * (5 * 64 + 4) * 4 and lib.regtr_head_tail_bwd_ws_bytes(100, 96) == 0
    assert lib.regtr_head_tail_bwd_ws_bytes(0, 64) == 0 and lib.regtr_head_tail_bwd_ws_bytes(5000, 256) == 157 * (5 * 256 + 4) * 4
