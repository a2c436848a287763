"""CPU: the cross-encoder backward's two entry points (regtr_layernorm_bwd, regtr_bias_relu_bwd and their *_ws_bytes queries) --
exported, declared, in the header's mapping table, and every refusal decided on the host with nothing launched; the float64 yardstick
tests/cross_encoder_grads_ref.py pinned to the goldens of the REAL reference TransformerCrossEncoder
(tools/make_golden_cross_encoder_grads.py) and to torch's LayerNorm autograd; forward_grad's refusals."""
import os

import numpy as np
import pytest
import torch

from tests import cross_encoder_grads_ref as R
from tests.util import ROOT

FAKE = 0x10000          # never dereferenced: every call below is refused (or has nothing to do) before a launch
NAMES = ('regtr_layernorm_bwd', 'regtr_layernorm_bwd_ws_bytes', 'regtr_bias_relu_bwd', 'regtr_bias_relu_bwd_ws_bytes')


def _lib():
    from regtr_amd import _lib as L
    return L.lib()


def _ln(n=64, D=256, ws_bytes=1 << 24, **kw):
    p = {k: kw.get(k, FAKE) for k in ('x', 'gamma', 'dy', 'dres', 'dx', 'dgamma', 'dbeta', 'ws')}
    return _lib().regtr_layernorm_bwd(p['x'], n, D, p['gamma'], 1e-5, p['dy'], p['dres'], p['dx'], p['dgamma'], p['dbeta'], p['ws'], ws_bytes,
                                      None)


def _br(n=64, N=256, ws_bytes=1 << 24, **kw):
    p = {k: kw.get(k, FAKE) for k in ('g', 'h', 'dh', 'db', 'ws')}
    ld = {k: kw.get(k, N) for k in ('ldg', 'ldh', 'ld_dh')}
    return _lib().regtr_bias_relu_bwd(p['g'], ld['ldg'], p['h'], ld['ldh'], p['dh'], ld['ld_dh'], p['db'], n, N, p['ws'], ws_bytes, None)


def test_entry_points_exported_declared_and_mapped():
    from regtr_amd import _lib as L
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES and f'{name}(' in hdr
    table = hdr.split('#ifndef REGTR_HIP_H')[0]                  # the mapping table at the top
    assert 'regtr_layernorm_bwd ' in table and 'regtr_bias_relu_bwd ' in table and 'transformers.py:194-238' in table
    from regtr_amd import build, ops
    assert 'layer_bwd.hip' in build.SOURCES and callable(ops.layernorm_bwd) and callable(ops.bias_relu_bwd)


@pytest.mark.parametrize('name', ['x', 'gamma', 'dy', 'dx', 'dgamma', 'dbeta', 'ws'])
def test_layernorm_bwd_refuses_null_with_work(name):
    assert _ln(**{name: None}) == -2
    assert _ln(dres=None, ws_bytes=0) == -3                      # dres is optional: gets as far as the workspace check


@pytest.mark.parametrize('kw', [{'n': -1}, {'D': 0}, {'D': -4}, {'D': 2}, {'D': 254}, {'D': 258}, {'D': 1028}])
def test_layernorm_bwd_refuses_bad_shapes(kw):
    assert _ln(**kw) == -2


@pytest.mark.parametrize('name', ['x', 'gamma', 'dy', 'dres', 'dx', 'ws'])
def test_layernorm_bwd_refuses_misaligned(name):
    assert _ln(**{name: FAKE + 4}) == -2 and _ln(**{name: FAKE + 8}) == -2


def test_layernorm_bwd_workspace_and_nothing_to_do():
    L = _lib()
    need = L.regtr_layernorm_bwd_ws_bytes(64, 256)
    assert need >= 2 * 256 * 4 * (64 // R.chunk_rows(64))        # a (dgamma, dbeta) row per chunk
    assert _ln(ws_bytes=need - 1) == -3 and _ln(ws_bytes=0) == -3
    assert L.regtr_layernorm_bwd_ws_bytes(100000, 256) > L.regtr_layernorm_bwd_ws_bytes(1000, 256) > 0
    assert L.regtr_layernorm_bwd_ws_bytes(0, 256) == 0 and L.regtr_layernorm_bwd_ws_bytes(-1, 256) == 0 and L.regtr_layernorm_bwd_ws_bytes(64, 6) == 0
    for n in (1, 3, 4, 5, 257, 4099, 100000):                   # the chunking is the restatement's: one partial row per chunk
        assert L.regtr_layernorm_bwd_ws_bytes(n, 64) == -(-n // R.chunk_rows(n)) * 2 * 64 * 4
        assert L.regtr_bias_relu_bwd_ws_bytes(n, 768) == -(-n // R.chunk_rows(n)) * 768 * 4
    assert _ln(n=0) == 0
    assert _ln(n=0, D=258) == -2                                 # ... but the shape checks still hold
    assert _ln(n=0, x=None, gamma=None, dy=None, dres=None, dx=None, dgamma=None, dbeta=None, ws=None, ws_bytes=0) == 0


@pytest.mark.parametrize('name', ['g', 'db', 'ws'])
def test_bias_relu_bwd_refuses_null_with_work(name):
    assert _br(**{name: None}) == -2
    assert _br(h=None, dh=None, ws_bytes=0) == -3                # h and dh are optional
    assert _br(h=None) == -2                                     # ... but dh needs h


@pytest.mark.parametrize('kw', [{'n': -1}, {'N': 0}, {'N': -64}, {'N': 2}, {'N': 66}])
def test_bias_relu_bwd_refuses_bad_shapes(kw):
    assert _br(**kw) == -2


@pytest.mark.parametrize('name', ['ldg', 'ldh', 'ld_dh'])
def test_bias_relu_bwd_refuses_bad_strides(name):
    assert _br(**{name: 256 + 2}) == -2                          # not a multiple of 4
    assert _br(**{name: 256 - 4}) == -2                          # below N
    assert _br(**{name: 0}) == -2 and _br(**{name: -256}) == -2
    assert _br(ws_bytes=0, **{name: 1024}) == -3                 # legal: gets as far as the workspace check (too small: nothing launched)
    if name != 'ldg':                                            # a stride that is not read (its tensor is absent) is not judged
        assert _br(h=None, dh=None, ws_bytes=0, **{name: 3}) == -3


@pytest.mark.parametrize('name', ['g', 'h', 'dh', 'ws'])
def test_bias_relu_bwd_refuses_misaligned(name):
    assert _br(**{name: FAKE + 4}) == -2 and _br(**{name: FAKE + 8}) == -2


def test_bias_relu_bwd_workspace_and_nothing_to_do():
    L = _lib()
    need = L.regtr_bias_relu_bwd_ws_bytes(64, 256)
    assert need >= 256 * 4
    assert _br(ws_bytes=need - 1) == -3 and _br(ws_bytes=0) == -3
    assert L.regtr_bias_relu_bwd_ws_bytes(0, 256) == 0 and L.regtr_bias_relu_bwd_ws_bytes(-1, 256) == 0 and L.regtr_bias_relu_bwd_ws_bytes(64, 6) == 0
    assert _br(n=0) == 0
    assert _br(n=0, g=None, h=None, dh=None, db=None, ws=None, ws_bytes=0) == 0
    assert _br(n=0, N=66) == -2                                  # ... but the shape checks still hold


# ------------------------------------------------------------------------------------------------ the yardstick
def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


@pytest.mark.parametrize('name', list(R.CASES))
def test_yardstick_equals_the_real_reference_module(name):
    """Validates the yardstick, not the product: the float64 restatement against the stored results of the reference's own
    TransformerCrossEncoder on padded clouds (both float64)."""
    c = R.draw_case(name)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', f'cross_encoder_grads_{name}.npz'))
    assert int(g['seed']) == c['seed'] and list(g['src_lens']) == c['src'] and list(g['tgt_lens']) == c['tgt']
    assert (int(g['D']), int(g['H']), int(g['F']), int(g['L'])) == (c['D'], c['H'], c['F'], c['L'])
    assert list(g['sd_keys']) == list(c['sd'])
    assert [tuple(s[:v.dim()]) for s, v in zip(g['sd_shapes'], c['sd'].values())] == [tuple(v.shape) for v in c['sd'].values()]
    r = R.run_case(c)
    st = int(g['row_step'])
    assert tuple(r['out'].shape) == (c['L'] if c['final'] else 1, len(c['x']), c['D'])
    assert _rel(r['out'][:, ::st], g['out']) <= 1e-10 and _rel(r['dx'][::st], g['dx']) <= 1e-10
    if c['pe'] is not None:
        assert _rel(r['dpe'][::st], g['dpe']) <= 1e-10
    keys = [k for k in g.files if k.startswith('g/')]
    assert sorted(k[2:] for k in keys) == sorted(c['sd'])
    for k in keys:
        a = r['grads'][k[2:]].numpy()
        assert _rel(a[g['w_rows']] if a.ndim == 2 else a, g[k]) <= 1e-10, k


def test_project_encoder_has_the_reference_state_dict():
    from regtr_amd.transformer import TransformerCrossEncoder, TransformerCrossEncoderLayer
    c = R.draw_case('ragged')
    layer = TransformerCrossEncoderLayer(c['D'], c['H'], c['F'], 0.0, 'relu', True, True, True)
    enc = TransformerCrossEncoder(layer, c['L'], None, False)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'cross_encoder_grads_ragged.npz'))
    assert list(enc.state_dict()) == list(g['sd_keys'])
    enc.load_state_dict(c['sd'], strict=True)
    assert all(p.requires_grad for p in enc.parameters())


@pytest.mark.parametrize('offset', [0.0, 100.0])
@pytest.mark.parametrize('with_dres', [False, True])
def test_layernorm_restatement_equals_torch_autograd(offset, with_dres):
    rng = np.random.default_rng(5)
    n, D = 37, 64
    x, gamma, dy, dres = rng.normal(offset, 1, (n, D)), rng.normal(1, 0.1, D), rng.normal(0, 1, (n, D)), rng.normal(0, 1, (n, D))
    r = R.layernorm_bwd(x, gamma, dy, dres if with_dres else None)
    xt, gt, bt = (torch.tensor(a, requires_grad=True) for a in (x, gamma, np.zeros(D)))
    y = torch.nn.functional.layer_norm(xt, (D,), gt, bt, 1e-5)
    (y * torch.tensor(dy)).sum().backward()
    want = xt.grad.numpy() + (dres if with_dres else 0)
    assert _rel(r['dx'], want) <= 1e-10 and _rel(r['dgamma'], gt.grad.numpy()) <= 1e-10 and _rel(r['dbeta'], bt.grad.numpy()) <= 1e-10
    # ... and the torch form the stack uses
    dx, dg, db = R.ln_bwd(R.ln_fwd(torch.tensor(x), torch.tensor(gamma), torch.zeros(D, dtype=torch.float64))[1], torch.tensor(gamma), torch.tensor(dy))
    assert _rel(dx.numpy(), xt.grad.numpy()) <= 1e-10 and _rel(dg.numpy(), gt.grad.numpy()) <= 1e-10 and _rel(db.numpy(), bt.grad.numpy()) <= 1e-10
    for b in ('b_dx', 'b_dgamma', 'b_dbeta'):
        assert np.all(r[b] > 0) and np.all(np.isfinite(r[b]))


def test_bounds_cover_a_float32_numpy_evaluation():
    """A plain float32 numpy evaluation of the same formulas stays inside the kernels' bounds."""
    rng = np.random.default_rng(6)
    f = np.float32
    for offset in (0.0, 100.0):
        n, D = 257, 256
        x, gamma, dy = rng.normal(offset, 1, (n, D)).astype(f), rng.normal(1, 0.1, D).astype(f), rng.normal(0, 1, (n, D)).astype(f)
        r = R.layernorm_bwd(x, gamma, dy)
        mean = x.mean(1, keepdims=True, dtype=f)
        xc = x - mean
        rstd = f(1) / np.sqrt((xc * xc).mean(1, keepdims=True, dtype=f) + f(1e-5))
        xh, g = xc * rstd, dy * gamma
        dx = rstd * (g - g.mean(1, keepdims=True, dtype=f) - xh * (g * xh).mean(1, keepdims=True, dtype=f))
        assert (np.abs(dx - r['dx']) / r['b_dx']).max() <= 1.0
        assert (np.abs((dy * xh).sum(0, dtype=f) - r['dgamma']) / r['b_dgamma']).max() <= 1.0
        assert (np.abs(dy.sum(0, dtype=f) - r['dbeta']) / r['b_dbeta']).max() <= 1.0
    g, h = rng.normal(0, 1, (257, 768)).astype(f), np.maximum(rng.normal(0, 1, (257, 768)), 0).astype(f)
    for hh in (None, h):
        r = R.bias_relu_bwd(g, hh)
        dh = g if hh is None else np.where(hh > 0, g, f(0))
        assert np.array_equal(dh, r['dh'].astype(f)) and (np.abs(dh.sum(0, dtype=f) - r['db']) / r['b_db']).max() <= 1.0


# ------------------------------------------------------------------------------------------------ forward_grad's refusals
def _enc(**kw):
    from regtr_amd.transformer import TransformerCrossEncoder, TransformerCrossEncoderLayer
    a = dict(d_model=64, nhead=2, dim_feedforward=128, dropout=0.0, activation='relu', normalize_before=True, sa_val_has_pos_emb=True,
             ca_val_has_pos_emb=True)
    a.update(kw)
    layer = TransformerCrossEncoderLayer(**a)
    return TransformerCrossEncoder(layer, 2, None, False), layer


def _cpu_args(with_pe=True):
    x = torch.zeros(8, 64, requires_grad=True)
    return (x, torch.zeros(8, 64) if with_pe else None, torch.tensor([0, 4, 8], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
            torch.tensor([1, 0], dtype=torch.int32), 4)


def test_forward_grad_refuses_cpu_tensors():
    enc, layer = _enc()
    with pytest.raises(RuntimeError, match='GPU tensor'):
        enc.forward_grad(*_cpu_args())
    with pytest.raises(RuntimeError, match='GPU tensor'):
        layer.forward_grad(*_cpu_args(False))


@pytest.mark.parametrize('kw,word', [({'normalize_before': False}, 'normalize_before'), ({'sa_val_has_pos_emb': False}, 'sa_val_has_pos_emb'),
                                     ({'ca_val_has_pos_emb': False}, 'ca_val_has_pos_emb'), ({'dim_feedforward': 96}, 'dim_feedforward')])
def test_forward_grad_names_the_unsupported_option(kw, word):
    enc, layer = _enc(**kw)
    for m in (enc, layer):
        with pytest.raises(NotImplementedError, match=word):
            m.forward_grad(*_cpu_args())


def test_forward_grad_refuses_dropout():
    enc, layer = _enc()
    layer.self_attn.dropout = 0.1                               # the constructor already refuses it; a module edited afterwards
    with pytest.raises(NotImplementedError, match='dropout'):
        layer.forward_grad(*_cpu_args())
    from regtr_amd.transformer import TransformerCrossEncoderLayer
    with pytest.raises(NotImplementedError, match='dropout'):
        TransformerCrossEncoderLayer(64, 2, 128, dropout=0.1)
