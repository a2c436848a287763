"""CPU: the InstanceNorm / max-pool backward entry points (regtr_instnorm_bwd, regtr_maxpool_argmax, regtr_maxpool_gather_bwd) -- exported,
declared, bound, and every refusal decided on the host with nothing launched; the float64 yardstick tests/norm_pool_grads_ref.py pinned
to the reference code's goldens (tools/make_golden_norm_pool_grads.py) and to float64 torch autograd; the float32 ordered restatement of
the pool backward against the float64 one."""
import os

import numpy as np
import pytest
import torch

from tests import norm_pool_grads_ref as R
from tests.util import ROOT

FAKE = 0x10000          # never dereferenced: every call below is refused (or has nothing to do) before a launch
ENTRIES = ('regtr_instnorm_bwd', 'regtr_instnorm_bwd_ws_bytes', 'regtr_maxpool_argmax', 'regtr_maxpool_gather_bwd')


def _lib():
    from regtr_amd import _lib as L
    return L.lib()


def _in(n_clouds=4, max_len=65, C=64, act=1, ws_bytes=1 << 24, **kw):
    p = {n: kw.get(n, d) for n, d in (('x', FAKE), ('seg_off', FAKE), ('stats', FAKE), ('residual', None), ('res_stats', None), ('dy', FAKE),
                                      ('dx', FAKE), ('dres', None), ('ws', FAKE))}
    return _lib().regtr_instnorm_bwd(p['x'], p['seg_off'], n_clouds, max_len, C, p['stats'], p['residual'], p['res_stats'], act, 0.1, p['dy'],
                                     p['dx'], p['dres'], p['ws'], ws_bytes, None)


def _am(ns=100, C=64, ld=7, nq=50, H=7, **kw):
    p = {n: kw.get(n, FAKE) for n in ('x', 'nbr', 'arg')}
    return _lib().regtr_maxpool_argmax(p['x'], ns, C, p['nbr'], ld, nq, H, p['arg'], None)


def _pb(nq=50, H=7, C=64, ns=100, **kw):
    p = {n: kw.get(n, FAKE) for n in ('dy', 'arg', 'row_off', 'entries', 'dx')}
    return _lib().regtr_maxpool_gather_bwd(p['dy'], p['arg'], nq, H, C, p['row_off'], p['entries'], ns, p['dx'], None)


def test_entry_points_exported_declared_and_bound():
    from regtr_amd import _lib as L
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    table = hdr.split('#ifndef REGTR_HIP_H')[0]
    for name in ENTRIES:
        assert hasattr(lib, name) and name in L.SIGNATURES and f'{name}(' in hdr, name
        if not name.endswith('_ws_bytes'):
            assert name + ' ' in table, name                   # the mapping table at the top
    assert '#define REGTR_ABI_VERSION 11' in hdr and L.ABI_VERSION == 11 and lib.regtr_abi_version() == 11
    from regtr_amd import backbone_grad, build, ops
    assert 'norm_pool_bwd.hip' in build.SOURCES
    assert callable(ops.instnorm_bwd) and callable(ops.maxpool_argmax) and callable(ops.maxpool_bwd)
    assert callable(backbone_grad.instance_norm) and callable(backbone_grad.max_pool)


# ---- regtr_instnorm_bwd
@pytest.mark.parametrize('kw', [{'n_clouds': 0}, {'max_len': -1}, {'C': 0}, {'C': 2}, {'C': 6}, {'C': 48}, {'C': 1028}, {'C': 2048}, {'act': 2},
                                {'act': -1}, {'x': None}, {'seg_off': None}, {'stats': None}, {'dy': None}, {'dx': None}, {'ws': None},
                                {'dres': FAKE}, {'res_stats': FAKE}, {'x': FAKE + 4}, {'dy': FAKE + 8}, {'dx': FAKE + 4}, {'stats': FAKE + 8},
                                {'residual': FAKE + 4, 'dres': FAKE}, {'residual': FAKE, 'dres': FAKE + 8}])
def test_instnorm_bwd_refusals(kw):
    assert _in(**kw) == -2


def test_instnorm_bwd_accepts_the_forwards_widths_and_nothing_to_do():
    L = _lib()
    for C in (4, 8, 16, 32, 64, 128, 256, 512, 1024):
        assert _in(C=C, max_len=0) == 0
        assert L.regtr_instnorm_bwd_ws_bytes(4, 65, C) > 0
    assert _in(max_len=0, residual=FAKE, res_stats=FAKE, dres=FAKE, dx=None) == 0
    assert _in(max_len=0, residual=FAKE, dres=FAKE, dx=None, ws=None, ws_bytes=0) == 0     # a plain shortcut's gradient alone needs no sums
    assert _in(max_len=0, C=48) == -2                          # ... but the shape checks still hold
    for bad in ((0, 65, 64), (4, -1, 64), (4, 65, 48), (4, 65, 2048)):
        assert L.regtr_instnorm_bwd_ws_bytes(*bad) == 0


@pytest.mark.parametrize('C', [4, 32, 64, 256, 1024])
def test_instnorm_bwd_workspace_follows_the_chunking(C):
    """Three float64 sums per (cloud, chunk, channel) and one float4 of means per (cloud, channel), with the chunk length of
    tests/dispatch.in_rows -- the length the GPU cases' R + 1 clouds are built around."""
    L = _lib()
    for n_clouds, max_len in ((4, R.edge_lens(C)[-1]), (2, 8323), (64, 40000)):
        rows = R.in_rows(n_clouds, max_len, C)
        nchunk = -(-max_len // rows)
        need = L.regtr_instnorm_bwd_ws_bytes(n_clouds, max_len, C)
        up = lambda b: -(-b // 256) * 256
        assert need == up(nchunk * n_clouds * C * 24) + up(n_clouds * C * 16)
        assert _in(n_clouds=n_clouds, max_len=max_len, C=C, ws_bytes=need - 1) == -3


# ---- regtr_maxpool_argmax / regtr_maxpool_gather_bwd
@pytest.mark.parametrize('kw', [{'ns': -1}, {'nq': -1}, {'H': 0}, {'H': 32768, 'ld': 40000}, {'ld': 6}, {'C': 0}, {'C': 2}, {'C': 66}, {'x': None},
                                {'nbr': None}, {'arg': None}, {'x': FAKE + 4}, {'arg': FAKE + 2}, {'arg': FAKE + 4}])
def test_maxpool_argmax_refusals(kw):
    assert _am(**kw) == -2


def test_maxpool_argmax_nothing_to_do():
    assert _am(nq=0) == 0 and _am(nq=0, x=None, nbr=None, arg=None) == 0
    assert _am(nq=0, C=66) == -2


@pytest.mark.parametrize('kw', [{'ns': -1}, {'nq': -1}, {'H': 0}, {'H': 32768}, {'C': 0}, {'C': 2}, {'C': 66}, {'nq': 1 << 26, 'H': 40}, {'dy': None},
                                {'arg': None}, {'row_off': None}, {'entries': None}, {'dx': None}, {'dy': FAKE + 4}, {'dx': FAKE + 8},
                                {'arg': FAKE + 4}])
def test_maxpool_gather_bwd_refusals(kw):
    assert _pb(**kw) == -2


def test_maxpool_gather_bwd_nothing_to_do():
    assert _pb(ns=0) == 0 and _pb(ns=0, nq=0, dy=None, arg=None, row_off=None, entries=None, dx=None) == 0
    assert _pb(ns=0, C=66) == -2


# ---- the yardstick
@pytest.mark.parametrize('lrelu,shortcut', R.VARIANTS)
@pytest.mark.parametrize('name', ['in_c64', 'in_g32'])
def test_instnorm_yardstick_equals_float64_autograd(name, lrelu, shortcut):
    c = R.draw_case(name)
    res = None if shortcut == 'none' else c['res']
    r = R.instnorm_run(c['x'], c['lens'], c['dy'], res, shortcut == 'normed', lrelu, bounds=True)
    t = lambda a: torch.from_numpy(a).double()
    xt = t(c['x']).requires_grad_()
    rt = None if res is None else t(res).requires_grad_()
    out = R.torch_instance_norm(xt, c['lens'], rt, shortcut == 'normed', lrelu, slope=R.SLOPE, eps=R.EPS)
    (out * t(c['dy'])).sum().backward()
    pairs = [(r['out'], out.detach().numpy()), (r['dx'], xt.grad.numpy())] + ([] if res is None else [(r['dres'], rt.grad.numpy())])
    for got, ref in pairs:
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.all(r['b_dx'] > 0) and np.all(r['b_dx'] <= 1e-4 * np.abs(r['dx']).max())
    if 1 in c['lens']:
        one = int(c['seg_off'][c['lens'].index(1)])
        assert np.all(r['dx'][one] == 0)                       # a one-row cloud: xh = 0 and g - mean(g) = 0


def test_instnorm_yardstick_takes_the_mask_as_given():
    c = R.draw_case('in_g64')
    r = R.instnorm_run(c['x'], c['lens'], c['dy'], lrelu=True)
    flipped = r['z'] > 0
    flipped[5, 7] = ~flipped[5, 7]
    r2 = R.instnorm_run(c['x'], c['lens'], c['dy'], lrelu=True, mask=flipped)
    assert np.array_equal(r2['dx'][:, :7], r['dx'][:, :7]) and not np.allclose(r2['dx'][:37, 7], r['dx'][:37, 7], rtol=1e-6, atol=0)
    assert np.array_equal(R.instnorm_run(c['x'], c['lens'], c['dy'], lrelu=True, mask=r['z'] > 0)['dx'], r['dx'])


@pytest.mark.parametrize('name', R.POOL_CASES)
def test_pool_yardstick_equals_float64_autograd_and_its_float32_restatement(name):
    c = R.draw_case(name)
    ns, width = c['Ns'], c['width']
    r = R.pool_run(c['x'], c['nbr'], width, c['dy'])
    idx = c['nbr'][:, :width].astype(np.int64)
    idx = np.where((idx >= 0) & (idx < ns), idx, ns)
    xt = torch.from_numpy(c['x']).double().requires_grad_()
    out = R.torch_max_pool(xt, torch.from_numpy(idx))
    (out * torch.from_numpy(c['dy']).double()).sum().backward()
    assert np.array_equal(r['out'], out.detach().numpy()) and np.array_equal(r['dx'], xt.grad.numpy())      # the lowest-column rule is torch's
    d32 = R.pool_bwd_f32(c['dy'], r['arg'], c['nbr'], width, ns)
    deg = np.bincount(idx.reshape(-1), minlength=ns + 1)[:ns]
    a = np.zeros((ns + 1, c['C']))
    np.add.at(a, idx.reshape(-1), np.abs(np.repeat(c['dy'].astype(np.float64), width, axis=0)))
    assert d32.dtype == np.float32 and np.all(np.abs(d32 - r['dx']) <= deg[:, None] * R.U * a[:ns])
    assert r['arg'].dtype == np.int16 and r['arg'].min() >= -1 and r['arg'].max() < width
    if c.get('orphan'):
        assert deg[R.ORPHAN] == 0 and np.all(r['dx'][R.ORPHAN] == 0)
    if c.get('hub'):
        assert deg[R.HUB] == c['Nq'] > 64
    if c.get('full'):
        assert (r['out'] < 0).all() and (r['arg'] >= 0).all()
    if c.get('ties'):
        vals = np.concatenate([c['x'], np.zeros((1, c['C']), np.float32)])[idx]
        assert ((vals == r['out'][:, None, :]).sum(1) > 1).mean() > 0.3 and (r['arg'] == -1).any()      # most maxima are shared, some with the shadow


@pytest.mark.parametrize('name', R.GOLDEN_CASES)
def test_yardstick_equals_reference_code(name):
    """The float64 restatements against the REAL reference max_pool / BatchNormBlock + LeakyReLU forward and gradients (goldens): 1e-10
    relative (no element is left out here: float64 against float64 agree on every LeakyReLU side)."""
    c = R.draw_case(name)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', f'norm_pool_grads_{name}.npz'))
    assert int(g['seed']) == c['seed'] and int(g['C']) == c['C']
    step = int(g['step'])
    if c['kind'] == 'in':
        lrelu, shortcut = c['golden']
        assert list(g['lens']) == c['lens'] and (bool(g['lrelu']), str(g['shortcut'])) == (lrelu, shortcut)
        r = R.instnorm_run(c['x'], c['lens'], c['dy'], None if shortcut == 'none' else c['res'], shortcut == 'normed', lrelu)
        assert g['skip'].shape == g['out'].shape and g['skip'].mean() <= 1e-3
        what = ['out', 'dx'] + ([] if shortcut == 'none' else ['dres'])
    else:
        assert (int(g['Ns']), int(g['Nq']), int(g['ld']), int(g['width'])) == (c['Ns'], c['Nq'], c['ld'], c['width'])
        r = R.pool_run(c['x'], c['nbr'], c['width'], c['dy'])
        what = ['out', 'dx']
    for k in what:
        got, ref = r[k][::step], g[k]
        assert got.shape == ref.shape
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= 1e-10, (k, err)


def test_public_functions_refuse_cpu_tensors():
    from regtr_amd import backbone_grad
    x = torch.zeros(8, 32, requires_grad=True)
    off = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        backbone_grad.instance_norm(x, off, 8)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        backbone_grad.max_pool(x, torch.zeros((4, 3), dtype=torch.int32))
