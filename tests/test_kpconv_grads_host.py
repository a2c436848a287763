"""CPU: the KPConv-backward entry points (regtr_nbr_transpose, regtr_kpconv_gather_bwd, regtr_row_div, regtr_gemm_tn_any) -- exported,
declared, and every refusal decided on the host with nothing launched; the float64 yardstick tests/kpconv_grads_ref.py pinned to the
reference module's goldens (tools/make_golden_kpconv_grads.py) and to float64 torch autograd; the transposed-table restatement."""
import os

import numpy as np
import pytest
import torch

from tests import kpconv_grads_ref as R
from tests.util import ROOT

FAKE = 0x10000          # never dereferenced: every call below is refused (or has nothing to do) before a launch
ENTRIES = ('regtr_nbr_transpose', 'regtr_nbr_transpose_ws_bytes', 'regtr_kpconv_gather_bwd', 'regtr_row_div', 'regtr_gemm_tn_any',
           'regtr_gemm_tn_any_ws_bytes')


def _lib():
    from regtr_amd import _lib as L
    return L.lib()


def _tr(nq=100, H=40, ns=100, ws_bytes=1 << 24, **kw):
    p = {n: kw.get(n, FAKE) for n in ('nbr', 'row_off', 'entries', 'ws')}
    return _lib().regtr_nbr_transpose(p['nbr'], nq, H, ns, p['row_off'], p['entries'], p['ws'], ws_bytes, None)


def _gb(nq=100, ns=100, H=40, Cin=32, KP=15, extent=0.1, **kw):
    p = {n: kw.get(n, FAKE) for n in ('dwf', 'q_xyz', 's_xyz', 'kp', 'row_off', 'entries', 'dx')}
    return _lib().regtr_kpconv_gather_bwd(p['dwf'], p['q_xyz'], nq, p['s_xyz'], ns, H, Cin, p['kp'], KP, extent, p['row_off'],
                                          p['entries'], p['dx'], None)


def _tn(M=100, N1=480, N2=32, ws_bytes=1 << 26, **kw):
    p = {n: kw.get(n, FAKE) for n in ('a', 'b', 'out', 'ws')}
    ld = {n: kw.get(n, d) for n, d in (('lda', N1), ('ldb', N2), ('ldo', N2))}
    return _lib().regtr_gemm_tn_any(p['a'], ld['lda'], p['b'], ld['ldb'], M, N1, N2, p['out'], ld['ldo'], p['ws'], ws_bytes, None)


def _rd(n=100, N=32, **kw):
    p = {k: kw.get(k, FAKE) for k in ('x', 'div', 'out')}
    return _lib().regtr_row_div(p['x'], kw.get('ldx', N), p['div'], n, N, p['out'], kw.get('ldo', N), None)


def test_entry_points_exported_and_declared():
    from regtr_amd import _lib as L
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    table = hdr.split('#ifndef REGTR_HIP_H')[0]
    for name in ENTRIES:
        assert hasattr(lib, name) and name in L.SIGNATURES and f'{name}(' in hdr, name
        if not name.endswith('_ws_bytes'):
            assert name + ' ' in table, name                   # the mapping table at the top
    assert '#define REGTR_ABI_VERSION 11' in hdr and L.ABI_VERSION == 11
    from regtr_amd import ops
    from regtr_amd.kpconv import KPConv
    assert callable(ops.nbr_transpose) and callable(ops.kpconv_gather_bwd) and callable(KPConv.forward_grad)


# ---- regtr_nbr_transpose
@pytest.mark.parametrize('name', ['nbr', 'row_off', 'entries', 'ws'])
def test_transpose_refuses_null_with_work(name):
    assert _tr(**{name: None}) == -2


@pytest.mark.parametrize('kw', [{'nq': -1}, {'ns': -1}, {'H': 0}, {'H': -4}, {'nq': 1 << 26, 'H': 40}])
def test_transpose_refuses_bad_counts(kw):
    assert _tr(**kw) == -2
    a = dict(nq=100, H=40, ns=100)
    a.update(kw)
    assert _lib().regtr_nbr_transpose_ws_bytes(a['nq'], a['H'], a['ns']) == 0


def test_transpose_workspace():
    L = _lib()
    need = L.regtr_nbr_transpose_ws_bytes(100, 40, 100)
    assert need >= (100 * 40 + 100) * 4                        # the scratch entry list and the cursors
    assert _tr(ws_bytes=need - 1) == -3 and _tr(ws_bytes=0) == -3
    assert L.regtr_nbr_transpose_ws_bytes(100000, 40, 100000) > need
    assert _tr(nq=0, ns=0, row_off=None) == -2                 # row_off is always written (row_off[0] = 0)


# ---- regtr_kpconv_gather_bwd
@pytest.mark.parametrize('name', ['dwf', 'q_xyz', 's_xyz', 'kp', 'row_off', 'entries', 'dx'])
def test_gather_bwd_refuses_null_with_work(name):
    assert _gb(**{name: None}) == -2


@pytest.mark.parametrize('kw', [{'nq': -1}, {'ns': -1}, {'H': 0}, {'H': 449}, {'Cin': 0}, {'Cin': -32}, {'Cin': 257}, {'Cin': 288}, {'KP': 0},
                                {'KP': 17}, {'extent': 0.0}, {'extent': -1.0}, {'extent': float('nan')}, {'nq': 1 << 26, 'H': 40}])
def test_gather_bwd_refuses_bad_shapes(kw):
    assert _gb(**kw) == -2


@pytest.mark.parametrize('name', ['dwf', 'dx'])
def test_gather_bwd_refuses_misaligned_base(name):
    assert _gb(**{name: FAKE + 4}) == -2
    assert _gb(**{name: FAKE + 8}) == -2


def test_gather_bwd_nothing_to_do_is_ok():
    assert _gb(ns=0) == 0
    assert _gb(ns=0, nq=0, dwf=None, q_xyz=None, s_xyz=None, row_off=None, entries=None, dx=None) == 0
    assert _gb(ns=0, Cin=257) == -2                            # ... but the shape checks still hold


# ---- regtr_gemm_tn_any / regtr_row_div
@pytest.mark.parametrize('kw', [{'M': -1}, {'N1': 0}, {'N2': 0}, {'N1': -64}, {'N1': 1 << 15, 'N2': 1 << 13}, {'lda': 479}, {'ldb': 31}, {'ldo': 31},
                                {'a': None}, {'b': None}, {'out': None}, {'ws': None}])
def test_gemm_tn_any_refusals(kw):
    assert _tn(**kw) == -2


def test_gemm_tn_any_workspace():
    L = _lib()
    need = L.regtr_gemm_tn_any_ws_bytes(100000, 480, 32)
    assert need >= 480 * 32 * 4 and need % (480 * 32 * 4) == 0
    assert _tn(M=100000, ws_bytes=need - 1) == -3
    assert L.regtr_gemm_tn_any_ws_bytes(-1, 480, 32) == 0 and L.regtr_gemm_tn_any_ws_bytes(100, 0, 32) == 0
    assert L.regtr_gemm_tn_any_ws_bytes(100, 15, 64) > 0


@pytest.mark.parametrize('kw', [{'n': -1}, {'N': 0}, {'ldx': 31}, {'ldo': 31}, {'x': None}, {'div': None}, {'out': None}])
def test_row_div_refusals(kw):
    assert _rd(**kw) == -2
    assert _rd(n=0, x=None, div=None, out=None) == 0


# ---- the yardstick
@pytest.mark.parametrize('name', list(R.CASES))
def test_yardstick_equals_reference_module(name):
    """The float64 restatement against the REAL reference KPConv's forward and gradients (goldens): 1e-10 relative."""
    c = R.draw_case(name)
    g = np.load(os.path.join(ROOT, 'tests', 'golden', f'kpconv_grads_{name}.npz'))
    assert int(g['seed']) == c['seed'] and (int(g['Cin']), int(g['Cout']), int(g['Ns']), int(g['Nq']), int(g['H'])) == \
        (c['Cin'], c['Cout'], c['Ns'], c['Nq'], c['H'])
    assert np.array_equal(g['kernel_points'], c['kernel_points']) and float(g['extent']) == c['extent']
    r = R.run(c['q_pts'], c['s_pts'], c['nbr'], c['x'], c['weights'], c['kernel_points'], c['extent'], c['d_out'])
    for got, ref, what in ((r['out'][::int(g['q_step'])], g['out'], 'out'), (r['dx'][::int(g['s_step'])], g['dx'], 'dx'),
                           (r['dw'][:, g['w_chan']], g['dw'], 'dw')):
        assert got.shape == ref.shape
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= 1e-10, (what, err)


def test_yardstick_equals_float64_autograd():
    rng = np.random.default_rng(5)
    ns, nq, H, Cin, Cout = 23, 9, 6, 3, 5
    s_pts, q_pts = rng.uniform(0, 1, (ns, 3)), rng.uniform(0, 1, (nq, 3))
    nbr = R.neighbours(q_pts, s_pts, 0.5, H)
    assert (nbr == ns).any() and (nbr < ns).any()
    kp, x = rng.normal(0, 0.15, (R.KP, 3)), rng.normal(0.2, 1, (ns, Cin))
    W, d_out = rng.normal(0, 1, (R.KP, Cin, Cout)), rng.normal(0, 1, (nq, Cout))
    r = R.run(q_pts, s_pts, nbr, x, W, kp, 0.3, d_out, bounds=True)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    xt, wt = t(x).requires_grad_(), t(W).requires_grad_()
    out = R.torch_forward(t(q_pts), t(s_pts), torch.from_numpy(nbr).long(), xt, wt, t(kp), 0.3)
    (out * t(d_out)).sum().backward()
    for got, ref in ((r['out'], out.detach().numpy()), (r['dx'], xt.grad.numpy()), (r['dw'], wt.grad.numpy())):
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    dx2, b2 = R.gather_bwd(q_pts, s_pts, nbr, kp, 0.3, r['dwf'], ns)
    assert np.allclose(dx2, r['dx'], rtol=1e-13, atol=0) and np.all(b2 <= r['b_dx']) and np.all(r['b_dx'] >= 0) and np.all(r['b_dw'] > 0)


@pytest.mark.parametrize('name', list(R.CASES))
def test_transposed_table_round_trips(name):
    c = R.draw_case(name)
    nbr, ns = c['nbr'], c['Ns']
    row_off, ent = R.transpose_table(nbr, ns)
    H = nbr.shape[1]
    assert row_off[0] == 0 and row_off[-1] == len(ent) == int((nbr < ns).sum())
    back = np.full_like(nbr, ns)
    for s in range(ns):
        seg = ent[row_off[s]:row_off[s + 1]]
        assert np.all(np.diff(seg) > 0)                        # ascending q H + h
        back.reshape(-1)[seg] = s
    assert np.array_equal(back, nbr)
    deg = np.diff(row_off)
    if c.get('hub'):
        assert deg[R.HUB] == nbr.shape[0] > 64
    if c.get('orphan'):
        assert deg[R.ORPHAN] == 0
    assert len(ent) < nbr.size                                 # shadows were dropped


def test_forward_grad_refuses_cpu_tensors_and_fused_forms():
    from regtr_amd.kpconv import KPConv
    np.random.seed(0)
    conv = KPConv(15, 3, 32, 32, 0.1, 0.25)
    x = torch.zeros(8, 32, requires_grad=True)
    pts, nbr = torch.zeros(8, 3), torch.zeros((8, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        conv.forward_grad(pts, pts, nbr, x)
    with pytest.raises(TypeError):
        conv.forward_grad(pts, pts, nbr, x, x_stats=x)
