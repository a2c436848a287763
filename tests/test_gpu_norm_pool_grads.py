"""The InstanceNorm (+ LeakyReLU, + shortcut) and max-pool backward on the GPU (csrc/norm_pool_bwd.hip, regtr_amd/backbone_grad.py):
forward bit-identity with ops.instnorm_apply(ops.instnorm_stats(...)) and ops.maxpool; dx / dres against the float64 restatement of
tests/norm_pool_grads_ref.py under its derived float32 bound AND the flat 1e-4 bar every gradient of this project is held to (the
restatement is given the sign of the forward's own output as the LeakyReLU mask, so no element is left out), and against the reference
code's goldens; the pool gradient bit-equal to the float32 ordered restatement and the stored argmax equal to numpy's; determinism;
one-sided requires_grad; sentinel guards around every output.  C-ABI refusals: tests/test_norm_pool_grads_host.py (decided on the host).

Every launcher here has ONE instantiation of each of its kernels (the lanes per row are a launch argument).  What the cases reach:
  in_c4 / in_c64 / in_c256 / in_c1024   1 / 16 / 64 / 256 float4 columns, i.e. 256 / 16 / 4 / 1 row-threads; clouds [1, 0, 5, R + 1]
  in_chunks                             66 chunks in one cloud at C = 32: the fixed-order combine beyond one wave of lanes
  in_g*                                 the goldens' shapes;  every 'in' case runs act none / LeakyReLU x no / plain / normalised shortcut
  pool_h1 / pool_h7 / pool_h40          H = 1, 7, 40 at C = 4, 64, 1024 (1, 16, 64 lanes per row, the last striding four times); all-shadow
                                        rows (h1, h7), an in-degree-0 support (h7), an in-degree-70 support and a -1 index (h40)
  pool_width                            width 5 < ld 9, full rows with a negative maximum;  pool_ties: quantised x;  nq = 0: its own test

Every comparison prints err / bound and the flat ratio per case; docs/PARITY.md has the worst of each."""
import os

import numpy as np
import pytest
import torch

from tests import norm_pool_grads_ref as R
from tests.util import ROOT

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
GUARD = 5


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _check(name, got, ref, bound=None, keep=None):
    err = np.abs(got.astype(np.float64) - ref)
    if keep is not None:
        err = err * keep
    flat = float(err.max() / np.abs(ref).max())
    if bound is not None:
        ratio = float((err / (bound + 1e-300)).max())
        print(f'  {name}: worst err/bound {ratio:.4f}, max err / max |ref| {flat:.2e}')
        assert ratio <= 1.0, (name, ratio)
    else:
        print(f'  {name}: max err / max |ref| {flat:.2e}')
    assert flat <= 1e-4, (name, flat)


def _guarded(rows, C, dtype=torch.float32):
    """A (rows, C) view with GUARD sentinel rows on either side."""
    buf = torch.full((rows + 2 * GUARD, C), SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf, rows):
    b = buf.cpu().numpy()
    return bool(np.all(b[:GUARD] == SENTINEL) and np.all(b[GUARD + rows:] == SENTINEL))


# ------------------------------------------------------------------------------------------------ InstanceNorm
def _in_grads(c, lrelu, shortcut, x_grad=True, r_grad=True):
    from regtr_amd import backbone_grad, ops
    x, dy, off = _dev(c['x']).requires_grad_(x_grad), _dev(c['dy']), _dev(c['seg_off'], torch.int32)
    res = None if shortcut == 'none' else _dev(c['res']).requires_grad_(r_grad)
    normed = shortcut == 'normed'
    y = backbone_grad.instance_norm(x, off, c['max_len'], res, normed, lrelu, R.SLOPE, R.EPS)
    with torch.no_grad():
        st = ops.instnorm_stats(x, off, c['max_len'], R.EPS)
        rst = ops.instnorm_stats(res, off, c['max_len'], R.EPS) if normed else None
        plain = ops.instnorm_apply(x, off, c['max_len'], st, res, rst, lrelu=lrelu, slope=R.SLOPE)
    if x_grad or (res is not None and r_grad):
        y.backward(dy)
    torch.cuda.synchronize()
    return y, plain, x.grad, None if res is None else res.grad


_in_cache = {}


def _in_ref(name, lrelu, shortcut, mask):
    """The float64 restatement with its bounds, computed once per (case, variant) -- the mask is the same forward output every time."""
    key = (name, lrelu, shortcut)
    if key not in _in_cache:
        c = R.draw_case(name)
        _in_cache[key] = R.instnorm_run(c['x'], c['lens'], c['dy'], None if shortcut == 'none' else c['res'], shortcut == 'normed', lrelu,
                                        mask=mask, slope=R.SLOPE32, eps=R.EPS32, bounds=True)
    return _in_cache[key]


@pytest.mark.parametrize('lrelu,shortcut', R.VARIANTS)
@pytest.mark.parametrize('name', R.IN_CASES)
def test_instance_norm_vs_float64_and_reference(name, lrelu, shortcut):
    c = R.draw_case(name)
    y, plain, dx, dres = _in_grads(c, lrelu, shortcut)
    assert torch.equal(y, plain)                               # the forward is the two plain ops', bit for bit
    out = y.detach().cpu().numpy()
    r = _in_ref(name, lrelu, shortcut, out > 0)
    print(f'instance_norm {name} lrelu={lrelu} shortcut={shortcut}:')
    _check('out (flat bar only)', out, r['out'])
    _check('x.grad', dx.cpu().numpy(), r['dx'], r['b_dx'])
    if shortcut != 'none':
        _check('residual.grad', dres.cpu().numpy(), r['dres'], r['b_dres'])
    for n, o in zip(c['lens'], c['seg_off']):
        if n == 1:                                             # a one-row cloud: dx = 0 exactly
            assert np.all(dx.cpu().numpy()[o] == 0)
    if c.get('golden') == (lrelu, shortcut):
        g = np.load(os.path.join(ROOT, 'tests', 'golden', f'norm_pool_grads_{name}.npz'))
        step, keep = int(g['step']), ~g['skip']
        _check('out vs reference module', out[::step], g['out'], keep=keep)
        _check('x.grad vs reference module', dx.cpu().numpy()[::step], g['dx'], keep=keep)
        if shortcut != 'none':
            _check('residual.grad vs reference module', dres.cpu().numpy()[::step], g['dres'], keep=keep)


@pytest.mark.parametrize('name', ['in_c4', 'in_c1024', 'in_chunks'])
def test_instnorm_bwd_writes_its_rows_only_and_is_bit_reproducible(name):
    """ops.instnorm_bwd into guarded buffers, packed rows followed by rows that belong to no cloud: every output row of every cloud written,
    nothing before, after or beyond the last cloud; two runs equal."""
    from regtr_amd import ops
    c = R.draw_case(name)
    N, C = c['x'].shape
    pad = lambda a: _dev(np.concatenate([a, np.full((3, C), 5.0, np.float32)]))
    x, res, dy, off = pad(c['x']), pad(c['res']), pad(c['dy']), _dev(c['seg_off'], torch.int32)
    st, rst = ops.instnorm_stats(x, off, c['max_len'], R.EPS), ops.instnorm_stats(res, off, c['max_len'], R.EPS)
    bx, vx = _guarded(N + 3, C)
    br, vr = _guarded(N + 3, C)
    dx, dres = ops.instnorm_bwd(x, off, c['max_len'], st, dy, res, rst, True, R.SLOPE, want_dres=True, out_dx=vx, out_dres=vr)
    dx2, dres2 = ops.instnorm_bwd(x, off, c['max_len'], st, dy, res, rst, True, R.SLOPE, want_dres=True)
    torch.cuda.synchronize()
    assert dx.data_ptr() == vx.data_ptr() and _guards_intact(bx, N + 3) and _guards_intact(br, N + 3)
    for got, again in ((vx, dx2), (vr, dres2)):
        assert torch.all(got[N:] == SENTINEL) and torch.equal(got[:N], again[:N]) and torch.isfinite(got[:N]).all()


@pytest.mark.parametrize('shortcut', ['plain', 'normed'])
def test_instance_norm_one_sided_requires_grad(shortcut):
    c = R.draw_case('in_c64')
    _, _, dx, dres = _in_grads(c, True, shortcut)
    _, _, dx_only, none_r = _in_grads(c, True, shortcut, r_grad=False)
    _, _, none_x, dres_only = _in_grads(c, True, shortcut, x_grad=False)
    assert none_r is None and none_x is None
    assert torch.equal(dx_only, dx) and torch.equal(dres_only, dres)
    y, plain, none_x, none_r = _in_grads(c, True, shortcut, x_grad=False, r_grad=False)
    assert not y.requires_grad and torch.equal(y, plain)


# ------------------------------------------------------------------------------------------------ max-pool
def _pool_grads(c, shared_table=False):
    from regtr_amd import backbone_grad, ops
    x, nbr, dy = _dev(c['x']).requires_grad_(), _dev(c['nbr'], torch.int32), _dev(c['dy'])
    width = None if c['width'] == c['ld'] else c['width']
    table = None
    if shared_table:
        table = ops.nbr_transpose(nbr if width is None else nbr[:, :width].contiguous(), c['Ns'])
    out = backbone_grad.max_pool(x, nbr, width, transposed=table)
    with torch.no_grad():
        plain = ops.maxpool(x, nbr, width)
    out.backward(dy)
    torch.cuda.synchronize()
    return out, plain, x.grad


@pytest.mark.parametrize('name', R.POOL_CASES)
def test_max_pool_vs_restatements_and_reference(name):
    from regtr_amd import ops
    c = R.draw_case(name)
    ns, nq, C, width = c['Ns'], c['Nq'], c['C'], c['width']
    out, plain, dx = _pool_grads(c)
    _, _, dx2 = _pool_grads(c, shared_table=True)
    assert torch.equal(out, plain)                             # the forward is ops.maxpool's, bit for bit
    assert torch.equal(dx, dx2)                                # run to run, own table or a shared one
    r = R.pool_run(c['x'], c['nbr'], width, c['dy'])
    assert np.array_equal(out.detach().cpu().numpy().astype(np.float64), r['out'])
    # the stored argmax, into a guarded buffer: numpy's, exactly
    ba, va = _guarded(nq, C, torch.int16)
    arg = ops.maxpool_argmax(_dev(c['x']), _dev(c['nbr'], torch.int32), None if width == c['ld'] else width, out=va)
    torch.cuda.synchronize()
    assert arg.dtype == torch.int16 and np.array_equal(va.cpu().numpy(), r['arg']) and _guards_intact(ba, nq)
    # the gradient, into a guarded buffer: the float32 ordered restatement, bit for bit
    bd, vd = _guarded(ns, C)
    table = ops.nbr_transpose(_dev(c['nbr'][:, :width], torch.int32), ns)
    ops.maxpool_bwd(_dev(c['dy']), arg, width, table, out=vd)
    torch.cuda.synchronize()
    ref32 = R.pool_bwd_f32(c['dy'], r['arg'], c['nbr'], width, ns)
    got = vd.cpu().numpy()
    assert _guards_intact(bd, ns) and np.array_equal(got.view(np.uint32), ref32.view(np.uint32))
    assert np.array_equal(dx.cpu().numpy().view(np.uint32), ref32.view(np.uint32))
    print(f'max_pool {name}:')
    _check('x.grad', got, r['dx'])
    if c.get('orphan'):
        assert np.all(got[R.ORPHAN] == 0) and not np.signbit(got[R.ORPHAN]).any()      # a support nobody lists: an exact +0 row
    if c.get('golden'):
        g = np.load(os.path.join(ROOT, 'tests', 'golden', f'norm_pool_grads_{name}.npz'))
        step = int(g['step'])
        assert np.array_equal(out.detach().cpu().numpy()[::step].astype(np.float64), g['out'])
        _check('x.grad vs reference code', got[::step], g['dx'])


def test_max_pool_without_queries_or_supports():
    from regtr_amd import ops
    C, ns = 64, 11
    nbr = torch.zeros((0, 7), dtype=torch.int32, device='cuda')
    arg = ops.maxpool_argmax(torch.randn(ns, C, device='cuda'), nbr)
    assert tuple(arg.shape) == (0, C)
    bd, vd = _guarded(ns, C)
    ops.maxpool_bwd(torch.zeros((0, C), device='cuda'), arg, 7, ops.nbr_transpose(nbr, ns), out=vd)
    torch.cuda.synchronize()
    assert _guards_intact(bd, ns) and torch.all(vd == 0) and not torch.signbit(vd).any()
    # no supports: every winner is the shadow row, and there is no dx row to write
    nbr = torch.zeros((9, 7), dtype=torch.int32, device='cuda')
    arg = ops.maxpool_argmax(torch.zeros((0, C), device='cuda'), nbr)
    dx = ops.maxpool_bwd(torch.randn(9, C, device='cuda'), arg, 7, ops.nbr_transpose(nbr, 0))
    torch.cuda.synchronize()
    assert torch.all(arg == -1) and tuple(dx.shape) == (0, C)


def test_double_backward_is_refused():
    from regtr_amd import backbone_grad
    c = R.draw_case('pool_h7')
    x = _dev(c['x']).requires_grad_()
    out = backbone_grad.max_pool(x, _dev(c['nbr'], torch.int32))
    (gx,) = torch.autograd.grad(out, x, _dev(c['dy']), create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
