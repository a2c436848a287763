"""The KPConv backward on the GPU (csrc/kpconv_bwd.hip, regtr_amd/kpconv_grad.py): the transposed neighbour table against its numpy
restatement, exactly; ops.kpconv_gather_bwd and KPConv.forward_grad's gradients against the float64 restatement of
tests/kpconv_grads_ref.py under its float32 error bounds AND the flat 1e-4 bar every gradient of this project is held to, and against
the reference module's goldens; forward bit-identity with KPConv.forward; determinism; independence of the forward's operand format;
one-sided requires_grad.

Every comparison prints err / bound and the flat ratio per case; docs/PARITY.md has the worst of each."""
import os

import numpy as np
import pytest
import torch

from tests import kpconv_grads_ref as R
from tests.util import ROOT

pytestmark = pytest.mark.gpu

SENTINEL = 777.0
GUARD = 5


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _check(name, got, ref, bound=None):
    err = np.abs(got.astype(np.float64) - ref)
    flat = float(err.max() / np.abs(ref).max())
    ratio = None
    if bound is not None:
        ratio = float((err / (bound + 1e-300)).max())
        print(f'  {name}: worst err/bound {ratio:.4f}, max err / max |ref| {flat:.2e}')
        assert ratio <= 1.0, (name, ratio)
    else:
        print(f'  {name}: max err / max |ref| {flat:.2e}')
    assert flat <= 1e-4, (name, flat)
    return ratio, flat


def _conv(c):
    """A regtr_amd KPConv with the case's parameters loaded through state_dict (weights + kernel_points, the reference's keys)."""
    from regtr_amd.kpconv import KPConv
    np.random.seed(0)
    conv = KPConv(R.KP, 3, c['Cin'], c['Cout'], c['extent'], c['radius']).cuda()
    assert list(conv.state_dict()) == ['weights', 'kernel_points']
    conv.load_state_dict({'weights': torch.from_numpy(c['weights']), 'kernel_points': torch.from_numpy(c['kernel_points'])}, strict=True)
    return conv


def _tensors(c):
    return _dev(c['q_pts']), _dev(c['s_pts']), _dev(c['nbr'], torch.int32), _dev(c['x']), _dev(c['d_out'])


@pytest.mark.parametrize('name', list(R.CASES))
def test_nbr_transpose_equals_numpy(name):
    from regtr_amd import ops
    c = R.draw_case(name)
    row_off, ent = ops.nbr_transpose(_dev(c['nbr'], torch.int32), c['Ns'])
    row_off2, ent2 = ops.nbr_transpose(_dev(c['nbr'], torch.int32), c['Ns'])
    torch.cuda.synchronize()
    ref_off, ref_ent = R.transpose_table(c['nbr'], c['Ns'])
    assert row_off.dtype == torch.int32 and ent.dtype == torch.int32
    assert np.array_equal(row_off.cpu().numpy(), ref_off)
    assert np.array_equal(ent.cpu().numpy()[:len(ref_ent)], ref_ent)
    assert torch.equal(row_off, row_off2) and torch.equal(ent[:len(ref_ent)], ent2[:len(ref_ent)])


def test_nbr_transpose_empty_and_all_shadow():
    from regtr_amd import ops
    row_off, _ = ops.nbr_transpose(torch.zeros((0, 7), dtype=torch.int32, device='cuda'), 11)
    assert row_off.cpu().tolist() == [0] * 12
    row_off, _ = ops.nbr_transpose(torch.zeros((0, 7), dtype=torch.int32, device='cuda'), 0)
    assert row_off.cpu().tolist() == [0]
    row_off, _ = ops.nbr_transpose(torch.full((9, 7), 11, dtype=torch.int32, device='cuda'), 11)
    assert row_off.cpu().tolist() == [0] * 12
    # more supports than one scan workgroup takes (1024), a negative index treated as a shadow
    rng = np.random.default_rng(1)
    nbr = rng.integers(-1, 5001, (3000, 5)).astype(np.int32)
    row_off, ent = ops.nbr_transpose(_dev(nbr, torch.int32), 5000)
    ref_off, ref_ent = R.transpose_table(nbr, 5000)
    assert np.array_equal(row_off.cpu().numpy(), ref_off) and np.array_equal(ent.cpu().numpy()[:len(ref_ent)], ref_ent)


@pytest.mark.parametrize('name', list(R.CASES))
def test_gather_bwd_vs_float64(name):
    from regtr_amd import ops
    c = R.draw_case(name)
    ns, nq, Cin, H = c['Ns'], c['Nq'], c['Cin'], c['H']
    dwf = np.random.default_rng(c['seed'] + 100).normal(0, 1, (nq, R.KP, Cin)).astype(np.float32)
    table = ops.nbr_transpose(_dev(c['nbr'], torch.int32), ns)
    buf = torch.full((ns + GUARD, Cin), SENTINEL, dtype=torch.float32, device='cuda')
    args = (_dev(dwf.reshape(nq, -1)), _dev(c['q_pts']), _dev(c['s_pts']), H, _dev(c['kernel_points']), c['extent'], table)
    dx = ops.kpconv_gather_bwd(*args, out=buf[:ns])
    again = ops.kpconv_gather_bwd(*args)
    torch.cuda.synchronize()
    assert dx.data_ptr() == buf.data_ptr() and torch.equal(dx, again)
    got = buf.cpu().numpy()
    assert np.all(got[ns:] == SENTINEL)                        # nothing past row Ns
    assert np.all(np.isfinite(got[:ns]))
    ref, bound = R.gather_bwd(c['q_pts'], c['s_pts'], c['nbr'], c['kernel_points'], c['extent'], dwf, ns)
    print(f'kpconv_gather_bwd {name}:')
    _check('dx', got[:ns], ref, bound)
    deg = np.diff(R.transpose_table(c['nbr'], ns)[0])
    zero = got[:ns][deg == 0]
    assert np.all(zero == 0) and not np.signbit(zero).any()    # a support nobody lists: an exact +0 row
    if c.get('orphan'):
        assert deg[R.ORPHAN] == 0


def _grads(c, f16=False, x_grad=True, w_grad=True, shared_table=False):
    from regtr_amd import ops
    conv = _conv(c)
    q, s, nbr, x, d_out = _tensors(c)
    x.requires_grad_(x_grad)
    conv.weights.requires_grad_(w_grad)
    table = ops.nbr_transpose(nbr, c['Ns']) if shared_table else None
    with ops.f16_pair(f16):
        out = conv.forward_grad(q, s, nbr, x, transposed=table)
        with torch.no_grad():
            plain = conv(q, s, nbr, x.detach())
    out.backward(d_out)
    torch.cuda.synchronize()
    return out, plain, x.grad, conv.weights.grad


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('name', list(R.CASES))
def test_forward_grad_vs_float64_and_reference(name, f16):
    c = R.draw_case(name)
    out, plain, dx, dw = _grads(c, f16=f16, shared_table=f16)
    assert torch.equal(out, plain)                             # the forward is KPConv.forward's, bit for bit
    assert tuple(dw.shape) == (R.KP, c['Cin'], c['Cout']) and tuple(dx.shape) == (c['Ns'], c['Cin'])
    r = R.run(c['q_pts'], c['s_pts'], c['nbr'], c['x'], c['weights'], c['kernel_points'], c['extent'], c['d_out'], bounds=True)
    print(f'KPConv.forward_grad {name} f16_pair={f16}:')
    _check('out (flat bar only)', out.detach().cpu().numpy(), r['out'])
    _check('x.grad', dx.cpu().numpy(), r['dx'], r['b_dx'])
    _check('weights.grad', dw.cpu().numpy(), r['dw'], r['b_dw'])
    g = np.load(os.path.join(ROOT, 'tests', 'golden', f'kpconv_grads_{name}.npz'))
    _check('x.grad vs reference module', dx.cpu().numpy()[::int(g['s_step'])], g['dx'])
    _check('weights.grad vs reference module', dw.cpu().numpy()[:, g['w_chan']], g['dw'])
    _check('out vs reference module', out.detach().cpu().numpy()[::int(g['q_step'])], g['out'])


@pytest.mark.parametrize('name', list(R.CASES))
def test_backward_is_bit_reproducible(name):
    c = R.draw_case(name)
    _, _, dx1, dw1 = _grads(c)
    _, _, dx2, dw2 = _grads(c, shared_table=True)
    assert torch.equal(dx1, dx2) and torch.equal(dw1, dw2)


@pytest.mark.parametrize('name', ['c1', 'c32'])
def test_one_sided_requires_grad(name):
    c = R.draw_case(name)
    _, _, dx, dw = _grads(c)
    _, _, dx_only, none_w = _grads(c, w_grad=False)
    _, _, none_x, dw_only = _grads(c, x_grad=False)
    assert none_w is None and none_x is None
    assert torch.equal(dx_only, dx) and torch.equal(dw_only, dw)


def test_double_backward_is_refused():
    c = R.draw_case('c32')
    conv = _conv(c)
    q, s, nbr, x, d_out = _tensors(c)
    x.requires_grad_()
    out = conv.forward_grad(q, s, nbr, x)
    (gx,) = torch.autograd.grad(out, x, d_out, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
