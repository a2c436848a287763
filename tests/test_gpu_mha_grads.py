"""The attention backward (regtr_mha_bwd, csrc/attention_bwd.hip) and its autograd front (regtr_amd/attention.py) on the GPU: dq, dk,
dv against the float64 restatement of tests/mha_grads_ref.py under its float32 error bounds AND the flat 1e-4 bar the loss gradients
are held to; independence of the forward's precision; forward bit-identity with ops.mha; the nn.Module against float64
torch.nn.MultiheadAttention; determinism, double backward, no host synchronisation, exact zeros.

The launcher has ONE kernel per pass (k_mha_bwd_q, k_mha_bwd_kv: one wave per 32-row tile) and does not choose by problem size, so there
is no variant to steer; the segment lengths cover below / at / above one tile and many tiles."""
import numpy as np
import pytest
import torch

from tests import mha_grads_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
LENS = [1, 31, 32, 33, 64, 129, 257, 611]
SENTINEL = 777.0
PAD_ROWS = 5
KITCHEN = [410, 339, 394, 400]            # two kitchen-sized pairs: (410, 339) and (394, 400) tokens


def _pair_swap(n):
    kv = list(range(n))
    for i in range(0, n - 1, 2):
        kv[i], kv[i + 1] = i + 1, i
    return kv


def _layout(name):
    if name == 'self':
        return LENS, list(range(len(LENS)))
    if name == 'cross':
        return LENS, _pair_swap(len(LENS))
    if name == 'shared':            # clouds 0, 1, 2 all attend cloud 1; clouds 2 and 4 are attended by nobody
        return [33, 64, 129, 31, 257], [1, 1, 1, 0, 3]
    if name == 'empty':             # a self-attending cloud of length 0 in the middle of the batch
        return [33, 0, 64, 1], [0, 1, 2, 3]
    rng = np.random.default_rng(13)
    lens = [int(x) for x in rng.integers(1, 300, 13)]
    return lens, (list(range(13)) if name == 'ragged_self' else _pair_swap(13))


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _inputs(lens, n_heads, peaked, seed):
    """A packed (N + PAD_ROWS, 3E) projection (q | k | v column blocks) and d_out (N + PAD_ROWS, E), N(0, 1)."""
    rng = np.random.default_rng(seed)
    E = 32 * n_heads
    n = sum(lens) + PAD_ROWS
    qkv = rng.normal(0, 1, (n, 3 * E)).astype(F32)
    if peaked:
        qkv[:, :2 * E] *= 8          # scores of std ~ 64 / sqrt(32) * 5.7: the rows saturate
    return qkv, rng.normal(0, 1, (n, E)).astype(F32)


def _check(name, got, ref, bound, n_live):
    err = np.abs(got[:n_live].astype(np.float64) - ref[:n_live])
    q = err / (bound[:n_live] + 1e-300)
    ratio = float(q.max())
    w = np.unravel_index(int(q.argmax()), q.shape)
    print(f'  {name}: worst ratio at {w}: got {got[w]!r} ref {ref[w]!r} bound {bound[w]!r}')
    flat = float(err.max() / np.abs(ref).max())
    print(f'  {name}: worst err/bound {ratio:.4f}, max err / max |ref| {flat:.2e}')
    assert ratio <= 1.0, (name, ratio)
    assert flat <= 1e-4, (name, flat)
    return ratio


CASES = [(lay, 8, pk) for lay in ('self', 'cross', 'shared', 'empty', 'ragged_self', 'ragged_cross') for pk in (False, True)] + [('cross', 1, False)]


@pytest.mark.parametrize('layout,n_heads,peaked', CASES)
def test_grads_vs_float64(layout, n_heads, peaked):
    from regtr_amd import ops
    lens, kv = _layout(layout)
    E = 32 * n_heads
    n_live = sum(lens)
    qkv, d_out = _inputs(lens, n_heads, peaked, 100 + len(lens) + n_heads + peaked)
    seg = R.offsets(lens)
    t = _dev(qkv)
    out = torch.full((n_live + PAD_ROWS, 3 * E), SENTINEL, dtype=torch.float32, device='cuda')
    dq, dk, dv = ops.mha_bwd(t[:, :E], t[:, E:2 * E], t[:, 2 * E:], _dev(d_out), _dev(seg, torch.int32), _dev(np.array(kv), torch.int32),
                             max(lens), n_heads, out=out)
    torch.cuda.synchronize()
    assert dq.data_ptr() == out.data_ptr() and dk.data_ptr() == out.data_ptr() + 4 * E and dv.data_ptr() == out.data_ptr() + 8 * E
    got = out.cpu().numpy()
    assert np.all(got[n_live:] == SENTINEL)                  # rows outside every cloud are not written
    assert np.all(np.isfinite(got[:n_live]))
    ref = R.core(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], d_out, seg, kv, n_heads, bounds=True)
    print(f'mha_bwd {layout} heads={n_heads} peaked={peaked}:')
    worst = max(_check(n, got[:, i * E:(i + 1) * E], ref[n], ref['b_' + n], n_live) for i, n in enumerate(('dq', 'dk', 'dv')))
    if layout == 'shared':
        for c in (2, 4):                                     # attended by nobody: zero rows, written
            assert np.all(got[seg[c]:seg[c + 1], E:] == 0)
    print(f'mha_bwd {layout} heads={n_heads} peaked={peaked}: worst err/bound {worst:.4f}')


def _autograd_run(qkv, d_out, lens, kv, n_heads, precision, grad=True):
    from regtr_amd.attention import packed_mha
    E = 32 * n_heads
    t = _dev(qkv)
    if grad:
        t.requires_grad_()
    o = packed_mha(t[:, :E], t[:, E:2 * E], t[:, 2 * E:], _dev(R.offsets(lens), torch.int32), _dev(np.array(kv), torch.int32), max(lens),
                   n_heads, precision)
    if grad:
        o.backward(_dev(d_out))
    torch.cuda.synchronize()
    return o.detach(), (t.grad if grad else None)


@pytest.mark.parametrize('layout', ['self', 'cross'])
def test_grads_do_not_depend_on_forward_precision(layout):
    lens, kv = _layout(layout)
    qkv, d_out = _inputs(lens, 8, False, 5)
    grads = [_autograd_run(qkv, d_out, lens, kv, 8, p)[1] for p in range(4)]
    n_live = sum(lens)
    assert torch.all(grads[0][n_live:] == 0) and torch.any(grads[0][:n_live] != 0)
    for p in range(1, 4):
        assert torch.equal(grads[0].view(torch.int32), grads[p].view(torch.int32)), p


@pytest.mark.parametrize('precision', [0, 1, 2, 3])
def test_forward_bit_identical_to_ops_mha(precision):
    from regtr_amd import ops
    lens, kv = _layout('cross')
    E = 256
    qkv, d_out = _inputs(lens, 8, False, 6)
    t = _dev(qkv)
    ref = ops.mha(t[:, :E], t[:, E:2 * E], t[:, 2 * E:], _dev(R.offsets(lens), torch.int32), _dev(np.array(kv), torch.int32), max(lens), 8,
                  precision)
    n_live = sum(lens)
    for grad in (False, True):
        o, _ = _autograd_run(qkv, d_out, lens, kv, 8, precision, grad=grad)
        assert torch.equal(o[:n_live].view(torch.int32), ref[:n_live].view(torch.int32)), grad


@pytest.mark.parametrize('mode', ['self', 'cross'])
def test_module_vs_float64_multihead_attention(mode):
    from regtr_amd.attention import PackedMultiheadAttention
    rng = np.random.default_rng(21 + (mode == 'cross'))
    E, H = 256, 8
    lens = KITCHEN
    kv = list(range(4)) if mode == 'self' else _pair_swap(4)
    seg = R.offsets(lens)
    N = sum(lens)
    ref_mod = torch.nn.MultiheadAttention(E, H)
    w_in, w_out = ref_mod.in_proj_weight.detach().numpy(), ref_mod.out_proj.weight.detach().numpy()
    b_in, b_out = rng.normal(0, 0.1, 3 * E).astype(F32), rng.normal(0, 0.1, E).astype(F32)
    xq = rng.normal(0, 1, (N, E)).astype(F32)
    # self: one tensor for query, key and value (the packed projection path); cross: three different ones
    xk, xv = (xq, xq) if mode == 'self' else (rng.normal(0, 1, (N, E)).astype(F32), rng.normal(0, 1, (N, E)).astype(F32))
    d_y = rng.normal(0, 1, (N, E)).astype(F32)
    ref = R.torch_module(xq, xk, xv, w_in, b_in, w_out, b_out, d_y, seg, kv, H)

    m = PackedMultiheadAttention(E, H).cuda()
    m.load_state_dict({'in_proj_weight': torch.from_numpy(w_in), 'in_proj_bias': torch.from_numpy(b_in),
                       'out_proj.weight': torch.from_numpy(w_out), 'out_proj.bias': torch.from_numpy(b_out)})
    tq = _dev(xq).requires_grad_()
    tk, tv = (tq, tq) if mode == 'self' else (_dev(xk).requires_grad_(), _dev(xv).requires_grad_())
    y = m(tq, tk, tv, _dev(seg, torch.int32), _dev(np.array(kv), torch.int32), max(lens))
    y.backward(_dev(d_y))
    torch.cuda.synchronize()
    err_y = float(np.abs(y.detach().cpu().numpy() - ref['y']).max())
    print(f'module {mode}: output max abs err {err_y:.2e}')
    assert err_y <= 1e-4
    got = {'d_in_proj_weight': m.in_proj_weight.grad, 'd_in_proj_bias': m.in_proj_bias.grad, 'd_out_proj_weight': m.out_proj.weight.grad,
           'd_out_proj_bias': m.out_proj.bias.grad}
    if mode == 'self':
        got['d_x'] = tq.grad
        ref['d_x'] = ref['d_query'] + ref['d_key'] + ref['d_value']
    else:
        got.update({'d_query': tq.grad, 'd_key': tk.grad, 'd_value': tv.grad})
    for name, g in got.items():
        err = float(np.abs(g.cpu().numpy() - ref[name]).max() / np.abs(ref[name]).max())
        print(f'module {mode}: {name} max err / max |ref| {err:.2e}')
        assert err <= 1e-4, (name, err)


def test_backward_bit_reproducible():
    lens, kv = _layout('shared')
    qkv, d_out = _inputs(lens, 8, False, 9)
    a = _autograd_run(qkv, d_out, lens, kv, 8, 0)[1].cpu().numpy()
    b = _autograd_run(qkv, d_out, lens, kv, 8, 0)[1].cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    lens, kv = KITCHEN, _pair_swap(4)
    qkv, d_out = _inputs(lens, 8, False, 10)
    a = _autograd_run(qkv, d_out, lens, kv, 8, 0)[1].cpu().numpy()
    b = _autograd_run(qkv, d_out, lens, kv, 8, 0)[1].cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_double_backward_refused():
    from regtr_amd.attention import packed_mha
    lens, kv = [40, 50], [1, 0]
    qkv, _ = _inputs(lens, 1, False, 2)
    q, k, v = (_dev(qkv[:, 32 * i:32 * i + 32].copy()).requires_grad_() for i in range(3))
    o = packed_mha(q, k, v, _dev(R.offsets(lens), torch.int32), _dev(np.array(kv), torch.int32), 50, 1)
    (gq,) = torch.autograd.grad(o.sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        gq.sum().backward()


def test_needs_input_grad_is_honoured():
    from regtr_amd.attention import packed_mha
    lens, kv = [40, 50], [1, 0]
    qkv, _ = _inputs(lens, 1, False, 2)
    q, k, v = (_dev(qkv[:, 32 * i:32 * i + 32].copy()) for i in range(3))
    k.requires_grad_()
    packed_mha(q, k, v, _dev(R.offsets(lens), torch.int32), _dev(np.array(kv), torch.int32), 50, 1).sum().backward()
    assert q.grad is None and v.grad is None and k.grad is not None and torch.isfinite(k.grad).all()


def test_no_host_sync():
    from regtr_amd.attention import PackedMultiheadAttention
    lens, kv = KITCHEN, _pair_swap(4)
    m = PackedMultiheadAttention(256, 8).cuda()
    x = torch.randn(sum(lens), 256, device='cuda', requires_grad=True)
    seg, kvt = _dev(R.offsets(lens), torch.int32), _dev(np.array(kv), torch.int32)
    g = torch.randn(sum(lens), 256, device='cuda')

    def step():
        y = m(x, x, x, seg, kvt, max(lens))
        y.backward(g)
        return y
    step()                                                  # first-call preparation
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        y = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and torch.isfinite(m.in_proj_weight.grad).all()


def test_zero_upstream_gradient_of_a_cloud_gives_exact_zero_dq():
    from regtr_amd import ops
    lens, kv = _layout('cross')
    qkv, d_out = _inputs(lens, 8, False, 12)
    seg = R.offsets(lens)
    c = 5
    d_out[seg[c]:seg[c + 1]] = 0
    t = _dev(qkv)
    dq, dk, dv = ops.mha_bwd(t[:, :256], t[:, 256:512], t[:, 512:], _dev(d_out), _dev(seg, torch.int32), _dev(np.array(kv), torch.int32),
                             max(lens), 8)
    torch.cuda.synchronize()
    assert torch.all(dq[seg[c]:seg[c + 1]] == 0)
    assert torch.any(dq[seg[c - 1]:seg[c]] != 0) and torch.any(dk[seg[c]:seg[c + 1]] != 0)
    assert torch.all(dq[sum(lens):] == 0)                   # out=None: a zero-filled buffer, the padding rows stay 0
