"""CPU: the attention-backward entry points (regtr_mha_bwd / regtr_mha_bwd_ws_bytes) -- exported, declared, and every refusal decided
on the host with nothing launched; the float64 yardstick tests/mha_grads_ref.py pinned to torch.nn.MultiheadAttention (the class the
reference's transformers.py:197-226 calls); PackedMultiheadAttention's state_dict layout; packed_mha's refusal of CPU tensors."""
import numpy as np
import pytest
import torch

from tests import mha_grads_ref as R


def _lib():
    from regtr_amd import _lib as L
    return L.lib()


FAKE = 0x10000          # never dereferenced: every call below is refused (or has nothing to do) before a launch


def _bwd(n_heads=8, n_clouds=2, n_total=64, max_len=32, head_dim=32, ws_bytes=1 << 20, **kw):
    p = {n: kw.get(n, FAKE) for n in ('q', 'k', 'v', 'd_out', 'dq', 'dk', 'dv', 'seg_off', 'kv_of', 'ws')}
    ld = {n: kw.get(n, 3 * n_heads * 32) for n in ('ldq', 'ldk', 'ldv', 'ld_do', 'ld_dq', 'ld_dk', 'ld_dv')}
    return _lib().regtr_mha_bwd(p['q'], ld['ldq'], p['k'], ld['ldk'], p['v'], ld['ldv'], p['d_out'], ld['ld_do'],
                                p['dq'], ld['ld_dq'], p['dk'], ld['ld_dk'], p['dv'], ld['ld_dv'], p['seg_off'], p['kv_of'],
                                n_clouds, n_total, max_len, n_heads, head_dim, 32 ** -0.5, p['ws'], ws_bytes, None)


def test_entry_points_exported_and_declared():
    import os
    from regtr_amd import _lib as L
    from tests.util import ROOT
    lib = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    for name in ('regtr_mha_bwd', 'regtr_mha_bwd_ws_bytes'):
        assert hasattr(lib, name) and name in L.SIGNATURES and f'{name}(' in hdr
    assert 'regtr_mha_bwd ' in hdr.split('#ifndef REGTR_HIP_H')[0]           # the mapping table at the top


@pytest.mark.parametrize('name', ['q', 'k', 'v', 'd_out', 'dq', 'dk', 'dv', 'seg_off', 'kv_of', 'ws'])
def test_refuses_null_with_work(name):
    assert _bwd(**{name: None}) == -2


@pytest.mark.parametrize('kw', [{'n_clouds': 0}, {'n_clouds': -1}, {'n_total': -1}, {'max_len': -1}, {'n_heads': -1}, {'n_heads': 0}])
def test_refuses_bad_counts(kw):
    assert _bwd(**kw) == -2


@pytest.mark.parametrize('hd', [0, 16, 64, -32])
def test_refuses_other_head_dims(hd):
    assert _bwd(head_dim=hd) == -2


@pytest.mark.parametrize('name', ['ldq', 'ldk', 'ldv', 'ld_do', 'ld_dq', 'ld_dk', 'ld_dv'])
def test_refuses_bad_strides(name):
    assert _bwd(**{name: 8 * 32 + 2}) == -2           # not a multiple of 4
    assert _bwd(**{name: 8 * 32 - 4}) == -2           # below n_heads * 32
    assert _bwd(ws_bytes=0, **{name: 8 * 32}) == -3   # legal: gets as far as the workspace check (too small: nothing launched)
    assert _bwd(**{name: 0}) == -2 and _bwd(**{name: -256}) == -2


@pytest.mark.parametrize('name', ['q', 'k', 'v', 'd_out', 'dq', 'dk', 'dv'])
def test_refuses_misaligned_base(name):
    assert _bwd(**{name: FAKE + 4}) == -2
    assert _bwd(**{name: FAKE + 8}) == -2


def test_workspace():
    L = _lib()
    need = L.regtr_mha_bwd_ws_bytes(64, 8)
    assert need >= 2 * 64 * 8 * 4                     # lse and delta per (row, head)
    assert _bwd(ws_bytes=need - 1) == -3 and _bwd(ws_bytes=0) == -3
    assert L.regtr_mha_bwd_ws_bytes(-1, 8) == 0 and L.regtr_mha_bwd_ws_bytes(64, -8) == 0
    assert L.regtr_mha_bwd_ws_bytes(100000, 8) > L.regtr_mha_bwd_ws_bytes(1000, 8) > 0


def test_nothing_to_do_is_ok():
    assert _bwd(max_len=0) == 0
    assert _bwd(max_len=0, q=None, k=None, v=None, d_out=None, dq=None, dk=None, dv=None, ws=None, ws_bytes=0) == 0
    assert _bwd(max_len=0, head_dim=16) == -2         # ... but the shape checks still hold


# the ragged three-pair layout of test 2: six clouds, pair (2 b, 2 b + 1)
LENS = [37, 21, 5, 64, 33, 1]
KV = {'self': [0, 1, 2, 3, 4, 5], 'cross': [1, 0, 3, 2, 5, 4]}


@pytest.mark.parametrize('mode', ['self', 'cross'])
def test_yardstick_equals_torch_multihead_attention(mode):
    """Validates the yardstick, not the product: passes without the feature by design."""
    rng = np.random.default_rng(7 + (mode == 'cross'))
    E, H = 64, 2
    N = sum(LENS)
    seg, kv = R.offsets(LENS), KV[mode]
    x = [rng.normal(0, 1, (N, E)) for _ in range(3)]
    w_in, b_in = rng.normal(0, E ** -0.5, (3 * E, E)), rng.normal(0, 0.1, 3 * E)
    w_out, b_out = rng.normal(0, E ** -0.5, (E, E)), rng.normal(0, 0.1, E)
    d_y = rng.normal(0, 1, (N, E))
    got = R.module(*x, w_in, b_in, w_out, b_out, d_y, seg, kv, H)
    ref = R.torch_module(*x, w_in, b_in, w_out, b_out, d_y, seg, kv, H)
    assert set(got) == set(ref)
    for name in ref:
        err = np.abs(got[name] - ref[name]).max() / np.abs(ref[name]).max()
        assert err <= 1e-10, (name, err)


def test_yardstick_bounds_cover_a_float32_numpy_evaluation():
    """The bounds are positive on every row of a cloud, and a plain float32 numpy evaluation of the same formulas stays inside them."""
    rng = np.random.default_rng(3)
    N, E = sum(LENS) + 3, 64                              # three padding rows past the last cloud
    q, k, v, g = (rng.normal(0, 1, (N, E)).astype(np.float32) for _ in range(4))
    seg, kv = R.offsets(LENS), KV['cross']
    r = R.core(q, k, v, g, seg, kv, 2, bounds=True)
    plain = R.core(q, k, v, g, seg, kv, 2)
    scale = np.float32(32 ** -0.5)
    for n in ('dq', 'dk', 'dv'):
        assert np.array_equal(plain[n], r[n])
        b = r['b_' + n]
        assert np.all(b[:seg[-1]] > 0) and np.all(np.isfinite(b)) and np.all(b[seg[-1]:] == 0) and np.all(r[n][seg[-1]:] == 0), n
    f32 = {n: np.zeros((N, E), np.float32) for n in ('dq', 'dk', 'dv')}
    for c in range(len(kv)):
        qs, ks = slice(seg[c], seg[c + 1]), slice(seg[kv[c]], seg[kv[c] + 1])
        for h in range(2):
            cs = slice(32 * h, 32 * h + 32)
            s_ = scale * (q[qs, cs] @ k[ks, cs].T)
            e = np.exp(s_ - s_.max(1, keepdims=True))
            P = e / e.sum(1, keepdims=True, dtype=np.float32)
            dP = g[qs, cs] @ v[ks, cs].T
            dS = P * (dP - (P * dP).sum(1, keepdims=True, dtype=np.float32))
            f32['dq'][qs, cs] = scale * (dS @ k[ks, cs])
            f32['dk'][ks, cs] += scale * (dS.T @ q[qs, cs])
            f32['dv'][ks, cs] += P.T @ g[qs, cs]
    for n in ('dq', 'dk', 'dv'):
        ratio = np.abs(f32[n] - r[n]) / (r['b_' + n] + 1e-300)
        assert ratio.max() <= 1.0, (n, ratio.max())


def test_state_dict_matches_multihead_attention():
    from regtr_amd.attention import PackedMultiheadAttention
    ref = torch.nn.MultiheadAttention(256, 8)
    m = PackedMultiheadAttention(256, 8)
    sd, rsd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rsd) == ['in_proj_weight', 'in_proj_bias', 'out_proj.weight', 'out_proj.bias']
    assert [tuple(t.shape) for t in sd.values()] == [tuple(t.shape) for t in rsd.values()]
    m.load_state_dict(rsd, strict=True)
    for k_ in rsd:
        assert torch.equal(m.state_dict()[k_], rsd[k_])
    assert all(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match='head_dim'):
        PackedMultiheadAttention(256, 4)


def test_packed_mha_refuses_cpu_tensors():
    from regtr_amd.attention import PackedMultiheadAttention, packed_mha
    x = torch.zeros(8, 32, requires_grad=True)
    seg, kv = torch.tensor([0, 8], dtype=torch.int32), torch.tensor([0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        packed_mha(x, x, x, seg, kv, 8, 1)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        PackedMultiheadAttention(32, 1)(x, x, x, seg, kv, 8)
