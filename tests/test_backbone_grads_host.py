"""CPU: the float64 yardstick of the backbone's gradients (tests/backbone_grads_ref.py) against float64 finite differences on a tiny
encoder, its `sides` hand-over, the seeded block cases' promised properties, and the refusals of the differentiable blocks that are
decided on the host (nothing launched)."""
import numpy as np
import pytest
import torch

from tests import backbone_grads_ref as BR
from tests.util import load_cfg


def test_restatement_against_finite_differences():
    """Central differences in float64 with the LeakyReLU sides, pool winners and neighbour counts FIXED to the base point's (the function
    the restatement differentiates); h = 1e-6 on O(1) weights: truncation ~1e-12, rounding ~1e-10 -- the bar is 1e-6 of the largest
    gradient entry, four orders below the 1e-4 the GPU is held to against this yardstick."""
    blocks, meta, x, d_out = BR.tiny_encoder_case()
    base = BR.run(blocks, x, meta, d_out)
    assert base['out'].shape == d_out.shape and np.isfinite(base['out']).all()
    assert base['margin'] > 1e-5, 'a choice of the tiny case sits on its boundary: draw another seed'
    sides = base['sides']
    again = BR.run(blocks, x, meta, d_out, sides=sides)
    assert np.array_equal(again['out'], base['out']) and all(np.array_equal(again['grads'][k], g) for k, g in base['grads'].items())
    f = lambda bl: float((BR.run(bl, x, meta, d_out, sides=sides, backward=False)['out'] * d_out.astype(np.float64)).sum())
    rng = np.random.default_rng(5)
    h = 1e-6
    assert len(base['grads']) == 1 + 4 + 3 + 4
    for (bi, name), g in base['grads'].items():
        assert np.abs(g).max() > 0, (bi, name)
        for _ in range(2):
            at = tuple(int(rng.integers(0, s)) for s in g.shape)
            vals = []
            for sgn in (1, -1):
                bl = [dict(b) for b in blocks]
                w = bl[bi][name].astype(np.float64)
                w[at] += sgn * h
                bl[bi][name] = w
                vals.append(f(bl))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[at]) <= 1e-6 * np.abs(g).max(), (bi, name, at, fd, g[at])


def test_given_sides_are_used():
    """Flipping one LeakyReLU side, one pool winner or one row flag changes the restatement's result: the hand-over is live."""
    blocks, meta, x, d_out = BR.tiny_encoder_case()
    base = BR.run(blocks, x, meta, d_out)
    for bi, kind in ((0, 'masks'), (2, 'winners'), (1, 'pos')):
        sides = [dict((k, [a.copy() for a in v]) for k, v in s.items()) for s in base['sides']]
        a = sides[bi][kind][0]
        if kind == 'winners':
            a[0, 0] = (a[0, 0] + 1) % meta['pool_width'][0]
        else:
            a.reshape(-1)[0] = ~a.reshape(-1)[0]
        assert not np.array_equal(BR.run(blocks, x, meta, d_out, sides=sides)['out'], base['out']), kind


@pytest.mark.parametrize('name', list(BR.CASES))
def test_block_cases_hold_what_they_promise(name):
    blk, meta, x, d_out, c = BR.draw_case(name)
    assert meta['lens'][0][:3] == [1, 0, 5] and 100 <= meta['lens'][0][3] <= 999 and x.shape[0] == sum(meta['lens'][0])
    if c['kind'] == 'unary':
        return
    n = x.shape[0]
    if c.get('strided'):
        pool, w = meta['pools'][0], meta['pool_width'][0]
        assert w < pool.shape[1] == c['H'] and (pool[:, :w] >= n).all(1).any()
        assert (np.bincount(pool[pool < n], minlength=n) == 0).any(), 'an in-degree-0 support'
        assert d_out.shape[0] == meta['points'][1].shape[0] < n
    r = BR.run([blk], x, meta, d_out, x_grad=c['Cin'] > 1)
    assert np.isfinite(r['out']).all() and all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in r['grads'].values())


def test_refusals_decided_on_the_host():
    from regtr_amd import kpconv as K
    cfg = load_cfg('3dmatch')
    simple = K.SimpleBlock('simple', 1, 64, 0.0625, 0, cfg)
    resnet = K.ResnetBottleneckBlock('resnetb', 64, 128, 0.0625, 0, cfg)
    unary = K.UnaryBlock(64, 32, True, 0.02)
    meta = {'points': [torch.zeros(4, 3)], '_neighbors_i32': [torch.zeros((4, 3), dtype=torch.int32)], '_pools_i32': [None], '_pool_width': [3],
            '_seg_off': [torch.tensor([0, 4], dtype=torch.int32)], '_lens_host': [[4]]}
    with pytest.raises(RuntimeError, match='GPU tensor'):
        unary.forward_grad(torch.zeros(4, 64), meta['_seg_off'][0], 4)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        simple.forward_grad(torch.ones(4, 1), meta)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        resnet.forward_grad(torch.zeros(4, 64), meta)
    enc = K.KPFEncoder(cfg, cfg.d_embed)
    with pytest.raises(RuntimeError, match='GPU tensor'):
        enc.forward_grad(torch.ones(4, 1), meta)
    assert all(not b.KPConv.kernel_points.requires_grad for b in enc.encoder_blocks)
    # deformable blocks and use_batch_norm: false never get as far as a forward_grad
    with pytest.raises(NotImplementedError):
        K.SimpleBlock('simple_deformable', 1, 64, 0.0625, 0, cfg)
    with pytest.raises(NotImplementedError):
        K.ResnetBottleneckBlock('resnetb_deformable', 64, 128, 0.0625, 0, cfg)
    no_bn = load_cfg('3dmatch')
    no_bn.use_batch_norm = False
    with pytest.raises(NotImplementedError):
        K.SimpleBlock('simple', 1, 64, 0.0625, 0, no_bn)
    with pytest.raises(NotImplementedError):
        K.UnaryBlock(64, 32, False, 0.02)


def test_linear_bwd_picks_the_transposed_gemm_by_width(monkeypatch):
    """dW through ops.gemm_tn where both widths are multiples of 64 -- what every caller before the backbone launched -- else gemm_tn_any."""
    from regtr_amd import ops, transformer_grad
    calls = []
    monkeypatch.setattr(ops, 'gemm_tn', lambda g, a: calls.append('tn') or None)
    monkeypatch.setattr(ops, 'gemm_tn_any', lambda g, a: calls.append('any') or None)
    for n, k in ((64, 128), (256, 256), (32, 64), (128, 32), (96, 64)):
        transformer_grad.linear_bwd(torch.zeros(3, k), None, None, None, torch.zeros(3, n), None, (False, True, False))
    assert calls == ['tn', 'tn', 'any', 'any', 'any']
