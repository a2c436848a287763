"""CPU: the bounds of tests/test_gpu_pose.py are loose enough for an honest float32 evaluation and tight enough to catch a subtly wrong
kernel.

For every coordinate-attention case: a float32 online softmax over 32-key tiles (the kernel's order of operations, on the CPU) stays
within the per-row bound; a float64 evaluation that drops the most-attended key of each partner cloud's last (partial) tile, or that reads
keys and coordinates from the query cloud instead of its partner, moves some row by more than 10x its bound.  For the pose: the float64
reference returns R = I and t = c_b - c_a for a zero covariance, and the pose bound catches a pose solved without one point."""
import math

import pytest
import torch

from tests import test_gpu_pose as gp


def attn_f32(q, k, xyz, lens, kv, TK=32):
    """float32 flash-style evaluation: scores of q * float32(1 / sqrt(D)), running max / sum rescaled per 32-key tile, o / l at the end."""
    L, N, D = q.shape
    seg = gp._seg(lens)
    scale = torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32)
    out = torch.zeros(L, N, 3)
    for c, kc in enumerate(kv):
        nq, nk = lens[c], lens[kc]
        if nq == 0 or nk == 0:
            continue
        qs = q[:, seg[c]:seg[c + 1]] * scale
        m = torch.full((L, nq, 1), -math.inf)
        lsum = torch.zeros(L, nq, 1)
        o = torch.zeros(L, nq, 3)
        for t in range(0, nk, TK):
            rows = slice(seg[kc] + t, seg[kc] + min(t + TK, nk))
            s = qs @ k[:, rows].transpose(1, 2)
            m_new = torch.maximum(m, s.amax(-1, keepdim=True))
            alpha = torch.exp(m - m_new)
            p = torch.exp(s - m_new)
            lsum = lsum * alpha + p.sum(-1, keepdim=True)
            o = o * alpha + p @ xyz[rows]
            m = m_new
        out[:, seg[c]:seg[c + 1]] = o / lsum
    return out


def _live_ratio(out, ref, bound, lens, kv):
    seg = gp._seg(lens)
    live = torch.zeros(out.shape[1], dtype=torch.bool)
    for c, kc in enumerate(kv):
        if lens[kc]:
            live[seg[c]:seg[c + 1]] = True
    return ((out.double() - ref).abs().amax(-1)[:, live] / bound[:, live]).max().item()


@pytest.mark.parametrize('name,head_dim,lens,kv,layers,kind,route', gp.ATTN_CASES, ids=gp.ATTN_IDS)
def test_attn_bound_is_sharp(name, head_dim, lens, kv, layers, kind, route):
    q, k, xyz = gp.attn_case(name, head_dim, lens, kv, layers, kind)
    ref = gp.attn_ref(q, k, xyz, lens, kv)
    bound = gp.attn_bound(q, k, xyz, lens, kv, ref)
    honest = gp.attn_ratio(attn_f32(q, k, xyz, lens, kv), ref, bound, lens, kv)
    dropped, wrong = gp.attn_defects(q, k, xyz, lens, kv, ref)
    r_drop = _live_ratio(dropped, ref, bound, lens, kv)
    r_wrong = _live_ratio(wrong, ref, bound, lens, kv) if wrong is not None else math.inf
    print(f'attn_xyz {name}: float32 err/bound {honest:.3f}; one key dropped {r_drop:.3g}, wrong cloud {r_wrong:.3g}')
    assert honest <= 0.5, 'the bound is too tight for a float32 evaluation'
    assert r_drop > 10 and r_wrong > 10


def test_zero_covariance_reference_is_identity():
    """torch.linalg.svd of a zero matrix returns U = V = I: the reference's pose for one point / zero weights is R = I, t = c_b - c_a."""
    a = torch.tensor([[1.0, 2.0, 3.0]])
    b = torch.tensor([[-1.0, 0.5, 4.0]])
    for w in (torch.tensor([0.3]), torch.tensor([0.0])):
        T, _, _ = gp.kabsch64(a, b, w)
        assert torch.equal(T[:, :3], torch.eye(3, dtype=torch.float64))
        assert torch.allclose(T[:, 3], (b - a).double() if w.item() else torch.zeros(3, dtype=torch.float64))


def test_pose_bound_catches_a_missing_point():
    """A pose solved without one of 257 points (a kernel whose stride loop skips the row past 256) fails the pose bound by 10x."""
    g = torch.Generator().manual_seed(5)
    a = (torch.rand(257, 3, generator=g) - 0.5) * 2
    b = gp._motion(a, gp.rot([0.4, 0.1, -0.3], 0.9), [0.1, 0.2, 0.3], 0.02, g)
    w = torch.sigmoid(torch.randn(257, generator=g).double())
    T, kappa, scale = gp.kabsch64(a, b, w)
    assert gp.pose_ratio(T.float(), T, kappa, scale) <= 0.5
    T_miss, _, _ = gp.kabsch64(a[:256], b[:256], w[:256])
    r = gp.pose_ratio(T_miss.float(), T, kappa, scale)
    print(f'pose bound, one of 257 points missing: err/bound {r:.3g}')
    assert r > 10
