"""GPU (-m gpu): the per-query neighbour-group count of the KPConv gathers -- the skip path against the full path of the same build.

k_kpconv_gather_mfma runs a query through a body compiled for the groups up to its highest real slot, and the Cin = 1 kernels stop their
pair walk at the last pair that holds a real neighbour of any of a wave's four queries.  A skipped slot is a shadow: influence +0 times a
finite feature, added to an accumulator that starts at +0 and so is never -0 -- the identity.  The check is therefore BIT EQUALITY of one
neighbourhood built twice:
  shadow form    shadows written as index == ns (what the tables hold): queries run their own group count;
  sentinel form  ns + 1 supports, the extra one at (1e6, 1e6, 1e6) with zero features and flag 0, every shadow slot pointing at it: no
                 slot is a shadow, every query runs all J groups / all pairs.
The arithmetic is the same statement for statement (a shadow is placed at 1e6 before the query is subtracted, either way).  The
normaliser must not count the sentinel: its record flag is 0 (PRE, Cin = 1), its zero feature is not > 0 (Cin = 1 without records), and
in the folded form the statistics have positive means, so its row lrelu((0 - mean) rstd) sums to a negative number.  The same index
table serves both forms (index ns is the shadow of one and the sentinel support of the other).  The full-J body itself is held to
float64 by tests/test_gpu_gather.py.

Rows of one launch (tiled to nq; the period is odd, so the patterns meet every position of a wave's queries):
  * 4-query groups with different counts, an all-shadow group and an all-small group (Cin = 1: the bound is per group);
  * the last real slot at every value 0 ... H (a row with no real neighbour, a full row);
  * a shadow in the middle of a full row, and a row whose only real slots are the first and the last: nothing may be skipped;
  * neighbouring queries alternating between the smallest and the largest count (0 | H and 1 | H): the software pipeline crosses bodies
    on every iteration.
nq is never a multiple of the queries per wave, so the prefetch clamps at the end.  WF and num sit inside sentinel rows."""
import numpy as np
import pytest
import torch

from tests import dispatch
from tests.util import seg_of

pytestmark = pytest.mark.gpu

KP = 15
SLOPE = 0.1
PAD = 8
SENTINEL = 7.25
NS = 301
R = 0.1                 # kernel-point radius; supports and queries fill a 0.12 cube, so most influences are non-zero
EXTENT = 0.08


def _lib():
    from regtr_amd import _lib
    return _lib


def _last_real(H):
    """Per row: (number of leading real slots L, kind) -- kind 0 plain prefix, 1 full row with a shadow in the middle, 2 only the first
    and the last slot real."""
    groups = [(0, H, 3, H // 2), (2, 2, 2, 2), (0, 0, 0, 0), (1, 1, 1, H), (H, H - 1, 5, 4), (H - 3, 1, 0, 9)]
    rows = [(L, 0) for g in groups for L in g]
    rows += [(L, 0) for L in range(H + 1)]
    rows += [(H, 1), (H, 2), (H, 1)]
    rows += [(L, 0) for _ in range(8) for L in (0, H)]
    rows += [(L, 0) for _ in range(8) for L in (1, H)]
    if len(rows) % 2 == 0:
        rows.append((H // 3, 0))
    return rows


def _neighbourhood(H, nq, seed):
    """-> (q, s, idx int32 (nq, H) with shadows == NS, rows) on the GPU."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 0.12, (NS, 3)).astype(np.float32)
    q = rng.uniform(0, 0.12, (nq, 3)).astype(np.float32)
    pat = _last_real(H)
    L = np.array([pat[i % len(pat)][0] for i in range(nq)])
    kind = np.array([pat[i % len(pat)][1] for i in range(nq)])
    idx = rng.integers(0, NS, (nq, H)).astype(np.int32)
    idx[np.arange(H)[None, :] >= L[:, None]] = NS
    idx[kind == 1, H // 2] = NS
    idx[kind == 2, 1:H - 1] = NS
    return torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda(), torch.from_numpy(idx).cuda(), L, kind


def _boxed(rows, cols):
    buf = torch.full(((rows + 2 * PAD) * cols,), SENTINEL, device='cuda')
    lo, hi = PAD * cols, (PAD + rows) * cols
    buf[lo:hi] = float('nan')
    return buf, buf[lo:hi].view(rows, cols), lo, hi


def _gather(q, s, ns, idx, x, kp, xyzf=None, stats=None, q_seg=None, ld_wf=0):
    """regtr_kpconv_gather with WF and num inside sentinel rows -> (wf, num), both checked: written everywhere, nothing outside."""
    lib = _lib()
    nq, H = idx.shape
    Cin = x.shape[1]
    wbuf, wf, wlo, whi = _boxed(nq, ld_wf or KP * Cin)
    nbuf, num, nlo, nhi = _boxed(nq, 1)
    lib.check(lib.lib().regtr_kpconv_gather(lib.ptr(q), nq, lib.ptr(s), ns, lib.iptr(idx), H, lib.ptr(x), Cin, None, lib.ptr(xyzf),
                                            lib.ptr(kp), KP, EXTENT, lib.ptr(stats), lib.iptr(q_seg) if stats is not None else None,
                                            stats.shape[0] if stats is not None else 0, SLOPE, wf.data_ptr(), ld_wf, num.data_ptr(),
                                            lib.stream()), 'regtr_kpconv_gather')
    torch.cuda.synchronize()
    for what, buf, lo, hi in (('wf', wbuf, wlo, whi), ('num', nbuf, nlo, nhi)):
        assert (buf[:lo] == SENTINEL).all() and (buf[hi:] == SENTINEL).all(), f'{what}: written outside its view'
        assert not torch.isnan(buf[lo:hi]).any(), f'{what}: elements of the view left unwritten'
    return wf, num.view(nq)


def _kp():
    from regtr_amd.kernel_points import K015_CENTER
    return torch.tensor(K015_CENTER * R, dtype=torch.float32, device='cuda')


def _twin(H, nq, Cin, form, seed, ld_wf=0):
    """Both forms of one neighbourhood -> (wf, num) of the shadow form, after the bit-equality asserts; form: 'pre' ((x, y, z, flag)
    records, final features), 'stats' (folded InstanceNorm + LeakyReLU), 'records' (Cin = 1: (x, y, z, feature)), 'derived' (Cin = 1:
    coordinates and features apart, the flag from the feature)."""
    q, s, idx, L, kind = _neighbourhood(H, nq, seed)
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn((NS, Cin), device='cuda', generator=g)
    far = torch.full((1, 3), 1e6, device='cuda')
    s1, x1 = torch.cat((s, far)).contiguous(), torch.cat((x, torch.zeros((1, Cin), device='cuda'))).contiguous()
    kw0, kw1 = {}, {}
    if form in ('pre', 'records'):
        last = (x.sum(1, keepdim=True) > 0).float() if form == 'pre' else x
        kw0['xyzf'] = torch.cat((s, last), 1).contiguous()
        kw1['xyzf'] = torch.cat((kw0['xyzf'], torch.tensor([[1e6, 1e6, 1e6, 0.0]], device='cuda'))).contiguous()
    elif form == 'stats':
        lens = [5, 0, 1, nq // 2, 7, 0, nq - nq // 2 - 13]                       # cloud boundaries inside waves, empty clouds
        mu = torch.rand((len(lens), Cin), device='cuda', generator=g) * 0.5 + 0.05      # positive: the sentinel's folded row sums < 0
        rstd = torch.rand((len(lens), Cin), device='cuda', generator=g) * 2.7 + 0.3
        kw0['stats'] = kw1['stats'] = torch.stack((mu, rstd), -1).contiguous()
        kw0['q_seg'] = kw1['q_seg'] = seg_of(lens)
    kp = _kp()
    wf0, num0 = _gather(q, s, NS, idx, x, kp, ld_wf=ld_wf, **kw0)
    wf1, num1 = _gather(q, s1, NS + 1, idx, x1, kp, ld_wf=ld_wf, **kw1)
    # bit patterns, not values: a -0 where the full path gives +0 would be a difference too
    assert torch.equal(wf0.view(torch.int32), wf1.view(torch.int32)), \
        f'WF differs on {int((wf0.view(torch.int32) != wf1.view(torch.int32)).any(1).sum())} of {nq} queries'
    assert torch.equal(num0, num1), f'num differs on {int((num0 != num1).sum())} of {nq} queries'
    empty = torch.from_numpy(L == 0).cuda()
    assert empty.any() and (wf0[empty] == 0).all() and (num0[empty] == 1).all(), 'a row with no real neighbour: WF 0, num 1'
    full = torch.from_numpy((L == H) & (kind == 0)).cuda()
    assert (wf0[full].abs().amax(1) > 0).all(), 'full rows must have gathered something'
    return wf0, num0


# (H, J): J = 10; J = 10 with two dead lanes in the last group; 13; 16
H_CASES = [40, 38, 50, 64]
# Cin 32: V = 2; 64: V = 4, one pass; 128: V = 4, two passes.  nq 331: one query per wave; 9 235: four (a three-query last wave);
# 21 511 (Cin 32 only): eight (a seven-query last wave)
MFMA_CASES = [(H, Cin, form, nq) for H in H_CASES for Cin in (32, 64, 128) for form in ('pre', 'stats')
              for nq in ((331, 9235, 21511) if Cin == 32 else (331, 9235))]


@pytest.mark.parametrize('H,Cin,form,nq', MFMA_CASES, ids=[f'H{c[0]}-C{c[1]}-{c[2]}-n{c[3]}' for c in MFMA_CASES])
def test_mfma_skip_path_equals_full_path(H, Cin, form, nq):
    J = 10 if H <= 40 else (13 if H <= 52 else 16)
    V = 4 if Cin % 64 == 0 else 2
    qpw = {331: 1, 9235: 4, 21511: 8}[nq]
    for ns in (NS, NS + 1):
        assert dispatch.route_gather(nq, ns, Cin, H, KP, False, form == 'pre', form == 'stats') == \
            f"mfma<{J},{V}{',pre' if form == 'pre' else ''}>/qpw{qpw}"
    assert nq % qpw != 0 or qpw == 1
    _twin(H, nq, Cin, form, seed=H * 1000 + Cin + nq)


# Cin = 1: k_kpconv_gather_c1 (331 queries; with records and without) and the pipelined k_kpconv_gather_c1p<NS> (33 001 queries: two
# 4-query groups per wave, a one-query last group), ld_wf = 16 (the first block's form) and KP
C1_CASES = [(H, form, nq, ld) for H in H_CASES for form, nq, ld in (('records', 331, 16), ('derived', 331, 0), ('records', 33001, 16))]


@pytest.mark.parametrize('H,form,nq,ld_wf', C1_CASES, ids=[f'H{c[0]}-{c[1]}-n{c[2]}' for c in C1_CASES])
def test_c1_skip_path_equals_full_path(H, form, nq, ld_wf):
    route = dispatch.route_gather(nq, NS, 1, H, KP, False, form == 'records', False, ld_wf=ld_wf)
    assert route == ('c1' if nq == 331 else f'c1p<{3 if H <= 48 else 4}>/g2') and nq % 4 != 0
    wf, _ = _twin(H, nq, 1, form, seed=H * 1000 + nq, ld_wf=ld_wf)
    if ld_wf == 16:
        assert (wf[:, KP:] == 0).all()
