"""GPU (-m gpu): every KPConv gather and max-pool kernel regtr_kpconv_gather / regtr_maxpool_gather can launch, against float64.

The gather is called directly (not through ops.kpconv), so the weighted neighbour features WF and the normaliser `num` are checked
themselves rather than after the contraction and the divide.  Both are views inside larger buffers: NaN inside, finite sentinel rows
around, so a branch that writes nothing, a tail workgroup or a dead lane that writes past the view, fails.  tests/dispatch.py names the
route of every case; torch.profiler confirms that the kernel the route names is the one that ran, and tests/test_dispatch_routes.py
(CPU) asserts that the cases reach every instantiation, every queries-per-wave regime of the pipelines and every group count they need."""
import functools
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import dispatch
from tests.test_gpu_dispatch import _report
from tests.util import seg_of, synth_cloud, to_dev

pytestmark = pytest.mark.gpu

SLOPE = 0.1
KP = 15
PAD = 8                 # sentinel rows before and after WF and num
SENTINEL = 7.25
U = 2.0 ** -24
CHUNK = 8192            # queries per float64 reference step


def _lib():
    from regtr_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ which kernel ran
_KERNEL_NAME = {      # route kernel -> the demangled kernel name (spaces removed) it must have launched
    'c1': 'k_kpconv_gather_c1(', 'rowsum': 'k_rowsum_positive(', 'rowsum/stats': 'k_rowsum_positive(',
    **{f'c1p<{n}>': f'k_kpconv_gather_c1p<{n}>(' for n in (2, 3, 4)},
    **{f'lq<{n}>': f'k_kpconv_gather<{n}>(' for n in (16, 32, 64)},
    **{f"mfma<{J},{V}{p}>": f"k_kpconv_gather_mfma<{J},{V},{'true' if p else 'false'}>(" for J in (10, 13, 16) for V in (2, 4)
       for p in ('', ',pre')},
    **{f'mp_buf<{n}>': f'k_maxpool_gather_buf<{n},8>(' for n in (4, 2, 1)},
    **{f'mp<{n}>': f'k_maxpool_gather<{n}>(' for n in (4, 2, 1)},
}
assert set(_KERNEL_NAME) == dispatch.GATHER_KERNELS | dispatch.MAXPOOL_KERNELS


@functools.lru_cache(maxsize=None)
def _demangle(name):
    if not name.startswith('_Z'):
        return name
    for tool in ('c++filt', 'llvm-cxxfilt', '/opt/rocm/llvm/bin/llvm-cxxfilt'):
        if shutil.which(tool):
            return subprocess.run([tool], input=name, capture_output=True, text=True, timeout=60).stdout.strip()
    return name


def _launched(fn):
    """Run fn once under torch.profiler (kernel trace only) -> (fn's result, names of the gather / max-pool / flag kernels launched)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = {_demangle(e.key).replace(' ', '') for e in prof.key_averages()}
    return res, sorted(n for n in names if 'k_kpconv' in n or 'k_maxpool' in n or 'k_rowsum' in n)


def _names(name, want):
    """name holds the kernel `want` names (its '(' may be missing where the trace drops the argument list)."""
    base, i = want[:-1], name.find(want[:-1])
    while i >= 0:
        if name[i + len(base):][:1] in ('', '('):
            return True
        i = name.find(base, i + 1)
    return False


def _assert_ran(route, names):
    want = sorted({_KERNEL_NAME[k] for k in dispatch.kernels(route)})
    got = sorted({w for w in want for n in names if _names(n, w)})
    stray = [n for n in names if not any(_names(n, w) for w in want)]
    assert got == want and not stray, f'route {route}: expected {want}, the profiler saw {names}'


# ------------------------------------------------------------------------------------------------ inputs
def _clouds(lens, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([synth_cloud(rng, n) for n in lens]).astype(np.float32).reshape(-1, 3)


def _radius(lens, H):
    """A ball holding ~0.7 H supports of the largest cloud (synth_cloud: four 2 x 2 planes), so rows are a mix of full and shadow-padded."""
    return float(np.sqrt(0.7 * H * 16.0 / (np.pi * max(lens))))


def _table(s, s_lens, q, q_lens, r, H):
    ops = _ops()
    grid = ops.CellGrid(s, seg_of(s_lens), s.shape[0], r)
    return grid.query(q, seg_of(q_lens), q.shape[0], H)


def _ops():
    from regtr_amd import ops
    return ops


def _edit_rows(idx, ns):
    """Hand-made rows at both ends of the table (indices stay in [0, ns]): a repeated index; an all-shadow row (num 1, WF 0); a shadow in
    the middle of a row with a real neighbour after it; the last support ns - 1 (query nq - 1 is that support or its neighbour), twice."""
    nq, H = idx.shape
    if H >= 2:
        idx[0, 1] = idx[0, 0]
    if nq >= 4:
        idx[nq - 2, :] = ns
        if H >= 3:
            idx[nq - 3, H // 2] = ns
            idx[nq - 3, -1] = idx[nq - 3, 0]
        idx[nq - 1, 0] = ns - 1
        if H >= 2:
            idx[nq - 1, -1] = ns - 1
    return idx


def _boxed(rows, cols, dtype=torch.float32, misalign=0):
    """(buffer, view): `rows` x `cols` NaN rows inside PAD finite sentinel rows each side; misalign shifts the view by that many floats."""
    n = (rows + 2 * PAD) * cols + misalign
    buf = torch.full((n,), SENTINEL, dtype=dtype, device='cuda')
    lo = PAD * cols + misalign
    buf[lo:lo + rows * cols] = float('nan')
    return buf, buf[lo:lo + rows * cols].view(rows, cols), lo, lo + rows * cols


def _check_boxed(buf, lo, hi, what):
    assert (buf[:lo] == SENTINEL).all() and (buf[hi:] == SENTINEL).all(), f'{what}: written outside its view'
    assert not torch.isnan(buf[lo:hi]).any(), f'{what}: {int(torch.isnan(buf[lo:hi]).sum())} elements of the view left unwritten'


# ------------------------------------------------------------------------------------------------ the call and the reference
def _gather(q, s, idx, x, kp, extent, flag=None, xyzf=None, stats=None, q_seg=None, ld_wf=0, misalign=0):
    """regtr_kpconv_gather itself, with WF and num boxed; -> (wf view, num view, check-the-boxes closure)."""
    lib = _lib()
    L = lib.lib()
    nq, H = idx.shape
    ns, Cin = x.shape
    ld = ld_wf or KP * Cin
    wbuf, wf, wlo, whi = _boxed(nq, ld, misalign=misalign)
    nbuf, num, nlo, nhi = _boxed(nq, 1)
    n_seg = stats.shape[0] if stats is not None else 0
    lib.check(L.regtr_kpconv_gather(lib.ptr(q), nq, lib.ptr(s), ns, lib.iptr(idx), H, lib.ptr(x), Cin, lib.ptr(flag), lib.ptr(xyzf),
                                    lib.ptr(kp), KP, float(extent), lib.ptr(stats), lib.iptr(q_seg) if stats is not None else None,
                                    n_seg, SLOPE, wf.data_ptr(), ld_wf, num.data_ptr(), lib.stream()), 'regtr_kpconv_gather')

    def boxes():
        _check_boxed(wbuf, wlo, whi, 'wf')
        _check_boxed(nbuf, nlo, nhi, 'num')
    return wf, num.view(nq), boxes


def _flag_pass(x, stats=None, s_seg=None):
    lib = _lib()
    ns, Cin = x.shape
    flag = torch.full((ns,), float('nan'), device='cuda')
    lib.check(lib.lib().regtr_rowsum_positive(lib.ptr(x), ns, Cin, lib.ptr(stats), lib.iptr(s_seg) if stats is not None else None,
                                              stats.shape[0] if stats is not None else 0, SLOPE, lib.ptr(flag), lib.stream()),
              'regtr_rowsum_positive')
    return flag


def _verify(wf, num, q, s, idx, x, kp, extent, stats=None, q_cloud=None, rec_flag=None):
    """WF and num against float64 (computed on the GPU, CHUNK queries at a time); -> worst err / bound.

    WF64[q,k,c] = sum_h w_hk x'_{n_h,c},  w_hk = max(1 - |s_{n_h} - q - p_k| / extent, 0), the shadow index ns a point at 1e6 with a
    zero feature, x' = x or lrelu((x - mu) rstd) with the very float32 statistics the kernel was given (the query's cloud): the check
    isolates the gather.  Bound, element by element:  |WF - WF64| <= (H + 8) 2^-24 S + 1e-6 X
      S = sum_h |w_hk| |x'_hc|: H - 1 rounded additions and one rounded product per term (a sequential or MFMA-blocked float32 sum), two
          roundings of the folded x' ((x - mu) rstd, the LeakyReLU product), the rest headroom -- (H + 8) u;
      X = sum |x'_hc| over the neighbours with 1 - d_hk / extent > -1e-6: the influence itself carries an ABSOLUTE error -- float32 offsets
          s - q - p_k (half an ulp of each difference), the squared norm, the hardware sqrt (1 ulp), the product with a rounded 1 / extent
          -- a few ulp of d / extent <= 1, < 5e-7 (the kernel comment: ~2e-7); it reaches the neighbours whose influence is near 0 too.
    num: with records (rec_flag: PRE, Cin = 1) the count of real neighbours whose record flag is set, exactly.  Otherwise the flags are
    float32 row sums: exact on every query whose real neighbours all have |sum_c x'| > 1e-5 sum_c |x'| in float64 (>= 95 % of queries);
    on the rest num may differ by at most the number of such ambiguous neighbours."""
    nq, H = idx.shape
    ns, Cin = x.shape
    ext = float(np.float32(extent))
    s_pad = torch.cat((s.double(), torch.full((1, 3), 1e6, dtype=torch.float64, device='cuda')))
    kp64 = kp.double()
    worst, n_qual = 0.0, 0
    wf_k = wf[:, :KP * Cin].reshape(nq, KP, Cin)
    for a in range(0, nq, CHUNK):
        b = min(nq, a + CHUNK)
        ic = idx[a:b].long()
        real = ic < ns
        xg = x[ic.clamp_max(ns - 1)].double()
        if stats is not None:
            st = stats[q_cloud[a:b]].double()                                   # (chunk, Cin, 2)
            t = (xg - st[:, None, :, 0]) * st[:, None, :, 1]
            xg = torch.where(t > 0, t, t * float(np.float32(SLOPE)))
        xg = xg * real[..., None]
        rel = s_pad[ic] - q[a:b, None, :].double()
        d = (rel[:, :, None, :] - kp64[None, None]).norm(dim=-1)               # (chunk, H, KP)
        t = 1.0 - d / ext
        w = t.clamp_min(0.0)
        xa = xg.abs()
        ref = torch.einsum('qhk,qhc->qkc', w, xg)
        S = torch.einsum('qhk,qhc->qkc', w, xa)
        X = torch.einsum('qhk,qhc->qkc', (t > -1e-6).double(), xa)
        bound = (H + 8) * U * S + 1e-6 * X
        err = (wf_k[a:b].double() - ref).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0))
        r = ratio.max().item()
        if r > 1:
            i = int(ratio.flatten().argmax())
            qi, rest = divmod(i, KP * Cin)
            raise AssertionError(f'WF[{a + qi}, k={rest // Cin}, c={rest % Cin}] = {wf_k[a + qi, rest // Cin, rest % Cin].item()!r}, '
                                 f'float64 {ref[qi, rest // Cin, rest % Cin].item()!r}: err / bound = {r:.3g}')
        worst = max(worst, r)
        got = num[a:b].double()
        if rec_flag is not None:
            cnt = (real & (rec_flag[ic.clamp_max(ns - 1)] > 0)).sum(1).double()
            want = cnt.clamp_min(1.0)
            bad = (got != want).nonzero()
            assert bad.numel() == 0, f'num[{a + int(bad[0])}] = {got[bad[0]].item()}, the records count {want[bad[0]].item()}'
            n_qual += b - a
        else:
            rs, ab = xg.sum(-1), xa.sum(-1)
            amb = real & (rs.abs() <= 1e-5 * ab)
            cnt = (real & (rs > 0)).sum(1).double()
            want, namb = cnt.clamp_min(1.0), amb.sum(1).double()
            qual = namb == 0
            bad = ((got != want) & qual).nonzero()
            assert bad.numel() == 0, f'num[{a + int(bad[0])}] = {got[bad[0]].item()}, float64 {want[bad[0]].item()}'
            assert ((got - want).abs() <= namb).all(), 'num off by more than the ambiguous neighbours'
            n_qual += int(qual.sum())
    assert n_qual >= 0.95 * nq, f'only {n_qual} of {nq} queries have unambiguous neighbour flags'
    return worst


def _kp(r):
    from regtr_amd.kernel_points import K015_CENTER
    return torch.tensor(K015_CENTER * r, dtype=torch.float32, device='cuda')


def _stats(n_clouds, Cin, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    mu = torch.randn((n_clouds, Cin), device='cuda', generator=g) * 0.5
    rstd = torch.rand((n_clouds, Cin), device='cuda', generator=g) * 2.7 + 0.3
    return torch.stack((mu, rstd), -1).contiguous()


def _features(ns, Cin, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn((ns, Cin), device='cuda', generator=g)


def _lens(nq):
    """Query clouds whose boundaries fall inside waves: [5, 0, 1, ~nq / 2, 7, 0, rest] (empty clouds, a one-point cloud)."""
    return [5, 0, 1, nq // 2, 7, 0, nq - nq // 2 - 13]


def _run_self(Cin, H, nq, mode, route, seed, misalign=0):
    """Queries = supports (one conv table of a level): clouds _lens(nq), CellGrid table with hand-edited rows; mode 'plain', 'stats'
    (folded InstanceNorm + LeakyReLU) or 'pre' ((x, y, z, flag) records, final features)."""
    lens = _lens(nq)
    pts = _clouds(lens, seed)
    s = to_dev(pts)
    r = _radius(lens, H)
    idx = _edit_rows(_table(s, lens, s, lens, r, H), nq)
    kp, extent = _kp(r), r * 0.8
    x = _features(nq, Cin, seed)
    stats = _stats(len(lens), Cin, seed) if mode == 'stats' else None
    seg = seg_of(lens)
    q_cloud = torch.repeat_interleave(torch.arange(len(lens), device='cuda'), torch.tensor(lens, device='cuda'))
    xyzf = rec_flag = None
    if mode == 'pre':
        rec_flag = (x.sum(1) > 0).float()
        xyzf = torch.cat((s, rec_flag[:, None]), 1).contiguous()
    flag_given = dispatch.ops_flag_pass(nq, Cin, H, x_aligned=True) or misalign % 4 != 0
    assert dispatch.route_gather(nq, nq, Cin, H, KP, flag_given, xyzf is not None, stats is not None, misalign % 4 == 0) == route

    def call():
        flag = _flag_pass(x, stats, seg) if flag_given else None
        return _gather(s, s, idx, x, kp, extent, flag=flag, xyzf=xyzf, stats=stats, q_seg=seg, misalign=misalign)
    (wf, num, boxes), names = _launched(call)
    _assert_ran(route, names)
    boxes()
    worst = _verify(wf, num, s, s, idx, x, kp, extent, stats=stats, q_cloud=q_cloud, rec_flag=rec_flag)
    _report(route, worst)


# ------------------------------------------------------------------------------------------------ the matrix-core gather
# (Cin, H, nq, mode, route): every k_kpconv_gather_mfma<J, V, PRE> at one query per wave (nq 500), four (9 233: a one-query last wave)
# and eight (30 011: a three-query last wave); J = 10 / 13 / 16 at H 33, 40 | 41, 50, 52 | 53, 64; V = 2 at Cin 32, 96 (three passes),
# V = 4 at Cin 64 ... 512.  'stats' at eight per wave on clouds [5, 0, 1, 15005, 7, 0, 14993]: boundaries inside waves, empty clouds.
MFMA_CASES = [
    (32, 33, 500, 'plain', 'mfma<10,2>/qpw1'), (96, 40, 9233, 'plain', 'mfma<10,2>/qpw4'), (96, 33, 30011, 'stats', 'mfma<10,2>/qpw8'),
    (32, 40, 500, 'pre', 'mfma<10,2,pre>/qpw1'), (32, 33, 9233, 'pre', 'mfma<10,2,pre>/qpw4'), (96, 40, 30011, 'pre', 'mfma<10,2,pre>/qpw8'),
    (64, 40, 500, 'stats', 'mfma<10,4>/qpw1'), (512, 33, 9233, 'plain', 'mfma<10,4>/qpw4'), (128, 40, 30011, 'stats', 'mfma<10,4>/qpw8'),
    (256, 33, 500, 'pre', 'mfma<10,4,pre>/qpw1'), (64, 40, 9233, 'pre', 'mfma<10,4,pre>/qpw4'), (64, 33, 30011, 'pre', 'mfma<10,4,pre>/qpw8'),
    (96, 41, 500, 'stats', 'mfma<13,2>/qpw1'), (32, 50, 9233, 'plain', 'mfma<13,2>/qpw4'), (32, 52, 30011, 'stats', 'mfma<13,2>/qpw8'),
    (96, 52, 500, 'pre', 'mfma<13,2,pre>/qpw1'), (96, 41, 9233, 'pre', 'mfma<13,2,pre>/qpw4'), (32, 50, 30011, 'pre', 'mfma<13,2,pre>/qpw8'),
    (128, 50, 500, 'plain', 'mfma<13,4>/qpw1'), (256, 52, 9233, 'stats', 'mfma<13,4>/qpw4'), (64, 41, 30011, 'stats', 'mfma<13,4>/qpw8'),
    (512, 41, 500, 'pre', 'mfma<13,4,pre>/qpw1'), (128, 52, 9233, 'pre', 'mfma<13,4,pre>/qpw4'), (256, 50, 30011, 'pre', 'mfma<13,4,pre>/qpw8'),
    (32, 64, 500, 'plain', 'mfma<16,2>/qpw1'), (96, 53, 9233, 'stats', 'mfma<16,2>/qpw4'), (96, 64, 30011, 'stats', 'mfma<16,2>/qpw8'),
    (32, 53, 500, 'pre', 'mfma<16,2,pre>/qpw1'), (96, 64, 9233, 'pre', 'mfma<16,2,pre>/qpw4'), (32, 64, 30011, 'pre', 'mfma<16,2,pre>/qpw8'),
    (256, 64, 500, 'stats', 'mfma<16,4>/qpw1'), (128, 53, 9233, 'plain', 'mfma<16,4>/qpw4'), (64, 53, 30011, 'stats', 'mfma<16,4>/qpw8'),
    (64, 64, 500, 'pre', 'mfma<16,4,pre>/qpw1'), (512, 53, 9233, 'pre', 'mfma<16,4,pre>/qpw4'), (128, 64, 30011, 'pre', 'mfma<16,4,pre>/qpw8'),
]


@pytest.mark.parametrize('Cin,H,nq,mode,route', MFMA_CASES, ids=[f'{c[4]}-{c[3]}-C{c[0]}-H{c[1]}' for c in MFMA_CASES])
def test_mfma_gather_vs_fp64(Cin, H, nq, mode, route):
    _run_self(Cin, H, nq, mode, route, seed=Cin * 1000 + H)


# ------------------------------------------------------------------------------------------------ the generic LDS-tile gather
# (Cin, H, nq, mode, misalign, route): Cin not a multiple of 32, or H > 64, or a view the matrix-core path cannot take (16-byte loads):
# the flag pass first.  H 56 at Cin 16 needs 78 848 B of dynamic LDS, H 116 163 328 B (the largest the launcher accepts); the launcher
# sets no hipFuncAttributeMaxDynamicSharedMemorySize, and on MI355X both launches run and are correct without it.
GENERIC_CASES = [
    (16, 40, 3001, 'plain', 0, 'rowsum+lq<16>'),
    (16, 40, 3001, 'stats', 0, 'rowsum/stats+lq<16>'),
    (20, 40, 3001, 'stats', 0, 'rowsum/stats+lq<32>'),
    (20, 40, 3001, 'plain', 0, 'rowsum+lq<32>'),
    (48, 40, 3001, 'plain', 0, 'rowsum+lq<64>'),
    (48, 40, 3001, 'stats', 0, 'rowsum/stats+lq<64>'),
    (16, 56, 3001, 'plain', 0, 'rowsum+lq<16>'),
    (16, 116, 3001, 'stats', 0, 'rowsum/stats+lq<16>'),
    (64, 80, 3001, 'plain', 0, 'rowsum+lq<64>'),
    (64, 80, 3001, 'stats', 0, 'rowsum/stats+lq<64>'),
    (64, 40, 3001, 'plain', 1, 'rowsum+lq<64>'),                 # WF one float into its buffer: no 16-byte stores
]


@pytest.mark.parametrize('Cin,H,nq,mode,misalign,route', GENERIC_CASES,
                         ids=[f'{c[5]}-{c[3]}-C{c[0]}-H{c[1]}' + ('-unaligned' if c[4] else '') for c in GENERIC_CASES])
def test_generic_gather_vs_fp64(Cin, H, nq, mode, misalign, route):
    _run_self(Cin, H, nq, mode, route, seed=Cin * 1000 + H + misalign, misalign=misalign)


def test_generic_gather_refuses_lds_over_160k():
    """H 117 at Cin 16 would need 164 736 B of LDS: refused on the host, before any launch (real, in-contract operands)."""
    nq, H, Cin = 64, 117, 16
    assert dispatch.generic_lds(Cin, H)[1] > dispatch.LDS_LIMIT >= dispatch.generic_lds(Cin, H - 1)[1]
    assert dispatch.route_gather(nq, nq, Cin, H, KP, True) == 'refused'
    s = to_dev(_clouds([nq], 3))
    idx = torch.full((nq, H), nq, dtype=torch.int32, device='cuda')
    x = _features(nq, Cin, 3)
    flag = _flag_pass(x)
    with pytest.raises(RuntimeError, match='regtr_kpconv_gather: invalid argument'):
        _gather(s, s, idx, x, _kp(0.1), 0.08, flag=flag)


# ------------------------------------------------------------------------------------------------ Cin = 1 (first block)
# (H, nq, mode, route): mode 'derived' (flag from the feature), 'flag' (a flag pass), 'records' ((x, y, z, feature) records).  The
# pipelined kernel at 2 groups per wave (nq 40 000) and at 8 (250 000); its NS = 2 / 3 / 4 element slots at H 32 | 33 (odd: a pad slot), 40 |
# 49, 64.  Every case runs with ld_wf = KP and with ld_wf = 16 (the first-block form: a zero pad column).
C1_CASES = [
    (40, 500, 'derived', 'c1'),
    (33, 3001, 'derived', 'c1'),
    (40, 500, 'flag', 'rowsum+c1'),
    (33, 20000, 'records', 'c1'),
    (32, 40000, 'records', 'c1p<2>/g2'),
    (32, 250000, 'records', 'c1p<2>/g8'),
    (33, 40000, 'records', 'c1p<3>/g2'),
    (40, 250000, 'records', 'c1p<3>/g8'),
    (49, 40000, 'records', 'c1p<4>/g2'),
    (64, 250000, 'records', 'c1p<4>/g8'),
]


@pytest.mark.parametrize('H,nq,mode,route', C1_CASES, ids=[f'{c[3]}-{c[2]}-H{c[0]}-n{c[1]}' for c in C1_CASES])
def test_c1_gather_vs_fp64(H, nq, mode, route):
    lens = _lens(nq)
    s = to_dev(_clouds(lens, H + nq))
    r = _radius(lens, H)
    idx = _edit_rows(_table(s, lens, s, lens, r, H), nq)
    kp, extent = _kp(r), r * 0.8
    x = _features(nq, 1, H + nq)
    xyzf = torch.cat((s, x), 1).contiguous() if mode == 'records' else None
    assert dispatch.route_gather(nq, nq, 1, H, KP, mode == 'flag', xyzf is not None) == route
    for ld_wf in (16, 0):
        def call():
            flag = _flag_pass(x) if mode == 'flag' else None
            return _gather(s, s, idx, x, kp, extent, flag=flag, xyzf=xyzf, ld_wf=ld_wf)
        if ld_wf == 16:
            (wf, num, boxes), names = _launched(call)
            _assert_ran(route, names)
        else:
            wf, num, boxes = call()
        boxes()
        if ld_wf == 16:
            assert (wf[:, KP:] == 0).all() and not torch.signbit(wf[:, KP:]).any(), 'the pad column of a 16-float row must be +0'
        worst = _verify(wf, num, s, s, idx, x, kp, extent, rec_flag=(x[:, 0] > 0).float())
        _report(route + ('/ld16' if ld_wf == 16 else ''), worst)


# ------------------------------------------------------------------------------------------------ the matrix-core -> generic hand-off
HANDOFF_CASES = [(2_097_151, 'mfma<10,4>/qpw2'), (2_097_152, 'rowsum+lq<64>')]      # ns * Cin just below / at 2^29 (2 GiB of rows)


@pytest.mark.parametrize('ns,route', HANDOFF_CASES, ids=[c[1] for c in HANDOFF_CASES])
def test_gather_handoff_at_2_29_feature_elements(ns, route):
    """Cin 256: ns * Cin = 2^29 - 256 stays on the matrix-core kernel (range-checked buffer offsets up to 2 GiB - 1 KiB), 2^29 goes to the
    generic kernel with a flag pass.  4 096 queries: the last supports of the table, neighbours up to ns - 1."""
    Cin, H, nq = 256, 40, 4096
    pts = _clouds([ns], 17)
    s = to_dev(pts)
    q = s[ns - nq:].contiguous()
    r = _radius([ns], H)
    idx = _edit_rows(_table(s, [ns], q, [nq], r, H), ns)
    kp, extent = _kp(r), r * 0.8
    x = _features(ns, Cin, 17)
    flag_given = dispatch.ops_flag_pass(ns, Cin, H)
    assert dispatch.route_gather(nq, ns, Cin, H, KP, flag_given) == route
    try:
        def call():
            flag = _flag_pass(x) if flag_given else None
            return _gather(q, s, idx, x, kp, extent, flag=flag)
        (wf, num, boxes), names = _launched(call)
        _assert_ran(route, names)
        boxes()
        assert (idx == ns - 1).any()
        worst = _verify(wf, num, q, s, idx, x, kp, extent)
        _report(route + '/2GiB', worst)
    finally:
        del x
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ max-pool
@pytest.mark.parametrize('C', [4, 60, 64, 68, 128, 132, 256, 1024])
def test_maxpool_vs_ref(C):
    """k_maxpool_gather_buf<QW, 8> against regtr_ref.max_pool, bit for bit: H 1, 7, 8, 9 (one batch of 8 rows and a partial one), 40, 50;
    3 001 queries (not a multiple of any wave's 4 / 2 / 1); hand-edited rows; a `width` below the table's, whose hidden columns point at
    a row that would change every maximum."""
    from oracle import regtr_ref
    ops = _ops()
    nq = 3001
    route = dispatch.route_maxpool(nq, C)
    assert route == f"mp_buf<{4 if C <= 64 else 2 if C <= 128 else 1}>"
    s = to_dev(_clouds([nq], C))
    x = _features(nq, C, C)
    x[17] = 1e3                                                                 # the row the hidden columns point at
    for n, H in enumerate((1, 7, 8, 9, 40, 50)):
        idx = _edit_rows(_table(s, [nq], s, [nq], _radius([nq], H), H), nq)
        if n == 0:
            out, names = _launched(lambda: ops.maxpool(x, idx))
            _assert_ran(route, names)
        else:
            out = ops.maxpool(x, idx)
        assert torch.equal(out, regtr_ref.max_pool(x, idx.long())), (C, H)
        if H >= 7:
            width = H - 3
            idx[:, width:] = 17
            out = ops.maxpool(x, idx, width=width)
            ref = regtr_ref.max_pool(x, idx[:, :width].long())
            assert torch.equal(out, ref), (C, H, width)
            assert not torch.equal(ref, regtr_ref.max_pool(x, idx.long()))


MAXPOOL_4GIB = [(64, 16_777_216), (128, 8_388_608), (256, 4_194_304)]


@pytest.mark.parametrize('C,ns', MAXPOOL_4GIB, ids=[f'C{c[0]}' for c in MAXPOOL_4GIB])
def test_maxpool_predicated_at_4_gib(C, ns):
    """Tables of exactly 4 GiB do not fit the branch-free kernel's 32-bit offsets: the predicated k_maxpool_gather<QW>, bit for bit
    against the reference's max over the listed rows and a zero shadow row; 4 096 queries over the whole table, ns - 1 and ns included."""
    assert ns * C * 4 == 1 << 32
    route = dispatch.route_maxpool(ns, C)
    assert route == f"mp<{4 if C <= 64 else 2 if C <= 128 else 1}>"
    ops = _ops()
    nq, H = 4096, 40
    g = torch.Generator(device='cuda').manual_seed(C)
    try:
        x = torch.randn((ns, C), device='cuda', generator=g)
        idx = torch.randint(0, ns + 1, (nq, H), device='cuda', generator=g, dtype=torch.int32)
        idx[:, -2:] = ns
        idx[0, :] = ns - 1
        idx[1, :] = ns
        idx[2, ::2] = ns - 1
        out, names = _launched(lambda: ops.maxpool(x, idx))
        _assert_ran(route, names)
        ic = idx.long()
        v = x[ic.clamp_max(ns - 1)]
        v[ic == ns] = 0.0
        assert torch.equal(out, v.amax(1))
        assert float(out[1].abs().max()) == 0.0 and torch.equal(out[0], x[ns - 1])
    finally:
        x = None
        torch.cuda.empty_cache()
