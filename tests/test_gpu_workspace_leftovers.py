"""GPU (-m gpu): no launcher depends on what its workspace held before the call, and none writes outside the bytes its size query names.

Every workspace of the library is handed out by regtr_amd.ops._ws.  Here that one function is replaced (tests/workspace_poison.py) by an
allocator that serves the middle of a larger buffer -- sentinel guard bands on both sides -- pre-filled with 0x00, 0xFF (NaN / -1), 0x7F
(a large finite float / a large positive integer) or seeded random bytes.  A case runs its wrapper once without the hook and once per
fill: every output must be the same BITS every time, every guard band must be intact, and a request of exactly the named size query's
byte count (> 0) must have been served, so a case cannot pass by never reaching the workspace path.  No tolerance anywhere.

CASES is keyed by the name of the size query (every `regtr_*_ws_bytes` / `*_scratch_bytes` of regtr_amd._lib's two signature tables,
plus the two typed scratch buffers without a query: the GEMM statistics partials and the optimiser partials);
tests/test_workspace_cases_host.py fails when a query has no case.  The shapes are the smallest at which the launchers' bookkeeping has
something to get wrong: a zero-length cloud, a cloud with fewer chunks than the launch has, a short last split, a row tile that holds
no row of some cloud, an ICP pair that is done at iteration 0.  docs/KERNELS.md ("What every workspace word is written by") has the
write / read table these cases rest on; docs/PARITY.md ("Workspace leftovers") the results.

The whole-model test repeats the property over forward, training_step + backward, one FusedAdamW step, validation_step and refine_pose
of the cut-down model on the two-pair golden crop: a workspace-carrying call the table misses, or wiring that hands one workspace to two
consumers, shows there."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests.workspace_poison import FILLS, PoisonedWorkspaces

pytestmark = pytest.mark.gpu

F32 = np.float32
PARTIALS = ('gemm_stats_partial', 'optim_partials')          # typed scratch served as a view of a _ws buffer; no size query
# size queries whose launchers tests/test_gpu_preprocess_routes.py holds to the same property (0x00, 0xFF, a larger build's leftovers)
COVERED_ELSEWHERE = {
    'regtr_grid_subsample_ws_bytes': 'tests/test_gpu_preprocess_routes.py::test_subsample_ignores_workspace_leftovers',
    'regtr_grid_subsample_ordered_ws_bytes': 'tests/test_gpu_preprocess_routes.py::test_subsample_ignores_workspace_leftovers',
    'regtr_cellgrid_ws_bytes': 'tests/test_gpu_preprocess_routes.py::test_cellgrid_ignores_workspace_leftovers',
}
CASES = {}                                                   # size query -> {case name: builder}
RANDOM_SEED = 20240


def case(*queries, name=None, args=()):
    """Registers a builder (called with `args`) under its size queries.  A builder returns (run, expect): run() -> list of output
    tensors; expect: a list of (query, args) -- the query's arguments, or the byte count itself for PARTIALS, or None where the arguments
    are tables only the wrapper builds (the two C-side orchestrators): the query is then watched and what it returned is what must have
    been served."""
    def reg(fn):
        for q in queries:
            CASES.setdefault(q, {})[name or fn.__name__] = functools.partial(fn, *args)
        return fn
    return reg


# ------------------------------------------------------------------------------------------------ the harness
def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _randn(shape, seed, scale=1.0, shift=0.0):
    """N(shift, scale) float32 drawn on the device (the large cases; the same bits on every call of one seed)."""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    return torch.randn(shape, generator=gen, device='cuda', dtype=torch.float32) * scale + shift


def _seg(lens):
    return _dev(np.concatenate([[0], np.cumsum(lens)]), torch.int32)


def _library(query):
    from regtr_amd import _lib
    return _lib.parity_lib() if query in _lib.PARITY_SIGNATURES else _lib.lib()


@contextlib.contextmanager
def _watch(query):
    """Records what every call of a size query returns."""
    L = _library(query)
    orig, seen = getattr(L, query), []

    def spy(*args):
        seen.append(int(orig(*args)))
        return seen[-1]
    setattr(L, query, spy)
    try:
        yield seen
    finally:
        setattr(L, query, orig)


def _bits(t):
    t = t.detach().contiguous()
    return t.reshape(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def _snapshot(outs):
    assert outs and all(isinstance(t, torch.Tensor) for t in outs)
    return [t.detach().clone() for t in outs]


def _assert_same(want, got, what):
    assert len(want) == len(got), what
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, i, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        if not torch.equal(_bits(a), _bits(b)):
            diff = int((_bits(a) != _bits(b)).sum())
            raise AssertionError(f'{what}: output {i} {tuple(a.shape)} {a.dtype} differs in {diff} bytes')


def _expected_bytes(expect):
    out = []
    for q, spec in expect:
        if spec is None:
            continue
        nb = int(spec) if q in PARTIALS else int(getattr(_library(q), q)(*spec))
        out.append((q, nb))
    return out


def _run_under_fills(run, expect, fills, what):
    want = _expected_bytes(expect)
    watched = [q for q, spec in expect if spec is None]
    assert all(nb > 0 for _, nb in want), (what, want)
    base = _snapshot(run())
    torch.cuda.synchronize()
    for fill in fills:
        with contextlib.ExitStack() as stack:
            seen = {q: stack.enter_context(_watch(q)) for q in watched}
            hook = stack.enter_context(PoisonedWorkspaces(fill, seed=RANDOM_SEED))
            got = _snapshot(run())
        torch.cuda.synchronize()
        n_req = hook.check()
        for q, nb in want + [(q, nb) for q in watched for nb in seen[q]]:
            assert nb > 0 and hook.served(nb) >= 1, f'{what}, fill {fill}: no workspace of {q} = {nb} bytes among {sorted(set(hook.sizes()))}'
        assert all(seen[q] for q in watched), f'{what}: {watched} never asked'
        _assert_same(base, got, f'{what}, fill {fill}')
        print(f'{what}: fill {fill}: {n_req} workspaces, {sum(hook.sizes())} bytes, guards intact, {len(got)} outputs bit-identical')


# ------------------------------------------------------------------------------------------------ InstanceNorm, block tail
def _in_inputs(name):
    """x, res, dy (N, C), lens: norm_pool_grads_ref's edge clouds [1, 0, 5, rows + 1], or one cloud of 66 chunks beside a one-row cloud."""
    from tests import norm_pool_grads_ref as NP
    if name == 'chunks66':
        C = 32
        rows = NP.in_rows(2, 65 * 128 + 3, C)
        lens = [65 * rows + 3, 1]
        assert NP.in_rows(2, max(lens), C) == rows and -(-lens[0] // rows) == 66
        N = sum(lens)
        return C, lens, _randn((N, C), 1, 1.0, 2.0), _randn((N, C), 2, 1.0, 1.0), _randn((N, C), 3)
    c = NP.draw_case(name)
    assert c['lens'][:3] == [1, 0, 5] and c['lens'][3] == NP.in_rows(4, c['max_len'], c['C']) + 1
    return c['C'], c['lens'], _dev(c['x']), _dev(c['res']), _dev(c['dy'])


def _instnorm_stats(name):
    from regtr_amd import ops
    C, lens, x, _, _ = _in_inputs(name)
    seg = _seg(lens)
    return (lambda: [ops.instnorm_stats(x, seg, max(lens))]), [('regtr_instnorm_ws_bytes', (len(lens), max(lens), C))]


def _instnorm_bwd(name):
    """The normalised shortcut with LeakyReLU: all three means of the carved table are used."""
    from regtr_amd import ops
    C, lens, x, res, dy = _in_inputs(name)
    seg, ml = _seg(lens), max(lens)

    def run():
        st, rst = ops.instnorm_stats(x, seg, ml), ops.instnorm_stats(res, seg, ml)
        dx, dres = ops.instnorm_bwd(x, seg, ml, st, dy, residual=res, res_stats=rst, lrelu=True, want_dx=True, want_dres=True)
        return [st, rst, dx, dres]
    return run, [('regtr_instnorm_bwd_ws_bytes', (len(lens), ml, C)), ('regtr_instnorm_ws_bytes', (len(lens), ml, C))]


for _n in ('in_c4', 'in_c1024', 'chunks66'):
    case('regtr_instnorm_ws_bytes', name=f'instnorm_stats_{_n}', args=(_n,))(_instnorm_stats)
    case('regtr_instnorm_bwd_ws_bytes', name=f'instnorm_bwd_{_n}', args=(_n,))(_instnorm_bwd)

BT_CHUNK = 2048                     # rows of one cloud per workgroup of the block tail's moment pass (csrc/block_tail.hip MO_ROWS_WG)
BT_LENS = {'edge': [1, 0, 5, BT_CHUNK + 1], 'chunks66': [65 * BT_CHUNK + 3, 1]}


def _block_tail(layout, first_block):
    from regtr_amd import ops
    lens = BT_LENS[layout]
    M, seg, ml = sum(lens), _seg(lens), max(lens)
    if first_block:                 # K1 = 16, K2 = 0, N = 64: rows of 15 weighted sums padded to 16, divided by the neighbour count
        wf = _randn((M, 16), 11)
        wf[:, 15] = 0
        num = torch.randint(1, 41, (M,), device='cuda', generator=torch.Generator(device='cuda').manual_seed(12)).float()
        w16 = _randn((16, 64), 13, 0.3)
        w16[15] = 0
        run = lambda: list(ops._block_tail(wf, None, num, None, w16, None, seg, ml, 0.1, 1e-5, True))
        return run, [('regtr_block_tail_ws_bytes', (len(lens), ml, 64, 16, 0))]
    x1, f = _randn((M, 32), 14, 1.0, 0.5), _randn((M, 64), 15, 1.0, -0.5)
    x1_stats = ops.instnorm_stats(x1, seg, ml)
    sw1, sw2 = ops.SplitWeight(_randn((32, 128), 16, 0.2), 'kn'), ops.SplitWeight(_randn((64, 128), 17, 0.2), 'kn')
    run = lambda: list(ops.block_tail(x1, x1_stats, f, sw1, sw2, seg, ml, want_stats=True))
    return run, [('regtr_block_tail_ws_bytes', (len(lens), ml, 128, 32, 64))]


@case('regtr_block_tail_ws_bytes')
def block_tail_edge():
    return _block_tail('edge', False)


@case('regtr_block_tail_ws_bytes')
def block_tail_chunks66():
    return _block_tail('chunks66', False)


@case('regtr_block_tail_ws_bytes')
def first_block_edge():
    return _block_tail('edge', True)


# ------------------------------------------------------------------------------------------------ dense: statistics partials, split-K
def _stat_lens(R):
    """Three clouds whose boundaries fall inside a row tile of R rows and one tile-aligned cloud: offsets R + 7, 3 R + 3, 4 R, 6 R -- the
    (tile, cloud) slots t + b of a tile that holds no row of cloud b are never written."""
    lens = [R + 7, 2 * R - 4, R - 3, 2 * R]
    off = np.cumsum(lens)
    assert off[0] % R and off[1] % R and off[2] % R == 0 and off[3] == 6 * R
    return lens


def _partial_bytes(M, R, n_clouds, N):
    return (-(-M // R) + n_clouds) * N * 2 * 8


def _gemm_x3_stats(N, K, fold):
    from regtr_amd import _lib, ops
    L = _lib.lib()
    R = L.regtr_gemm_x3_stat_tile_rows(6 * 64, N, K)
    lens = _stat_lens(R)
    M, seg = sum(lens), _seg(lens)
    assert R > 0 and L.regtr_gemm_x3_stat_tile_rows(M, N, K) == R and L.regtr_gemm_x3_supported(M, N, K)
    a, sw = _randn((M, K), 21, 1.0, 0.3), ops.SplitWeight(_randn((K, N), 22, K ** -0.5), 'kn')
    a_stats = ops.instnorm_stats(a, seg, max(lens)) if fold else None

    def run():
        keep, ops.force_x3_gemm = ops.force_x3_gemm, True
        try:
            return list(ops.gemm(a, sw, a_stats=a_stats, a_seg_off=seg if fold else None, want_stats=(seg, max(lens))))
        finally:
            ops.force_x3_gemm = keep
    expect = [('gemm_stats_partial', _partial_bytes(M, R, len(lens), N))]
    if L.regtr_gemm_x3_ws_bytes(M, N, K):
        expect.append(('regtr_gemm_x3_ws_bytes', (M, N, K)))
    return run, expect


@case('gemm_stats_partial')
def gemm_x3_stats_epilogue():
    return _gemm_x3_stats(64, 64, False)


@case('gemm_stats_partial')
def gemm_x3_stats_epilogue_folded_operand():
    return _gemm_x3_stats(128, 64, True)


@case('gemm_stats_partial', 'regtr_gemm_x3_ws_bytes')
def gemm_x3_split_k_stats_from_the_reduction():
    run, expect = _gemm_x3_stats(64, 512, False)
    assert [q for q, _ in expect] == ['gemm_stats_partial', 'regtr_gemm_x3_ws_bytes'], 'K = 512 on 96 rows must be a split launch'
    return run, expect


@case('regtr_gemm_x3_ws_bytes')
def gemm_x3_split_k_ragged_last_split():
    """K = 1088 = 4 x 256 + 64 over few rows: the last split is shorter than the others; with the fused epilogue."""
    from regtr_amd import _lib, ops
    M, N, K = 203, 64, 1088
    assert _lib.lib().regtr_gemm_x3_ws_bytes(M, N, K) > 0
    a, sw = _randn((M, K), 23), ops.SplitWeight(_randn((K, N), 24, K ** -0.5), 'kn')
    bias, res = _randn((N,), 25), _randn((M, N), 26)

    def run():
        keep, ops.force_x3_gemm = ops.force_x3_gemm, True
        try:
            return [ops.gemm(a, sw, bias=bias, residual=res, relu=True)]
        finally:
            ops.force_x3_gemm = keep
    return run, [('regtr_gemm_x3_ws_bytes', (M, N, K))]


def _gemm_stream_stats(fold):
    from regtr_amd import _lib, ops
    L = _lib.lib()
    R, N, K = L.regtr_gemm_stream_tile_rows(), 64, 32
    lens = _stat_lens(R)
    M, seg = sum(lens), _seg(lens)
    assert L.regtr_gemm_stream_supported(M, N, K)
    a, sw = _randn((M, K), 31, 1.0, 0.3), ops.SplitWeight(_randn((K, N), 32, K ** -0.5), 'kn')
    a_stats = ops.instnorm_stats(a, seg, max(lens)) if fold else None
    return (lambda: list(ops.gemm_stream(a, sw, seg, a_stats=a_stats, want_stats=True))), [('gemm_stats_partial', _partial_bytes(M, R, len(lens), N))]


@case('gemm_stats_partial')
def gemm_stream_stats():
    return _gemm_stream_stats(False)


@case('gemm_stats_partial')
def gemm_stream_stats_folded_operand():
    return _gemm_stream_stats(True)


def _gemm_f32(K, want_plan):
    from regtr_amd import ops
    from tests import dispatch
    M, N = 65, 64
    assert dispatch.gemm_f32_plan(M, N, K) == want_plan
    a, b, div = _randn((M, K), 41), _randn((K, N), 42, K ** -0.5), torch.arange(1, M + 1, device='cuda', dtype=torch.float32)
    return (lambda: [ops.gemm(a, b, row_div=div)]), [('regtr_gemm_f32_ws_bytes', (M, N, K))]


@case('regtr_gemm_f32_ws_bytes')
def gemm_f32_split():
    return _gemm_f32(512, (4, 128, 4))


@case('regtr_gemm_f32_ws_bytes')
def gemm_f32_split_ragged_last():
    return _gemm_f32(544, (4, 160, 4))               # splits of 160, 160, 160 and 64


@case('regtr_gemm_f32_ws_bytes')
def gemm_f32_fewer_splits_than_planes():
    return _gemm_f32(2080, (16, 160, 13))            # the workspace holds 16 planes, 13 are written and read


# ------------------------------------------------------------------------------------------------ transposed GEMMs
def _tn(kind, M, N1, N2):
    from regtr_amd import ops
    a, b = _randn((M, N1), 50 + M % 7), _randn((M, N2), 60 + M % 7)
    if kind == 'tn_any':
        return (lambda: [ops.gemm_tn_any(a, b)]), [('regtr_gemm_tn_any_ws_bytes', (M, N1, N2))]
    return (lambda: [ops.gemm_tn(a, b, fold=kind == 'tn_fold')]), [('regtr_gemm_tn_ws_bytes', (M, N1, N2))]


# (64-row chunks with a short last chunk: 65, 203; scaled chunks with a last chunk of 37 rows: 8197 -- tests/test_gpu_bwd_routes.py TN_CASES)
for _kind, _M, _N1, _N2 in [('tn', 65, 64, 64), ('tn_fold', 65, 64, 64), ('tn', 203, 64, 64), ('tn_fold', 203, 64, 64), ('tn', 8197, 256, 256),
                            ('tn_fold', 8197, 256, 256)]:
    case('regtr_gemm_tn_ws_bytes', name=f'gemm_{_kind}_m{_M}', args=(_kind, _M, _N1, _N2))(_tn)
for _M, _N1, _N2 in [(65, 15, 64), (203, 64, 50), (203, 70, 50), (8197, 480, 96)]:          # (70, 50), (480, 96): both edge guards
    case('regtr_gemm_tn_any_ws_bytes', name=f'gemm_tn_any_m{_M}_{_N1}x{_N2}', args=('tn_any', _M, _N1, _N2))(_tn)


# ------------------------------------------------------------------------------------------------ cross-encoder backward
def _layernorm_bwd(n, D):
    from regtr_amd import ops
    x, dy, dres, gamma = _randn((n, D), 71), _randn((n, D), 72), _randn((n, D), 73), _randn((D,), 74, 0.1, 1.0)
    return (lambda: list(ops.layernorm_bwd(x, gamma, dy, dres=dres))), [('regtr_layernorm_bwd_ws_bytes', (n, D))]


def _bias_relu_bwd(n, N):
    from regtr_amd import ops
    g, h = _randn((n, N), 75), torch.relu(_randn((n, N), 76))

    def run():
        dh, db = ops.bias_relu_bwd(g, h)
        return [dh, db, ops.bias_relu_bwd(g)]
    return run, [('regtr_bias_relu_bwd_ws_bytes', (n, N))]


for _n in (33, 32769):
    for _D in (64, 1024):
        case('regtr_layernorm_bwd_ws_bytes', name=f'layernorm_bwd_n{_n}_d{_D}', args=(_n, _D))(_layernorm_bwd)
    for _N in (64, 400):
        case('regtr_bias_relu_bwd_ws_bytes', name=f'bias_relu_bwd_n{_n}_w{_N}', args=(_n, _N))(_bias_relu_bwd)


def _mha_bwd(layout):
    """tests/test_gpu_mha_grads.py's layouts: lengths off the 32-row tile, a cloud nobody attends ('shared'), a zero-length cloud ('empty')."""
    from regtr_amd import ops
    from tests.test_gpu_mha_grads import PAD_ROWS, _inputs, _layout
    lens, kv = _layout(layout)
    n_heads, E, N = 8, 256, sum(lens)
    qkv, d_out = _inputs(lens, n_heads, False, 7)
    t, d = _dev(qkv[:N]), _dev(d_out[:N])
    seg, kv_of = _seg(lens), _dev(np.array(kv), torch.int32)
    assert PAD_ROWS > 0
    return (lambda: list(ops.mha_bwd(t[:, :E], t[:, E:2 * E], t[:, 2 * E:], d, seg, kv_of, max(lens), n_heads))), \
        [('regtr_mha_bwd_ws_bytes', (N, n_heads))]


@case('regtr_mha_bwd_ws_bytes')
def mha_bwd_shared():
    return _mha_bwd('shared')


@case('regtr_mha_bwd_ws_bytes')
def mha_bwd_empty():
    return _mha_bwd('empty')


# ------------------------------------------------------------------------------------------------ losses, head
@case('regtr_infonce_ws_bytes')
def infonce_rows_and_backward():
    """Anchor counts 40, 1 and 130: max_anc exceeds two pairs' counts, one of them a pair of a single anchor."""
    from regtr_amd import ops
    from tests.test_gpu_losses import R_N, R_P, _make_pairs, _pack
    pairs = _make_pairs(np.random.default_rng(81), [(40, 50), (1, 30), (130, 77)], 64, specials=False)
    A, P, ax, px, a_off, p_off = _pack(pairs)
    tA, tP, tax, tpx = _dev(A), _dev(P), _dev(ax), _dev(px)
    ta, tp = _dev(a_off, torch.int32), _dev(p_off, torch.int32)
    max_anc, max_pos = int(np.diff(a_off).max()), int(np.diff(p_off).max())
    grad = torch.tensor(0.7, device='cuda')

    def run():
        out, rl, rm = ops.infonce(tA, tP, tax, tpx, ta, tp, max_anc, R_P, R_N, rows=True)
        saved = ops.infonce_rows(tA, tP, tax, tpx, ta, tp, max_anc, R_P, R_N)
        d_anc, d_pos = ops.infonce_bwd(tA, tP, tax, tpx, ta, tp, max_anc, max_pos, R_N, saved, grad, float(len(pairs)))
        return [out, rl, rm, *saved, d_anc, d_pos]
    return run, [('regtr_infonce_ws_bytes', (len(pairs), max_anc))]


def _head_tail_bwd(m):
    from regtr_amd import ops
    D = 64
    dcorr, dlogit, h2, f = _randn((m, 3), 91), _randn((m,), 92), torch.relu(_randn((m, D), 93)), _randn((m, D), 94)
    w4, wc = _randn((3, D), 95, 0.2), _randn((D,), 96, 0.2)
    return (lambda: list(ops.head_tail_bwd(dcorr, dlogit, h2, f, w4, wc))), [('regtr_head_tail_bwd_ws_bytes', (m, D))]


@case('regtr_head_tail_bwd_ws_bytes')
def head_tail_bwd_m100():
    return _head_tail_bwd(100)


@case('regtr_head_tail_bwd_ws_bytes')
def head_tail_bwd_m1():
    return _head_tail_bwd(1)


# ------------------------------------------------------------------------------------------------ KPConv backward
def _nbr_transpose(ns):
    """Indices uniform over [-1, ns]: both shadows; support 5 is listed by nobody.  ns = 1500: two scan blocks, the second partial;
    ns = 1024: one full block whose last thread writes the total."""
    from regtr_amd import ops
    nq, H = 700, 5
    nbr = np.random.default_rng(ns).integers(-1, ns + 1, (nq, H)).astype(np.int32)
    nbr[nbr == 5] = 6
    nbr[0, 0], nbr[nq - 1, H - 1], nbr[nq // 2, 1] = -1, ns, ns - 1
    t = _dev(nbr, torch.int32)

    def run():
        row_off, entries = ops.nbr_transpose(t, ns)
        return [row_off, entries[:int(row_off[ns])]]           # entries past row_off[ns] are not written
    return run, [('regtr_nbr_transpose_ws_bytes', (nq, H, ns))]


@case('regtr_nbr_transpose_ws_bytes')
def nbr_transpose_ns1500():
    return _nbr_transpose(1500)


@case('regtr_nbr_transpose_ws_bytes')
def nbr_transpose_ns1024():
    return _nbr_transpose(1024)


# ------------------------------------------------------------------------------------------------ ICP
@case('regtr_icp_ws_bytes')
def icp_three_pairs_and_stats_only():
    """Source lengths 700, 2 and 257: three, one and two chunks of the three slots per pair; the two-point pair is done at iteration 0, so
    its slots go stale while the others iterate.  Then the stats-only call (evaluate_registration)."""
    from regtr_amd import refine
    from tests import icp_ref as R
    from tests.test_icp_host import H
    lens = [700, 2, 257]
    assert refine.CHUNK == 256
    srcs, tgts, poses = [], [], []
    for k, n in enumerate(lens):
        gt = R.pose_of([1 + k, 2, 3 - k], 10.0 + 7 * k, [0.3 - 0.1 * k, -0.2, 0.05 * k])
        s, t, _, _ = R.overlapping_pair(n, H, 200 + k, gt, extra=17 + 5 * k)
        srcs.append(_dev(s)); tgts.append(_dev(t))
        poses.append(np.asarray(R.perturbed(gt, [k % 3 == 0, 1, k % 2], 2.0, [0.01, -0.005, 0.008]), np.float32)[:3])
    pose0 = _dev(np.stack(poses))
    md = 1.2 * H

    def run():
        r = refine.icp(srcs, tgts, pose0.clone(), md, iters=6, return_idx=True)
        ev = refine.evaluate_registration(srcs, tgts, r.pose, md)
        assert int(r.iters_run[1]) == 0 and int(r.iters_run[0]) > 1, 'the two-point pair stops at once, the long one goes on'
        return [r.pose, r.fitness, r.inlier_rmse, r.n_inliers, r.iters_run, r.idx, *ev]
    return run, [('regtr_icp_ws_bytes', (len(lens), max(lens)))]


# ------------------------------------------------------------------------------------------------ optimiser
@case('optim_partials')
def grad_norm_and_adam_step_plain_and_guarded():
    """grad_sumsq + grad_norm_finish + adam_step, then the guarded form, over tensors of 0, 1, 257 and one norm slice + 1 elements."""
    from regtr_amd import ops
    ns = ops.optim_slices()[0]
    lens = [0, 1, 257, ns + 1]
    rng = np.random.default_rng(101)
    host = [[rng.standard_normal(n).astype(F32) for n in lens] for _ in range(2)] + [[np.abs(rng.standard_normal(n)).astype(F32) for n in lens]]
    grads = [_dev(rng.standard_normal(n).astype(F32)) for n in lens]
    hyper = (1e-3, 1e-2, 0.9, 0.999, 1e-8)
    scalars = [hyper + (1.0 - 0.9 ** 3, float(np.sqrt(1.0 - 0.999 ** 3)))] * len(lens)

    def run():
        p, m, v = ([_dev(h) for h in hs] for hs in host)
        partials = ops.grad_sumsq(grads)
        nc = ops.grad_norm_finish(partials, 0.1)
        ops.adam_step(p, grads, m, v, scalars, clip_coef=nc[1:])
        p2, m2, v2 = ([_dev(h) for h in hs] for hs in host)
        steps, guard = torch.full((len(lens),), 2.0, device='cuda'), ops.new_guard('cuda')
        nc2 = ops.clip_adam_step_guarded(p2, grads, m2, v2, [hyper] * len(lens), list(range(len(lens))), steps, guard, 0.1)
        return [partials, nc, *p, *m, *v, nc2, steps, guard, *p2, *m2, *v2]
    return run, [('optim_partials', sum(-(-n // ns) for n in lens) * 8)]


# ------------------------------------------------------------------------------------------------ the C-side orchestrators
def _cut_model():
    """The cut-down model of tests/test_gpu_training_step_grads.py (configuration A) and a maker of its two-pair golden batch."""
    from tests.test_gpu_training_step_grads import _batch, _model
    cfg, model, _ = _model('A')
    return cfg, model, _batch


FWD_LISTS = ('src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp', 'src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap')


def _forward_outputs(pred):
    return [t for k in FWD_LISTS for t in pred[k]] + [pred['pose']]


@case('regtr_cross_encoder_ws_bytes', 'regtr_encoder_ws_bytes')
def one_call_encoder_and_cross_encoder_forward():
    """A two-pair forward in the small-batch regime: the encoder's blocks and the cross-encoder's layers each go out through one C call
    that carves every intermediate from one workspace."""
    from tests import training_step_ref as TS
    cfg, model, batch = _cut_model()
    assert cfg.d_embed == TS.CUT['d_embed'] and cfg.num_encoder_layers == TS.CUT['num_encoder_layers']

    def run():
        with torch.no_grad():
            return _forward_outputs(model(batch()))
    return run, [('regtr_encoder_ws_bytes', None), ('regtr_cross_encoder_ws_bytes', None)]


# ------------------------------------------------------------------------------------------------ parity mode's KD-tree
@case('regtr_kdtree_ws_bytes', 'regtr_kdtree_query_scratch_bytes')
def kdtree_many_clouds():
    """tests/test_ref_order.py's many-cloud batch: lattice ties, clouds of 1, 9 and 11 points, 12-fold duplicates."""
    from regtr_amd import ops
    from tests.util import synth_cloud
    rng = np.random.default_rng(11)
    clouds = [synth_cloud(rng, n, lattice=lat) for n, lat in ((3000, 0.006), (1, 0.0), (9, 0.0), (11, 0.006), (2500, 0.0), (800, 0.02))]
    clouds.append(np.repeat(synth_cloud(rng, 40), 12, axis=0))
    pts, lens = _dev(np.concatenate(clouds)), [len(c) for c in clouds]
    seg, n, cap = _seg(lens), sum(lens), 128

    def run():
        tree = ops.KdTree(pts, seg, n)
        idx, max_count = tree.query(pts, seg, n, 0.0625, 16, list_cap=cap)
        return [idx, torch.tensor([max_count])]
    return run, [('regtr_kdtree_ws_bytes', (n, len(lens))), ('regtr_kdtree_query_scratch_bytes', (cap,))]


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize('query,name', [(q, n) for q in CASES for n in CASES[q]])
def test_launcher_ignores_workspace_leftovers(query, name):
    run, expect = CASES[query][name]()
    assert query in [q for q, _ in expect], 'a case names the size query it is filed under'
    _run_under_fills(run, expect, FILLS, f'{query} / {name}')


def test_whole_model_ignores_workspace_leftovers():
    """forward, training_step(train_backbone=True) + backward (every loss, every parameter's .grad), one FusedAdamW step (parameters and
    moments), validation_step and refine_pose: once without the hook, once under the 0xFF and the random fill."""
    from regtr_amd.optim import FusedAdamW
    cfg, model, batch = _cut_model()
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    params = model.trainable_parameters(backbone=True)
    names = sorted(k for k, p in model.named_parameters() if any(p is q for q in params))
    assert len(names) == len(params)

    def run():
        model.load_state_dict(sd0, strict=True)
        for p in model.parameters():
            p.grad = None
        named = dict(model.named_parameters())
        with torch.no_grad():
            fwd = model(batch())
        outs = _forward_outputs(fwd)
        pred, losses = model.training_step(batch(), train_backbone=True)
        losses['total'].backward()
        outs += [losses[k] for k in model.loss_keys()] + [named[k].grad for k in names]
        opt = FusedAdamW([named[k] for k in names], lr=1e-3, weight_decay=1e-2, max_grad_norm=0.1)
        opt.step()
        outs += [named[k] for k in names] + [opt.state[named[k]][s] for k in names for s in ('exp_avg', 'exp_avg_sq')]
        v_losses, v_metrics = model.validation_step(batch(), 0)
        outs += [v_losses[k] for k in sorted(v_losses)] + [v_metrics[k] for k in sorted(v_metrics)]
        b = batch()
        r = model.refine_pose(b, fwd['pose'][-1], iters=5)
        outs += [r.pose, r.fitness, r.inlier_rmse, r.n_inliers, r.iters_run]
        assert all(t is not None for t in outs)
        return outs

    base = _snapshot(run())
    torch.cuda.synchronize()
    for fill in ('ones', 'random'):
        with PoisonedWorkspaces(fill, seed=RANDOM_SEED) as hook:
            got = _snapshot(run())
        torch.cuda.synchronize()
        n_req = hook.check()
        assert n_req > 50, 'the hook must have served the model\'s workspaces'
        _assert_same(base, got, f'whole model, fill {fill}')
        print(f'whole model: fill {fill}: {n_req} workspaces, {sum(hook.sizes())} bytes, guards intact, {len(got)} tensors bit-identical')
