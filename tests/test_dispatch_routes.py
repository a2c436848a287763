"""CPU: tests/dispatch.py restates the GEMM / attention / KPConv gather / max-pool / InstanceNorm / block-tail dispatchers faithfully, and
the GPU cases reach every instantiation they can launch.

The mirror is checked against the plan queries libregtr_hip.so exports (host-only: no GPU needed); the coverage gate lists every
instantiation of the launch ladders (dispatch.X3_KERNELS / STREAM_KERNELS / MHA_KERNELS / ATTN_XYZ_KERNELS / GATHER_KERNELS /
MAXPOOL_KERNELS) and fails when no parametrized GPU case of tests/test_gpu_dispatch.py, tests/test_gpu_ops.py, tests/test_gpu_pose.py or
tests/test_gpu_gather.py routes to one -- e.g. after a planner retune moved a case off its branch.  The gather mirror is checked against the library's regtr_kpconv_gather_computes_flag only:
a refusal is never probed by calling a launcher with stand-in pointers (a mirror wrong about it would launch on garbage).  The backward
launchers (losses, LayerNorm / bias-ReLU, KPConv) are mirrored and gated the same way at the end of the file: their planners against
the workspace queries, their universes against tests/test_gpu_bwd_routes.py and the four *_grads files.  The exact-f32 GEMM closes the
file: choose_splits against regtr_gemm_f32_ws_bytes, dispatch.F32_KERNELS and its regimes against tests/test_gpu_f32_routes.py, and the
alignment refusals of regtr_layernorm / regtr_add_f32."""
import itertools

from tests import dispatch
from tests import dispatch_worker as dw
from tests import test_gpu_dispatch as gd
from tests import test_gpu_gather as gg

MS = [1, 2, 63, 64, 65, 127, 128, 129, 130, 300, 751, 1000, 2000, 2753, 6000, 9381, 12000, 20000, 38061, 50443, 70000, 100000,
      150000, 300000, 600000, 2400000]
NS = [32, 64, 96, 128, 192, 256, 320, 512, 768, 1024, 2048]
KS = [4, 15, 16, 32, 64, 100, 128, 256, 480, 512, 960, 1000, 1024, 1536, 1920, 3840]


def test_x3_plan_mirror_matches_library():
    """route_x3's planner (x3_plan / x3_plan_f16) against the library's own answers over 4 576 shapes: launch tile height, split-K
    workspace (= the split count), statistics tile height, f16-pair and row-strip support."""
    from regtr_amd import _lib
    L = _lib.lib()
    n = 0
    for M, N, K in itertools.product(MS, NS, KS):
        ok = dispatch.x3_supported(M, N, K)
        assert bool(L.regtr_gemm_x3_supported(M, N, K)) == ok, (M, N, K)
        for st in (0, 1):
            assert bool(L.regtr_gemm_x3_f16_supported(M, N, K, st)) == dispatch.x3_f16_supported(M, N, K, st), (M, N, K, st)
        assert L.regtr_gemm_x3_stat_tile_rows(M, N, K) == dispatch.x3_stat_tile_rows(M, N, K), (M, N, K)
        assert bool(L.regtr_gemm_stream_supported(M, N, K)) == (K in (32, 64, 128) and 32 <= N <= 512 and N % 32 == 0
                                                                 and dispatch.sg_cols_per_wg(N, K) > 0), (M, N, K)
        if not ok:
            assert L.regtr_gemm_x3_tile_rows(M, N, K) == 0 and L.regtr_gemm_x3_ws_bytes(M, N, K) == 0
            continue
        tile, splits, _, _ = dispatch.x3_plan(M, N, K)
        assert L.regtr_gemm_x3_tile_rows(M, N, K) == (64 if tile == 2 else 128), (M, N, K)
        assert L.regtr_gemm_x3_ws_bytes(M, N, K) == (splits * M * N * 4 if splits > 1 else 0), (M, N, K)
        n += 1
    assert n > 2000


def test_f16_pair_never_meets_the_eight_wave_tiled_kernel():
    """X3_LAUNCH launches nothing for the f16 pair on the 8-wave tiled tile; only the tile-0 demotion in regtr_gemm_x3 keeps a launch
    from getting there.  No shape under any planner setting may route to it."""
    envs = gd.FORCED_ENVS + [{'REGTR_X3_TILE': '0', 'REGTR_F16_CW4': '0'}, {'REGTR_X3_STRIP': '0'}, {'REGTR_X3_DEEP': '0'}]
    for env, (M, N, K) in itertools.product(envs, itertools.product(MS, NS, KS)):
        if not dispatch.x3_supported(M, N, K) or M < 1:
            continue
        for fold, st in itertools.product((False, True), (False, True)):
            if not (fold and N == 32):
                assert dispatch.route_x3(M, N, K, 4, fold, st, env) != 'none', (env, M, N, K, fold, st)


def _params(fn, names):
    """The parameter tuples of a pytest-parametrized test function (stacked parametrize marks multiply)."""
    sets = []
    for m in getattr(fn, 'pytestmark', []):
        if m.name == 'parametrize':
            argnames = [a.strip() for a in m.args[0].split(',')] if isinstance(m.args[0], str) else list(m.args[0])
            sets.append([dict(zip(argnames, v if len(argnames) > 1 else (v,))) for v in m.args[1]])
    return [tuple({k: v for d in combo for k, v in d.items()}[n] for n in names) for combo in itertools.product(*sets)]


def _gate(universe, routes):
    reached = set().union(*(dispatch.kernels(r) for r in routes))
    assert 'none' not in reached
    assert reached <= universe, sorted(reached - universe)
    assert not universe - reached, f'instantiations no GPU case reaches: {sorted(universe - reached)}'


def test_every_x3_instantiation_is_reached():
    routes = []
    for M, N, K, planes, fold, st, pad, route in _params(gd.test_gemm_route_vs_fp64, 'M N K planes a_stats want_stats pad route'.split()):
        assert dispatch.route_x3(M, N, K, planes, fold, st, ldc=N + pad) == route, (M, N, K, planes, fold, st)
        routes.append(route)
    for (env,) in _params(gd.test_gemm_forced_route_vs_fp64, ['env']):
        for M, N, K, planes, fold, st, pad in dw.forced_cases():
            routes.append(dispatch.route_x3(M, N, K, planes, fold, st, env, ldc=N if M == 1 else N + pad))
    _gate(dispatch.X3_KERNELS, routes)


def test_every_stream_instantiation_is_reached():
    from tests import test_gpu_ops
    routes = []
    for lens, K, N in _params(test_gpu_ops.test_gemm_stream_vs_exact_f32, ['lens', 'K', 'N']):
        routes += [dispatch.route_stream(sum(lens), N, K, fold) for fold in ((False, True) if K <= 64 else (False,))]
    _gate(dispatch.STREAM_KERNELS, routes)


def test_every_mha_instantiation_is_reached():
    routes = []
    for lens, p, peak, route in _params(gd.test_mha_route_vs_fp64, ['lens', 'precision', 'peak', 'route']):
        assert dispatch.route_mha(lens, p) == route, (len(lens), p)
        routes.append(route)
    routes += [dispatch.route_mha(gd.MHA_8V4_LENS, p, min_wg=1) for p in (0, 1, 3)]     # the dispatch variant's side of the bit-identity test
    _gate(dispatch.MHA_KERNELS, routes)


def test_every_attn_xyz_instantiation_is_reached():
    from tests import test_gpu_pose as gp
    routes = []
    for head_dim, lens, route in _params(gp.test_attn_xyz_vs_fp64, ['head_dim', 'lens', 'route']):
        assert dispatch.route_attn_xyz(lens, head_dim) == route, (head_dim, lens)
        routes.append(route)
    _gate(dispatch.ATTN_XYZ_KERNELS, routes)


def test_gather_flag_mirror_matches_library():
    """Which (Cin, H) regtr_kpconv_gather derives the neighbour flags for (Cin 1, or a multiple of 32 with H <= 64) -- the decision behind
    ops.kpconv's flag pass and the matrix-core route."""
    from regtr_amd import _lib
    L = _lib.lib()
    n = 0
    for Cin, H in itertools.product(list(range(1, 70)) + [94, 95, 96, 97, 127, 128, 160, 192, 256, 320, 512, 1024], list(range(1, 131))):
        assert bool(L.regtr_kpconv_gather_computes_flag(Cin, H)) == dispatch.gather_computes_flag(Cin, H), (Cin, H)
        n += dispatch.gather_computes_flag(Cin, H)
    assert n > 700


def test_gather_mirror_refusals_and_hand_off():
    """The host-side refusals the mirror restates (never probed on the library with stand-in pointers) and the ns * Cin = 2^29 hand-off."""
    assert dispatch.generic_lds(16, 56) == (16, 78848) and dispatch.generic_lds(16, 116) == (16, 163328)
    assert dispatch.route_gather(64, 64, 16, 116, flag_given=True) == 'rowsum+lq<16>'
    assert dispatch.route_gather(64, 64, 16, 117, flag_given=True) == 'refused'
    assert dispatch.route_gather(64, 64, 16, 40) == 'refused'                              # no flag where the gather cannot derive it
    assert dispatch.route_gather(64, 64, 64, 65) == 'refused'
    assert dispatch.route_gather(64, 64, 1, 40, x_stats=True) == 'refused'
    assert dispatch.route_gather(64, 64, 64, 40, xyzf=True, x_stats=True) == 'refused'
    assert dispatch.route_gather(64, 64, 64, 40, ld_wf=16) == 'refused'
    assert dispatch.route_gather(64, 64, 1, 40, ld_wf=16) == 'c1'
    assert dispatch.route_gather(64, 64, 64, 40, aligned16=False) == 'refused'
    assert dispatch.route_gather(64, 64, 64, 40, flag_given=True, aligned16=False) == 'rowsum+lq<64>'
    assert dispatch.route_gather(4096, 2 ** 21 - 1, 256, 40) == 'mfma<10,4>/qpw2'
    assert dispatch.route_gather(4096, 2 ** 21, 256, 40) == 'refused'
    assert not dispatch.ops_flag_pass(2 ** 21 - 1, 256, 40) and dispatch.ops_flag_pass(2 ** 21, 256, 40)
    assert dispatch.route_maxpool(2 ** 24 - 2, 64) == 'mp_buf<4>' and dispatch.route_maxpool(2 ** 24 - 1, 64) == 'mp<4>'
    assert dispatch.route_maxpool(100, 128, aligned16=False) == 'mp<2>'


def _gather_cases():
    """(route, nq, J/V/PRE kernel, lens or None) of every parametrized gather case in tests/test_gpu_gather.py, each route re-derived."""
    out = []
    for Cin, H, nq, mode, route in _params(gg.test_mfma_gather_vs_fp64, 'Cin H nq mode route'.split()):
        assert dispatch.route_gather(nq, nq, Cin, H, gg.KP, dispatch.ops_flag_pass(nq, Cin, H), mode == 'pre', mode == 'stats') == route
        out.append((route, nq, mode))
    for Cin, H, nq, mode, mis, route in _params(gg.test_generic_gather_vs_fp64, 'Cin H nq mode misalign route'.split()):
        assert dispatch.route_gather(nq, nq, Cin, H, gg.KP, True, False, mode == 'stats', mis % 4 == 0) == route
        out.append((route, nq, mode))
    for H, nq, mode, route in _params(gg.test_c1_gather_vs_fp64, 'H nq mode route'.split()):
        for ld_wf in (0, 16):
            assert dispatch.route_gather(nq, nq, 1, H, gg.KP, mode == 'flag', mode == 'records', ld_wf=ld_wf) == route
        out.append((route, nq, mode))
    for ns, route in _params(gg.test_gather_handoff_at_2_29_feature_elements, ['ns', 'route']):
        assert dispatch.route_gather(4096, ns, 256, 40, gg.KP, dispatch.ops_flag_pass(ns, 256, 40)) == route
        out.append((route, 4096, 'plain'))
    return out


def test_every_gather_instantiation_is_reached():
    _gate(dispatch.GATHER_KERNELS, [r for r, _, _ in _gather_cases()])


def test_gather_pipelines_are_reached():
    """The software pipelines see every regime: each k_kpconv_gather_mfma<J, V, PRE> at one query per wave, at some count in 2-7 and at 8,
    the multi-query regimes with a last wave that holds fewer queries than the others; the folded InstanceNorm at 8 per wave on clouds
    whose boundaries fall inside a wave's run (and empty clouds); k_kpconv_gather_c1p<NS> at 2 and at 8 groups per wave."""
    mfma, c1p, stats8 = {}, {}, set()
    for route, nq, mode in _gather_cases():
        for part in route.split('+'):
            if part.startswith('mfma<'):
                k, qpw = part.split('/qpw')
                qpw = int(qpw)
                tail = nq % qpw != 0
                mfma.setdefault(k, set()).add('1' if qpw == 1 else ('2-7' if qpw < 8 else '8') if tail else f'{qpw}/no-tail')
                if mode == 'stats' and qpw == 8:
                    lens = gg._lens(nq)
                    off = list(itertools.accumulate(lens, initial=0))
                    assert 0 in lens and any(o % 8 for o in off[1:-1]), lens
                    stats8.add(k)
            elif part.startswith('c1p<'):
                k, g = part.split('/g')
                c1p.setdefault(k, set()).add(int(g))
    for k in sorted(x for x in dispatch.GATHER_KERNELS if x.startswith('mfma<')):
        assert {'1', '2-7', '8'} <= mfma.get(k, set()), (k, mfma.get(k))
    assert stats8 == {k for k in dispatch.GATHER_KERNELS if k.startswith('mfma<') and not k.endswith(',pre>')}, sorted(stats8)
    for k in ('c1p<2>', 'c1p<3>', 'c1p<4>'):
        assert {2, 8} <= c1p.get(k, set()), (k, c1p.get(k))


def test_every_maxpool_instantiation_is_reached():
    routes = [dispatch.route_maxpool(3001, C) for (C,) in _params(gg.test_maxpool_vs_ref, ['C'])]
    routes += [dispatch.route_maxpool(ns, C) for C, ns in _params(gg.test_maxpool_predicated_at_4_gib, ['C', 'ns'])]
    _gate(dispatch.MAXPOOL_KERNELS, routes)


def test_gather_and_maxpool_edges_are_reached():
    """The regimes around the instantiations: the generic kernel above 64 KiB of dynamic LDS, at the largest tile the launcher accepts, at
    H > 64 with Cin % 32 == 0 and on an unaligned WF, each LQ with and without the folded statistics; both sides of the ns * Cin = 2^29
    hand-off; the Cin = 1 kernel with a derived flag, a given flag and records, at an odd H; max-pool rows of one float4, of a partial
    float4 group per lane and of many, and 4 GiB tables for every predicated QW."""
    gen = [(Cin, H, mode, mis) for Cin, H, _, mode, mis, _ in _params(gg.test_generic_gather_vs_fp64, 'Cin H nq mode misalign route'.split())]
    lds = {dispatch.generic_lds(Cin, H)[1] for Cin, H, _, _ in gen}
    assert max(lds) > 64 * 1024 and any(64 * 1024 < b < dispatch.LDS_LIMIT // 2 for b in lds)
    assert any(dispatch.generic_lds(Cin, H + 1)[1] > dispatch.LDS_LIMIT for Cin, H, _, _ in gen)
    assert {m for Cin, H, m, _ in gen if Cin % 32 == 0 and H > 64} == {'plain', 'stats'}
    assert any(mis % 4 and dispatch.gather_computes_flag(Cin, H) for Cin, H, _, mis in gen)
    assert {(dispatch.generic_lds(Cin, H)[0], m) for Cin, H, m, _ in gen} == {(lq, m) for lq in (16, 32, 64) for m in ('plain', 'stats')}
    assert {ns * 256 - (1 << 29) for ns, _ in _params(gg.test_gather_handoff_at_2_29_feature_elements, ['ns', 'route'])} == {-256, 0}
    c1 = _params(gg.test_c1_gather_vs_fp64, 'H nq mode route'.split())
    assert {m for H, nq, m, r in c1 if r.endswith('c1')} == {'derived', 'flag', 'records'} and any(H % 2 for H, _, _, _ in c1)
    Cs = [C for (C,) in _params(gg.test_maxpool_vs_ref, ['C'])]
    assert 4 in Cs and max(Cs) >= 1024 and {dispatch.route_maxpool(3001, C) for C in Cs if C % 16} == {'mp_buf<4>', 'mp_buf<2>', 'mp_buf<1>'}
    big = _params(gg.test_maxpool_predicated_at_4_gib, ['C', 'ns'])
    assert all(ns * C * 4 == 1 << 32 for C, ns in big) and {dispatch.route_maxpool(ns, C) for C, ns in big} == {'mp<4>', 'mp<2>', 'mp<1>'}


# ------------------------------------------------------------------------------------------------ InstanceNorm, finalize, block tail, strip GEMM
def test_instnorm_rows_mirror_matches_library():
    """in_rows (the rows per workgroup of the InstanceNorm statistics and apply launches) through the library's host-only workspace query:
    cdiv(max_len, rows) n_clouds C 16 + 256 bytes, and 256 for a width the kernels refuse."""
    from regtr_amd import _lib
    L = _lib.lib()
    n = 0
    for nc, ml, C in itertools.product([1, 2, 3, 8, 9, 70, 127, 128, 129, 384, 1023, 1024, 1025, 4000],
                                       [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 1000, 1024, 4097, 20000, 131072],
                                       dispatch.NORM_WIDTHS + (12, 2048, 0)):
        assert L.regtr_instnorm_ws_bytes(nc, ml, C) == dispatch.instnorm_ws_bytes(nc, ml, C), (nc, ml, C)
        n += C in dispatch.NORM_WIDTHS
    assert n > 2000
    assert all(L.regtr_instnorm_ws_bytes(4, 100, C) == 256 for C in (12, 2048, 0, 6, 1028))
    assert dispatch.route_instnorm(4, 100, 12) == 'refused' and dispatch.route_instnorm(4, 0, 64) == 'none'


def test_block_tail_mirror_matches_library():
    from regtr_amd import _lib
    L = _lib.lib()
    for M, N, K1, K2 in itertools.product([0, 1, 300, 131072], [32, 64, 128, 256], [0, 16, 32, 64], [0, 16, 32, 64]):
        r = dispatch.route_block_tail(M, N, K1, K2)
        assert bool(L.regtr_block_tail_supported(M, N, K1, K2)) == (r != 'refused'), (M, N, K1, K2)
        for nc, ml in itertools.product([1, 2, 70, 384], [0, 1, 2047, 2048, 2049, 70000]):
            assert L.regtr_block_tail_ws_bytes(nc, ml, N, K1, K2) == dispatch.block_tail_ws_bytes(nc, ml, N, K1, K2), (nc, ml, N, K1, K2)
    assert dispatch.route_block_tail(5, 128, 32, 64).count('+') == 3 and dispatch.route_block_tail(5, 64, 16, 0).count('+') == 2


def test_every_instnorm_regime_is_reached():
    """The statistics cases reach every reachable (C, rows) pair of in_rows; the apply cases reach the refusal widths' neighbours (C = 512 /
    1024) and the smallest rows of a small launch."""
    from tests import test_gpu_norm as gn
    reached = set()
    for C, kind, rows in _params(gn.test_instnorm_stats_vs_fp64, 'C kind rows'.split()):
        lens = gn.case_lens(C, kind, rows)
        r = dispatch.in_rows(len(lens), max(lens), C)
        assert r == rows and dispatch.route_instnorm(len(lens), max(lens), C) == f'in_partial/r{r}+in_finalize'
        assert 0 in lens and 1 in lens, (C, kind, rows)
        reached.add((C, r))
    assert reached == dispatch.NORM_KERNELS, sorted(dispatch.NORM_KERNELS - reached)
    many = {C for C, kind, _ in _params(gn.test_instnorm_stats_vs_fp64, 'C kind rows'.split()) if kind == 'many'}
    assert many == set(dispatch.NORM_WIDTHS)
    applied = {(C, dispatch.in_rows(len(lens), max(lens), C)) for C, lens in _params(gn.test_instnorm_apply_vs_fp64, ['C', 'lens'])}
    assert {C for C, _ in applied} >= {4, 64, 256, 512, 1024} and (1024, 8) in applied
    combos = {c for C, _ in _params(gn.test_instnorm_apply_vs_fp64, ['C', 'lens']) for c in gn.apply_combos(C)}
    assert len(combos) == 2 * 3 * 2 * 2 * 3


def test_every_finalize_form_is_reached():
    """Both finalize kernels, on either side of n_clouds C = 4096 and at it, all three thread-form block sizes, tile_rows 1 / 64 / 128 / 256,
    clouds over one to 300 tiles, starting mid-tile, and empty clouds."""
    from tests import test_gpu_norm as gn
    routes, sides, spans, mid, empty = set(), set(), set(), False, False
    for C, T, lens in _params(gn.test_instnorm_finalize_tiles_vs_fp64, 'C tile_rows lens'.split()):
        routes.add(dispatch.route_finalize_tiles(len(lens), C))
        sides.add(len(lens) * C - 4096)
        off = list(itertools.accumulate(lens, initial=0))
        for b, n in enumerate(lens):
            if n:
                spans.add((off[b + 1] - 1) // T - off[b] // T + 1)
                mid |= off[b] % T != 0
            empty |= n == 0
    assert routes == dispatch.FINALIZE_KERNELS
    assert 0 in sides and any(s < 0 for s in sides) and any(s > 0 for s in sides)
    assert {T for _, T, _ in _params(gn.test_instnorm_finalize_tiles_vs_fp64, 'C tile_rows lens'.split())} == {1, 64, 128, 256}
    assert 1 in spans and max(spans) >= 300 and mid and empty


def test_every_tail_instantiation_is_reached():
    """Both block-tail forms, on clouds at the 512-row wave and 2048-row chunk edges of k_moments, one-row and empty clouds, many clouds per
    256-row tile; and every strip GEMM instantiation from the float64 strip test as well."""
    from tests import test_gpu_norm as gn
    from tests import test_gpu_ops
    routes = []
    for (lens,) in _params(gn.test_block_tail_vs_fp64, ['lens']):
        routes.append(dispatch.route_block_tail(sum(lens), 128, 32, 64))
    for (lens,) in _params(gn.test_first_block_direct_vs_fp64, ['lens']):
        routes.append(dispatch.route_block_tail(sum(lens), 64, 16, 0))
    assert len(_params(gn.test_first_block_kpconv_vs_fp64, ['records'])) == 2
    _gate(dispatch.TAIL_KERNELS, routes)
    all_lens = [n for (lens,) in _params(gn.test_block_tail_vs_fp64, ['lens']) for n in lens]
    assert {0, 1, 511, 512, 513, 2047, 2048, 2049} <= set(all_lens) and any(n > 4096 for n in all_lens)
    assert any(len(lens) >= 64 and max(lens) <= 4 for (lens,) in _params(gn.test_block_tail_vs_fp64, ['lens']))
    assert [1] in [lens for (lens,) in _params(gn.test_block_tail_vs_fp64, ['lens'])]
    routes = []
    for li, K, N in _params(gn.test_gemm_stream_vs_fp64, ['li', 'K', 'N']):
        M = sum(test_gpu_ops.STREAM_LENS[li])
        routes += [dispatch.route_stream(M, N, K, fold) for fold in ((False, True) if K <= 64 else (False,))]
    _gate(dispatch.STREAM_KERNELS, routes)
    assert {li for li, _, _ in _params(gn.test_gemm_stream_vs_fp64, ['li', 'K', 'N'])} == set(range(len(test_gpu_ops.STREAM_LENS)))


# ------------------------------------------------------------------------------------------------ the backward launchers
BWD_NS = [0, 1, 31, 32, 33, 4099, 32767, 32768, 32769, 32772, 32773, 49151, 49152, 49153, 131072, 131073, 1000000, 2400000]


def test_bwd_chunk_rows_mirror_matches_library():
    """bwd_chunk_rows through the two workspace queries that reveal the chunk count: cdiv(n, rows) 2 D 4 and cdiv(n, rows) N 4 bytes,
    0 for what the launchers refuse; 32 rows up to n = 32768, 36 from 32769, 48 up to 49152, 52 from 49153."""
    from regtr_amd import _lib
    from tests import cross_encoder_grads_ref as CR
    L = _lib.lib()
    for n, W in itertools.product(BWD_NS + [-1], [0, 2, 4, 6, 60, 64, 128, 252, 256, 260, 512, 516, 1020, 1024, 1028, 3072]):
        assert L.regtr_layernorm_bwd_ws_bytes(n, W) == dispatch.layernorm_bwd_ws_bytes(n, W), (n, W)
        assert L.regtr_bias_relu_bwd_ws_bytes(n, W) == dispatch.bias_relu_bwd_ws_bytes(n, W), (n, W)
        assert dispatch.bwd_chunk_rows(n) == CR.chunk_rows(n)                 # the yardstick's own restatement agrees
    assert [dispatch.bwd_chunk_rows(n) for n in (32768, 32769, 49152, 49153)] == [32, 36, 48, 52]
    assert L.regtr_layernorm_bwd_ws_bytes(32769, 64) == -(-32769 // 36) * 2 * 64 * 4
    assert dispatch.route_layernorm_bwd(5, 1028) == 'refused' and dispatch.route_layernorm_bwd(0, 64) == 'none'
    assert dispatch.route_bias_relu_bwd(5, 6, False) == 'refused' and dispatch.route_bias_relu_bwd(0, 64, True) == 'none'
    # 'grouped' from the chunk rows: the narrow kernel's 16 row lanes need 49 rows, which only a chunk beyond 48 rows has
    assert dispatch.route_bias_relu_bwd(49152, 64, False) == 'bias_relu<16>/full/tail_only/sum'
    assert dispatch.route_bias_relu_bwd(49153, 64, False) == 'bias_relu<16>/full/grouped/sum'
    assert dispatch.route_bias_relu_bwd(24, 128, True) == 'bias_relu<32>/full/tail_only/relu'
    assert dispatch.route_bias_relu_bwd(25, 128, True) == 'bias_relu<32>/full/grouped/relu'


def _tn_thresholds(tiles):
    """The row counts at which the split plan of a shape with this many tiles changes regime: one split up to 64 rows, 64-row chunks
    up to 64 target rows (target = cdiv(2048, tiles)), scaled chunks beyond."""
    t = 64 * -(-2048 // tiles)
    return [0, 1, 3, 4, 63, 64, 65, 127, 128, 129, 203, t - 1, t, t + 1, t + 4, 2 * t + 5, 8197, 131077, 2400000]


def test_gemm_tn_split_mirror_matches_library():
    """gemm_tn_splits / tn_any_splits through the workspace queries (splits N1 N2 4 bytes), at each shape's thresholds +- 1."""
    from regtr_amd import _lib
    L = _lib.lib()
    n = 0
    for N1, N2 in [(64, 64), (256, 256), (64, 128), (512, 512), (1024, 1024), (15, 64), (64, 50), (480, 32), (480, 96), (70, 50),
                   (130, 17), (1, 1), (3840, 256)]:
        for M in _tn_thresholds((N1 // 64) * (N2 // 64) or 1) + _tn_thresholds(-(-N1 // 64) * -(-N2 // 64)) + [-1]:
            assert L.regtr_gemm_tn_ws_bytes(M, N1, N2) == dispatch.gemm_tn_ws_bytes(M, N1, N2), (M, N1, N2)
            assert L.regtr_gemm_tn_any_ws_bytes(M, N1, N2) == dispatch.gemm_tn_any_ws_bytes(M, N1, N2), (M, N1, N2)
            n += 1
    assert n > 400
    assert L.regtr_gemm_tn_any_ws_bytes(4, 16384, 16384) == 0 and dispatch.route_gemm_tn_any(4, 16384, 16384) == 'refused'
    assert dispatch.route_gemm_tn(4, 15, 64, False) == 'refused' and dispatch.route_gemm_tn(4, 64, 128, True) == 'refused'
    # (256, 256): 16 tiles, 128 splits aimed at -- 64-row chunks up to 8192 rows, 68 from 8193
    assert [dispatch.gemm_tn_plan(M, 256, 256) for M in (64, 65, 8192, 8193)] == [(1, 64), (2, 64), (128, 64), (121, 68)]
    assert dispatch.tn_any_plan(131072, 15, 64) == (2048, 64) and dispatch.tn_any_plan(131073, 15, 64) == (1928, 68)


def test_nbr_transpose_mirror_matches_library():
    """The workspace of regtr_nbr_transpose (cursors | block sums | scratch list) and the one regime of its scan: k_scan_bsums takes
    cdiv(cdiv(ns, 1024), 256) block sums per thread, one up to ns = 262144."""
    from regtr_amd import _lib
    L = _lib.lib()
    for ns, (nq, H) in itertools.product([0, 1, 1023, 1024, 1025, 4096, 262143, 262144, 262145, 300001, 2400000],
                                         [(0, 7), (1, 1), (3000, 5), (20000, 5), (2 ** 27, 16)]):
        assert L.regtr_nbr_transpose_ws_bytes(nq, H, ns) == dispatch.nbr_transpose_ws_bytes(nq, H, ns), (nq, H, ns)
    assert [dispatch.route_nbr_transpose(ns) for ns in (0, 1, 262144, 262145)] == ['none', 'scan/per1', 'scan/per1', 'scan/perN']


def _bwd():
    from tests import test_gpu_bwd_routes
    return test_gpu_bwd_routes


def test_every_infonce_bwd_instantiation_is_reached():
    from tests import test_gpu_loss_grads as gl
    routes = []
    for D, route in _params(_bwd().test_infonce_widths_vs_float64, ['D', 'route']):
        assert dispatch.route_infonce(D) == route, D
        routes.append(route)
    routes += [dispatch.route_infonce(D) for (D,) in _params(gl.test_infonce_grads_vs_float64, ['D'])]
    _gate(dispatch.INFONCE_KERNELS, routes)
    assert len(dispatch.INFONCE_KERNELS) == 24 and dispatch.route_infonce(576) == dispatch.route_infonce(96) == 'refused'


def test_every_layernorm_bwd_instantiation_is_reached():
    """Every k_layernorm_bwd<NG> with and without a partly outside column group; the rows per workgroup are a kernel argument that no
    instantiation treats differently, and are held to be reached as a regime of their own (32 and beyond), as are many chunks."""
    from tests import test_gpu_cross_encoder_grads as gc
    routes = []
    for n, D, route in _params(_bwd().test_layernorm_bwd_vs_float64, ['n', 'D', 'route']):
        assert dispatch.route_layernorm_bwd(n, D) == route, (n, D)
        routes.append(route)
    routes += [dispatch.route_layernorm_bwd(n, D) for (D,) in _params(gc.test_layernorm_bwd_against_float64, ['D']) for n in gc.ROWS]
    _gate(dispatch.LN_BWD_KERNELS, [r.rsplit('/', 1)[0] for r in routes])
    _gate(dispatch.BWD_ROW_REGIMES, [r.rsplit('/', 1)[1] for r in routes])
    cases = _params(_bwd().test_layernorm_bwd_vs_float64, ['n', 'D'])
    assert any(n > 32 * 64 and D > 512 for n, D in cases)                     # more chunks than one lane of the final sum takes


def test_every_bias_relu_bwd_instantiation_is_reached():
    """Every case runs without h ('sum', its route) and with it ('relu'), as do the model's widths in the cross-encoder file."""
    from tests import test_gpu_cross_encoder_grads as gc
    routes = [dispatch.route_bias_relu_bwd(n, N, with_h) for (N,) in _params(gc.test_bias_relu_bwd_against_float64, ['N']) for n in gc.ROWS
              for with_h in (False, True)]
    for n, N, route in _params(_bwd().test_bias_relu_bwd_vs_float64, ['n', 'N', 'route']):
        assert dispatch.route_bias_relu_bwd(n, N, False) == route, (n, N)
        routes += [route, dispatch.route_bias_relu_bwd(n, N, True)]
    _gate(dispatch.BIAS_RELU_KERNELS, routes)
    assert {k for (k,) in _params(_bwd().test_bias_relu_bwd_vs_float64, ['kind'])} == {'normal', 'exact'}


def test_every_gather_bwd_instantiation_is_reached():
    from tests import kpconv_grads_ref as KR
    from tests import test_gpu_kpconv_grads as gk
    routes = []
    for Cin, KP, route in _params(_bwd().test_gather_bwd_widths_vs_float64, ['Cin', 'KP', 'route']):
        assert dispatch.route_gather_bwd(Cin, KP) == route, (Cin, KP)
        routes.append(route)
    routes += [dispatch.route_gather_bwd(KR.CASES[name]['Cin'], KR.KP) for (name,) in _params(gk.test_gather_bwd_vs_float64, ['name'])]
    _gate(dispatch.GATHER_BWD_KERNELS, routes)
    assert dispatch.route_gather_bwd(257, 15) == dispatch.route_gather_bwd(32, 17) == dispatch.route_gather_bwd(0, 15) == 'refused'


def test_every_nbr_transpose_bwd_instantiation_is_reached():
    routes = []
    for ns, route in _params(_bwd().test_nbr_transpose_scan_regimes, ['ns', 'route']):
        assert dispatch.route_nbr_transpose(ns) == route, ns
        routes.append(route)
    _gate(dispatch.NBR_TRANSPOSE_KERNELS, routes)
    assert any(ns % 1024 == 0 for ns, _ in _params(_bwd().test_nbr_transpose_scan_regimes, ['ns', 'route']))


def test_every_gemm_tn_bwd_instantiation_is_reached():
    """Both entry points in every split regime (the fold in each); regtr_gemm_tn_any's two edge guards in every combination; the
    scaled-chunk cases have chunks beyond 64 rows and a last split whose length is no multiple of 4; M = 0, M < 4 and M = 4 occur."""
    routes, edges, scaled = [], [], 0
    for kind, M, N1, N2, route in _params(_bwd().test_gemm_tn_vs_float64, 'kind M N1 N2 route'.split()):
        if kind == 'tn_any':
            assert dispatch.route_gemm_tn_any(M, N1, N2) == route, (M, N1, N2)
            plan = dispatch.tn_any_plan(M, N1, N2)
            regime = '/'.join(route.split('/')[:2])
            routes.append(regime)
            edges.append('tn_any' + route[len(regime):])
        else:
            assert dispatch.route_gemm_tn(M, N1, N2, kind == 'tn_fold') == route, (kind, M, N1, N2)
            plan = dispatch.gemm_tn_plan(M, N1, N2)
            routes.append(route)
        if 'chunk_scaled' in route:
            assert plan[1] > 64 and plan[0] > 1 and dispatch.tn_last_chunk(M, plan) % 4 != 0, (kind, M, N1, N2, plan)
            scaled += 1
    _gate(dispatch.GEMM_TN_KERNELS, routes)
    _gate(dispatch.TN_ANY_EDGES, edges)
    assert scaled >= 5
    for kind in ('tn', 'tn_fold', 'tn_any'):
        assert {0, 1, 3, 4} <= {M for k, M, _, _, _ in _params(_bwd().test_gemm_tn_vs_float64, 'kind M N1 N2 route'.split()) if k == kind}


# ------------------------------------------------------------------------------------------------ preprocessing (csrc/preprocess.hip)
def _pre():
    from tests import test_gpu_preprocess_routes
    return test_gpu_preprocess_routes


def _around(xs, hi=3000000):
    return sorted({min(max(x + d, 1), hi) for x in xs for d in (-1, 0, 1)})


# capacities around every boundary: 1, 42, 43 and 64 tiles of the table and of the points, 256 tiles, the self kernel's chunk sizes
PRE_CAPS = _around([1, 42, 43, 64, 682, 683, 1024, 28672, 29355, 43008, 43690, 43691, 44032, 65536, 87381, 174762, 174763, 262144, 349525,
                    349526, 524288, 699050, 699051, 1048576, 1398101, 1398102, 2097152, 2796202, 3000000]) + [0, -5]


def test_preprocess_workspace_mirror_matches_library():
    """cellgrid_ws_bytes / grid_subsample_ws_bytes (carve_grid, carve_subsample, the 256-byte carver, + 4096) against the library's
    queries: SCAN_TILE, the 1.5 x table rule and the tile counts are what the scan routes are derived from."""
    from regtr_amd import _lib
    L = _lib.lib()
    for cap in PRE_CAPS:
        for nc in (1, 2, 130):
            assert L.regtr_cellgrid_ws_bytes(cap, nc) == dispatch.cellgrid_ws_bytes(cap), (cap, nc)
            for ro in (0, 1):
                assert L.regtr_grid_subsample_ordered_ws_bytes(cap, nc, ro) == dispatch.grid_subsample_ws_bytes(cap, nc, ro), (cap, nc, ro)
            assert L.regtr_grid_subsample_ws_bytes(cap, nc) == dispatch.grid_subsample_ws_bytes(cap, nc, 0)
    assert len(PRE_CAPS) > 70
    assert [dispatch.live_table(n) for n in (0, 43, 44, 683, 684, 43690, 43691, 43692)] == [64, 64, 128, 1024, 2048, 65536, 65536, 131072]
    assert [dispatch.route_scan(n) for n in (1, 1024, 1025, 65536, 65537, 262144, 262145)] == [
        'scan/chained1', 'scan/chained1', 'scan/chained', 'scan/chained', 'scan/three/per1', 'scan/three/per1', 'scan/three/perN']
    assert [dispatch.route_cellgrid(n) for n in (683, 684, 43691, 43692, 174763, 174764)] == [
        'grid/scan/chained1', 'grid/scan/chained', 'grid/scan/chained', 'grid/scan/three/per1', 'grid/scan/three/per1', 'grid/scan/three/perN']
    # the self kernel's chunk: 16 slots per wave at capacity = live until the launch is capped at 8192 workgroups, then 32, 64, two steps
    assert [dispatch.route_radius_self(n, n) for n in (262144, 349525, 349526, 699051, 699052, 1398101, 1398102)] == [
        'self/spw16/pass1', 'self/spw16/pass1', 'self/spw32/pass1', 'self/spw32/pass1', 'self/spw64/pass1', 'self/spw64/pass1',
        'self/spw64/passN']
    assert [dispatch.radius_cap(K) for K in (0, 1, 40, 128, 129, 160, 224, 225, 300, 448, 449)] == [
        'refused', 256, 256, 256, 320, 320, 448, 512, 512, 512, 'refused']
    assert dispatch.shrinks([64] * 8, 512, 448) == (1, 448) and dispatch.shrinks([64] * 9, 512, 448) == (2, 448)
    assert dispatch.shrinks([64, 64, 64, 63], 256, 40) == (1, 40) and dispatch.shrinks([64, 64, 64], 256, 40) == (0, 192)
    assert dispatch.route_radius_query(65536, 65536) == ('rq/per_wave1', False)
    assert dispatch.route_radius_query(65537, 65537) == ('rq/per_waveN', True)


def test_preprocess_refusals():
    """Argument and workspace refusals of the radius queries and the ordered subsample; stand-in pointers, nothing is launched."""
    from regtr_amd import _lib
    L = _lib.lib()
    FAKE = 0x10000
    big = 1 << 30

    def rq(K=16, order=0, ws_bytes=big):
        return L.regtr_radius_query(FAKE, FAKE, 100, FAKE, 100, 2, 0.1, K, order, FAKE, ws_bytes, FAKE, None, None, None)

    def rs(K=16, order=0, ws_bytes=big):
        return L.regtr_radius_query_self(FAKE, 100, 2, 0.1, K, order, FAKE, ws_bytes, FAKE, None, None, None)

    for f in (rq, rs):
        assert f(K=0) == -2 and f(K=449) == -2 and f(order=2) == -2 and f(K=-3) == -2
        assert f(ws_bytes=dispatch.cellgrid_ws_bytes(100) - 1) == -3 and f(ws_bytes=0) == -3

    def sub(row_order=0, key_mode=0, out_cap=100, ws_bytes=big, n_cap=100):
        return L.regtr_grid_subsample_ordered(FAKE, FAKE, 2, n_cap, 0.05, row_order, key_mode, out_cap, FAKE, FAKE, FAKE, ws_bytes, None)

    assert sub(row_order=1, out_cap=99) == -2                       # the container order is replayed over whole clouds
    assert sub(row_order=1, key_mode=1) == -2 and sub(row_order=1, key_mode=2) == -2
    assert sub(row_order=2) == -2 and sub(key_mode=3) == -2
    for ro in (0, 1):
        assert sub(row_order=ro, ws_bytes=dispatch.grid_subsample_ws_bytes(100, 2, ro) - 1) == -3


def test_binned_reference_equals_the_oracle():
    """tests/preprocess_ref.py: the linear-time restatement equals the brute-force oracle element for element on every small case of the
    GPU file -- the row-regime case (duplicates, lattice ties, an empty cloud, empty rows) at every K and both orders, with bins of the
    default side and of a coarser one, the many-cloud cases, and uniform clouds."""
    import numpy as np
    from tests import preprocess_ref as PR
    c = PR.row_case()
    assert 0 in c['s_lens']
    for order in (0, 1):
        for q, ql in ((c['q'], c['q_lens']), (c['s'], c['s_lens'])):
            full = PR.oracle_radius(q, c['s'], ql, c['s_lens'], c['r'], max(PR.ROW_KS), order)      # a row at K is a prefix of the row at 448
            assert full[1].max() > max(PR.ROW_KS)
            for K in PR.ROW_KS:
                for side in ((None, 0.17) if K in (16, 448) else (None,)):
                    got = PR.binned_radius(q, c['s'], ql, c['s_lens'], c['r'], K, order, cell=side)
                    assert np.array_equal(got[0], full[0][:, :K]) and np.array_equal(got[1], full[1]), (K, order, side)
    for n_clouds in (130, 260):
        pts, lens, r, _ = PR.many_clouds(n_clouds)
        for order in (0, 1):
            ref = PR.oracle_radius(pts, pts, lens, lens, r, 16, order)
            got = PR.binned_radius(pts, pts, lens, lens, r, 16, order)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (n_clouds, order)
    pts, lens, r = PR.uniform_clouds(8000, 44)
    rows = np.arange(5, 8000, 3)
    ql = np.array([(rows < lens[0]).sum(), (rows >= lens[0]).sum()], np.int32)
    ref = PR.oracle_radius(pts[rows], pts, ql, lens, r, 16)
    got = PR.binned_radius(pts, pts, lens, lens, r, 16, q_rows=rows)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def _preprocess_labels():
    """Every label the parametrized cases of tests/test_gpu_preprocess_routes.py reach: the shape labels from the parameters, the row
    labels from the case generator's reference counts."""
    from tests import preprocess_ref as PR
    g = _pre()
    labels = set()
    for n_cap, n_live, route in _params(g.test_subsample_scan_forms, ['n_cap', 'n_live', 'route']):
        assert dispatch.route_subsample(n_cap) == route and n_live <= n_cap
        labels.add(route)
    for ns, route in _params(g.test_cellgrid_scan_forms, ['ns', 'route']):
        assert dispatch.route_cellgrid(ns) == route
        labels.add(route)
        labels.add(dispatch.route_radius_query(ns, ns)[0])                        # the general kernel over every support
    for ns_cap, ns, route in _params(g.test_self_query_chunking, ['ns_cap', 'ns', 'route']):
        assert dispatch.route_radius_self(ns_cap, ns) == route
        labels.add(route)
    for nq_cap, nq, route, empty in _params(g.test_radius_query_wave_runs, ['nq_cap', 'nq', 'route', 'empty']):
        assert dispatch.route_radius_query(nq_cap, nq) == (route, empty)
        labels.add(route)
        if empty and nq_cap >= 16 * nq:
            labels.add('rq/empty_waves')
    for (n_clouds,) in _params(g.test_many_clouds, ['n_clouds']):
        n = len(PR.many_clouds(n_clouds)[0])
        labels |= set(dispatch.route_subsample(n, 1).split('+')) | {dispatch.route_cellgrid(n)}
    rows = _params(g.test_row_regimes, ['kernel', 'K', 'order'])
    assert {(k, o) for k, _, o in rows} == {(k, o) for k in ('rq', 'self') for o in (0, 1)}
    for kernel, K, _ in rows:
        labels |= PR.row_case_labels(K, kernel)[0]
    return labels


def test_every_preprocess_regime_is_reached():
    labels = _preprocess_labels()
    assert labels <= dispatch.PREPROCESS_KERNELS, sorted(labels - dispatch.PREPROCESS_KERNELS)
    assert not dispatch.PREPROCESS_KERNELS - labels, f'regimes no GPU case reaches: {sorted(dispatch.PREPROCESS_KERNELS - labels)}'


def test_preprocess_edges_are_reached():
    """Around the labels: both sides of every scan boundary, live counts far below the capacity in the chained and in the three-launch
    scan, the self kernel's last two regimes at their first size, the limit K = 448, every listed length the row case must produce."""
    from tests import preprocess_ref as PR
    g = _pre()
    sub = _params(g.test_subsample_scan_forms, ['n_cap', 'n_live', 'route'])
    assert {65536, 65537, 262144, 262145} <= {c for c, _, _ in sub}
    assert {dispatch.route_scan(c) for c, n, _ in sub if n * 8 <= c} >= {'scan/chained', 'scan/three/per1'}
    assert {43690, 43692, 174762, 174764} <= {n for n, _ in _params(g.test_cellgrid_scan_forms, ['ns', 'route'])}
    self_cases = _params(g.test_self_query_chunking, ['ns_cap', 'ns', 'route'])
    assert {(c // n) for c, n, r in self_cases if r in ('self/spw4/pass1', 'self/spw8/pass1')} == {4, 2}
    assert {(349526, 349526), (699052, 699052), (1398102, 1398102)} <= {(c, n) for c, n, _ in self_cases}
    # labels that other tests reach as well keep their dedicated cases: the last chained subsample, the query runs beyond one per wave
    assert (65536, 65536, 'sub/scan/chained') in sub
    rq = _params(g.test_radius_query_wave_runs, ['nq_cap', 'nq', 'route', 'empty'])
    assert {(c, e) for c, n, r, e in rq if r == 'rq/per_waveN' and c == n} == {(70001, True), (131072, False)}
    assert any(c >= 16 * n for c, n, _, _ in rq)
    assert {K for _, K, _ in _params(g.test_row_regimes, ['kernel', 'K', 'order'])} >= {40, 300, 448}
    assert dispatch.radius_cap(448) == 448 + 64
    for kernel in ('rq', 'self'):
        listed = PR.row_case_labels(16, kernel)[1]
        assert {1, 31, 32, 33, 40, 64, 65, 72} <= listed and (kernel == 'self' or 0 in listed)
    assert {n for (n,) in _params(g.test_many_clouds, ['n_clouds'])} == {130, 260}


# ------------------------------------------------------------------------------------------------ the exact-f32 GEMM (csrc/gemm.hip)
F32_NS = NS + [1, 3, 15, 31, 33, 50]


def test_gemm_f32_split_mirror_matches_library():
    """choose_splits through the workspace query (splits M N 4 bytes, 0 without a split) over the grid of the split kernel's mirror and
    the thin / unaligned widths; the shapes whose plan the GPU cases lean on, by hand: S asked, chunk (rounded up to 32), S_eff, last chunk."""
    from regtr_amd import _lib
    L = _lib.lib()
    n = 0
    for M, N, K in itertools.product(MS, F32_NS, KS + [515, 640, 1030]):
        assert L.regtr_gemm_f32_ws_bytes(M, N, K) == dispatch.gemm_f32_ws_bytes(M, N, K), (M, N, K)
        n += dispatch.gemm_f32_splits(M, N, K) > 1
    assert n > 500
    last = lambda M, N, K: K - (dispatch.gemm_f32_plan(M, N, K)[2] - 1) * dispatch.gemm_f32_plan(M, N, K)[1]
    assert dispatch.gemm_f32_plan(300, 32, 1030) == (8, 160, 7) and last(300, 32, 1030) == 70
    assert dispatch.gemm_f32_plan(300, 32, 1024) == (8, 128, 8)
    assert dispatch.gemm_f32_plan(300, 3, 640) == (5, 128, 5)
    assert dispatch.gemm_f32_plan(130, 50, 515) == (4, 160, 4) and last(130, 50, 515) == 35
    assert dispatch.gemm_f32_plan(130, 1024, 3840) == (16, 256, 15)
    assert dispatch.gemm_f32_plan(129, 64, 511) == (1, 511, 1) and dispatch.gemm_f32_plan(64 * 384, 64, 3840) == (1, 3840, 1)
    assert dispatch.route_gemm_f32(300, 32, 1030) == 'f32<0,0,4,1>/split/split_short/nk_odd/ktail+splitk_reduce'
    assert dispatch.route_gemm_f32(300, 3, 640) == 'f32<1,0,4,1>/split/nk_even+splitk_reduce'
    assert dispatch.route_gemm_f32(129, 64, 64, lda=68, a_aligned16=False) == 'f32<0,0,2,2>/nosplit/nk_even'
    assert dispatch.route_gemm_f32(129, 32, 64, ldb=33) == 'f32<1,0,4,1>/nosplit/nk_even'
    assert dispatch.route_gemm_f32(5, 32, 64, lda=63) == 'refused' and dispatch.route_gemm_f32(0, 32, 64) == 'none'
    assert dispatch.gemm_f32_fold_tags(305, 32, [33, 1, 0, 64, 7, 200]) == {'fold_one_cloud', 'fold_straddle'}
    assert dispatch.gemm_f32_fold_tags(128, 32, [0, 128, 0]) == {'fold_one_cloud'}


def test_every_gemm_f32_instantiation_is_reached():
    """All five k_gemm_f32 instantiations, each unsplit and split (no split is unreachable: every instantiation has a shape with fewer than
    384 tiles and K >= 512), each with one, an odd and an even number of k tiles per chunk and with a k tail (the unaligned ones with a tail
    shorter than a float4); S_eff < S; the fold on one-cloud and on straddling tiles of both tile shapes, unsplit and split; M = 0 and
    M = 1; the row-tile edges bm - 1, bm, bm + 1 of both tiles."""
    from tests import test_gpu_f32_routes as gf
    plain = _params(gf.test_gemm_f32_vs_fp64_and_chain, 'M N K view route'.split())
    fold = _params(gf.test_gemm_f32_fold_vs_fp64_and_chain, 'N K route'.split())
    routes, seen = [], {}
    for M, N, K, view, route in plain:
        assert gf._r(M, N, K, view) == route, (M, N, K, view)
        routes.append(route)
        seen.setdefault(dispatch.f32_tags(route)[0], set()).update(dispatch.f32_tags(route)[1])
    _gate(dispatch.F32_KERNELS, routes)
    for k in sorted(dispatch.F32_KERNELS - {'splitk_reduce'}):
        want = {'nosplit', 'split', 'nk1', 'nk_odd', 'nk_even', 'ktail'} | ({'ktail_lt4'} if k.startswith('f32<0') else set())
        assert want <= seen[k], (k, sorted(want - seen[k]))
        # a split exists for every instantiation, so none is exempt
        assert any(dispatch.f32_tags(r)[0] == k and 'split' in dispatch.f32_tags(r)[1] for r in routes)
    assert any('split_short' in dispatch.f32_tags(r)[1] for r in routes)
    views = {(dispatch.f32_tags(r)[0], v) for _, _, _, v, r in plain}
    assert {('f32<0,0,4,1>', 'off1'), ('f32<0,0,2,2>', 'off1'), ('f32<1,1,4,1>', 'strided'), ('f32<1,1,2,2>', 'strided'),
            ('f32<1,0,4,1>', 'strided')} <= views
    assert any(v == 'strided' and '+splitk_reduce' in r for _, _, _, v, r in plain)          # ldc > N through the reduction too
    for thin, bm in ((True, 128), (False, 64)):
        Ms = {M for M, N, _, _, _ in plain if (N <= 32) == thin}
        assert {1, bm - 1, bm, bm + 1} <= Ms, (bm, sorted(Ms))
    assert dispatch.route_gemm_f32(0, 32, 64) == 'none' and callable(gf.test_gemm_f32_no_rows)
    for N in (32, 64):
        for split in (False, True):
            tags = set().union(*(dispatch.f32_tags(r)[1] for n, K, r in fold if n == N and ('split' in dispatch.f32_tags(r)[1]) == split))
            assert {'fold_one_cloud', 'fold_straddle'} <= tags, (N, split)
    for N, K, route in fold:
        assert gf._r(gf.FOLD_M, N, K, lens=gf.FOLD_LENS) == route
    assert 0 in gf.FOLD_LENS and 1 in gf.FOLD_LENS
    assert {dispatch.f32_tags(r)[0] for _, _, r in fold} >= {'f32<1,1,4,1>', 'f32<0,0,4,1>', 'f32<1,1,2,2>', 'f32<0,0,2,2>'}


def test_layernorm_and_add_refuse_misaligned_pointers():
    """regtr_layernorm and regtr_add_f32 read and write float4: every non-null pointer must be 16-byte aligned.  Stand-in pointers, only
    calls the host refuses: nothing is launched."""
    from regtr_amd import _lib
    L = _lib.lib()
    FAKE = 0x10000
    names = ['x', 'gamma', 'beta', 'add', 'y', 'y_plain']

    def ln(n=8, D=64, **off):
        p = {k: None if k in off and off[k] is None else FAKE + off.get(k, 0) for k in names}
        return L.regtr_layernorm(p['x'], n, D, p['gamma'], p['beta'], 1e-5, p['add'], p['y'], p['y_plain'], None)

    for name in names:
        for o in (4, 8, 12):
            assert ln(**{name: o}) == -2, (name, o)
            assert ln(n=0, **{name: o}) == -2, (name, o)                 # refused before the empty-input return
    assert ln(add=None, y_plain=None, x=4) == -2 and ln(add=None, y=12) == -2
    assert ln(D=6, x=4) == -2 and ln(D=2) == -2 and ln(n=-1) == -2 and ln(x=None) == -2 and ln(y=None) == -2
    assert ln(n=0) == 0 and ln(n=0, add=None, y_plain=None) == 0           # aligned and empty: accepted, nothing to launch
    for o in (4, 8, 12):
        assert L.regtr_add_f32(FAKE + o, FAKE, 16, FAKE, None) == -2 and L.regtr_add_f32(FAKE, FAKE + o, 16, FAKE, None) == -2
        assert L.regtr_add_f32(FAKE, FAKE, 16, FAKE + o, None) == -2
    assert L.regtr_add_f32(FAKE, FAKE, 0, FAKE, None) == 0
