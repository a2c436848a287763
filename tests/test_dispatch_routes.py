"""CPU: tests/dispatch.py restates the GEMM / attention dispatchers faithfully, and the GPU cases reach every instantiation they can launch.

The mirror is checked against the plan queries libregtr_hip.so exports (host-only: no GPU needed); the coverage gate lists every
instantiation of the launch ladders (dispatch.X3_KERNELS / STREAM_KERNELS / MHA_KERNELS) and fails when no parametrized GPU case of
tests/test_gpu_dispatch.py or tests/test_gpu_ops.py routes to one -- e.g. after a planner retune moved a case off its branch."""
import itertools

from tests import dispatch
from tests import dispatch_worker as dw
from tests import test_gpu_dispatch as gd

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
