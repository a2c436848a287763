"""GPU (-m gpu): every GEMM and attention instantiation the dispatchers can launch, against float64.

Natural shapes (the product library: the branches large forwards take) and forced routes at small, ragged shapes (a child process per
planner setting on libregtr_hip.dispatch.so, tests/dispatch_worker.py).  tests/dispatch.py names the route of every case, and
tests/test_dispatch_routes.py (CPU) asserts that the cases below reach every instantiation of the launch ladders."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import dispatch, dispatch_worker as dw
from tests.util import ROOT

pytestmark = pytest.mark.gpu


def natural_lens(M):
    """Large clouds around an empty cloud, two one-row clouds and a 37-row cloud, all inside one row tile."""
    return [M // 3, 0, 1, 37, 1, M - M // 3 - 39]


# (M, N, K, planes, a_stats, want_stats, ldc - N, route): planes 4 = the f16 pair; route as tests/dispatch.py:route_x3 names it
X3_NATURAL = [
    (50443, 512, 256, 3, False, False, 4, 'x3d<4,4,4>/p3'),                 # the wide contractions of a large forward: interleaved 128 x 128
    (50443, 512, 256, 3, False, True, 4, 'x3d<4,4,4>/p3/stat'),
    (50443, 512, 256, 4, False, False, 3, 'x3d<4,4,2>/p4'),
    (50443, 512, 256, 4, False, True, 4, 'x3d<4,4,2>/p4/stat'),
    (100000, 256, 64, 3, True, False, 4, 'x3/tile0/p3/astats'),             # level-0/1 unary with InstanceNorm folded into A
    (100000, 256, 64, 3, True, True, 3, 'x3/tile0/p3/astats/stat'),
    (100000, 256, 64, 4, True, False, 4, 'x3/tile1/p4/astats'),             # f16 pair: the folded-norm tile-0 -> tile-1 demotion
    (100000, 256, 64, 4, True, True, 4, 'x3/tile1/p4/astats/stat'),
    (300000, 64, 32, 3, True, True, 4, 'x3/tile1/p3/astats/stat'),
    (300000, 64, 32, 4, True, False, 4, 'x3/tile1/p4/astats'),
    (70000, 64, 960, 3, False, False, 3, 'x3d<4,2,3>/p3'),                  # deep K, 128 x 64 strips
    (70000, 64, 960, 3, False, True, 4, 'x3d<4,2,3>/p3/stat'),
    (70000, 64, 960, 4, False, True, 4, 'x3d<4,2,2>/p4/stat'),
    (70000, 128, 64, 3, False, True, 4, 'x3/tile2/p3/stat'),                # more than 512 tiles of 64 x 64
    (70000, 128, 64, 4, False, True, 4, 'x3/tile2/p4/stat'),
    (70000, 128, 64, 4, False, False, 4, 'x3d<4,2,2>/p4'),                  # x3_plan_f16: 64 x 64 promoted to 128 x 64 strips
    (2000, 128, 64, 3, False, True, 4, 'x3q/p3/stat'),
    (2000, 128, 64, 4, False, True, 4, 'x3q/p4/stat'),
    (2000, 128, 64, 3, True, True, 4, 'x3/tile2/p3/astats/stat'),
    (2000, 128, 64, 4, True, False, 4, 'x3/tile2/p4/astats'),
    (751, 1024, 1024, 3, False, True, 3, 'x3/tile2/p3+reduce_stats/novec'),  # one pair per forward: few tiles, deep K -> split-K
    (751, 1024, 1024, 4, False, True, 4, 'x3/tile2/p4+reduce_stats/vec'),
    (751, 256, 1024, 3, False, True, 4, 'x3q/p3+reduce_stats/vec'),
    (751, 256, 1024, 4, False, True, 2, 'x3q/p4+reduce_stats/novec'),
    (751, 256, 1024, 3, False, False, 4, 'x3q/p3+reduce'),
    (130, 2048, 1024, 3, False, True, 0, 'x3q/p3+reduce+stats_pass'),       # N > 1024: no statistics reduction (see the test)
    (130, 2048, 1024, 4, False, True, 0, 'x3q/p4+reduce+stats_pass'),
]

# planner settings of the forced-route children (REGTR_DEV=1 REGTR_VARIANT=dispatch); each runs dispatch_worker.forced_cases()
FORCED_ENVS = [
    {},                                                      # the planner's own choice at small shapes: x3q, tiled 64 x 64, split-K
    {'REGTR_X3_TILE': '0'},                                  # 128 x 128: interleaved strip kernel; tiled where K % 32 != 0
    {'REGTR_X3_TILE': '0', 'REGTR_X3_IL': '0'},              # 128 x 128 strips, two-slot A ring
    {'REGTR_X3_TILE': '0', 'REGTR_X3_STRIP': '0'},           # the 8-wave tiled kernel; f16 pair demoted to 128 x 64
    {'REGTR_X3_TILE': '1'},                                  # 128 x 64 strips, A two tiles ahead
    {'REGTR_X3_TILE': '1', 'REGTR_X3_ARING': '2'},           # 128 x 64 strips, two-slot A ring
    {'REGTR_X3_TILE': '1', 'REGTR_X3_STRIP': '0'},           # the 128 x 64 tiled kernel
    {'REGTR_X3_TILE': '2', 'REGTR_X3_DEEP': '0', 'REGTR_X3_SPLITS': '3'},   # 64 x 64 tiled kernel, split-K in three (K = 1000: short last chunk)
]

MHA_EDGE = [129, 255, 256, 257, 1, 0, 300]                  # x 13: the swapped partner of a 256-token cloud is an empty cloud
# (lens, precision, peak, route)
MHA_NATURAL = [
    *[([260, 130] * 260, p, 0.0, f'mha_bf16<BW8>/p{p}') for p in (0, 1, 3)],               # 8 320 eight-wave workgroups
    *[([560 + (37 * i) % 81 for i in range(512)], p, 0.0, f'mha_bf16<BW8>/p{p}') for p in (0, 1, 3)],   # ModelNet-like: 512 clouds
    *[(MHA_EDGE[:6], p, 0.0, r) for p, r in ((0, 'mha_f32<4>'), (1, 'mha_bf16<BW4>/p1'), (2, 'mha_f32<4>'), (3, 'mha_f32<4>'))],
    *[(MHA_EDGE * 13, p, 0.0, r) for p, r in ((0, 'mha_bf16<BW4>/p0'), (1, 'mha_bf16<BW4>/p1'), (2, 'mha_f32<1>'), (3, 'mha_bf16<BW4>/p3'))],
    *[(MHA_EDGE * 13, p, 96.0, r) for p, r in ((0, 'mha_bf16<BW4>/p0'), (2, 'mha_f32<1>'), (3, 'mha_bf16<BW4>/p3'))],   # peaked logits
]
MHA_8V4_LENS = MHA_EDGE * 3 + [64]                          # 22 clouds: the 4-wave kernel in the product, 8 waves in the dispatch variant
MHA_TOL = {0: 2e-5, 1: 6e-2, 2: 2e-5, 3: 2e-5}

_worst = {}


def _report(route, err):
    _worst[route] = max(_worst.get(route, 0.0), err)
    print(f'{route}: max err {err:.2e} (worst on this route so far {_worst[route]:.2e})')


@pytest.mark.parametrize('M,N,K,planes,a_stats,want_stats,pad,route', X3_NATURAL)
def test_gemm_route_vs_fp64(M, N, K, planes, a_stats, want_stats, pad, route):
    """The split GEMM on the branch a large forward takes, full epilogue, NaN-filled strided C inside finite sentinels: within the
    float32-grade bound of its format (bf16x3: the exact-f32 kernel's bound and 2x its error; f16 pair: 3e-6 relative), every element of
    the view written, nothing outside it; InstanceNorm statistics (ragged clouds, an empty and one-row clouds) vs float64."""
    assert dispatch.route_x3(M, N, K, planes, a_stats, want_stats, ldc=N + pad) == route
    if route.endswith('+stats_pass'):
        # split-K where the reduction cannot emit statistics (N / 4 not a power of two <= 256): ops.gemm hands C to regtr_instnorm_stats,
        # which has the same column limit -- that combination is refused loudly, never answered wrongly; C itself must still be right
        with pytest.raises(RuntimeError, match='regtr_instnorm_stats: invalid argument'):
            dw.check_gemm(M, N, K, planes, a_stats, want_stats, pad, lens=natural_lens(M))
        want_stats, route = False, route[:-len('+stats_pass')]
        assert dispatch.route_x3(M, N, K, planes, a_stats, want_stats, ldc=N + pad) == route
    v = dw.check_gemm(M, N, K, planes, a_stats, want_stats, pad, lens=natural_lens(M))
    _report(route, v['err'])
    assert v['finite'] and v['outside_untouched'], v
    assert v['ok'] and v.get('stats_ok', True), v


def test_gemm_f32_unaligned_a_vs_fp64():
    """The exact-f32 kernel's aligned_a == false form: A a view one column into a wider buffer (16-byte loads impossible)."""
    from regtr_amd import ops
    M, N, K = 751, 256, 256
    g = torch.Generator().manual_seed(3)
    big = torch.randn(M, K + 4, generator=g).cuda()
    a = big[:, 1:K + 1]
    b = torch.randn(K, N, generator=g).cuda()
    bias, res = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
    div = torch.randint(1, 40, (M,), generator=g).float().cuda()
    assert a.data_ptr() % 16 != 0
    out = ops.gemm(a, b, bias=bias, row_div=div, residual=res, relu=True)
    ref = torch.relu(a.double() @ b.double() / div.double()[:, None] + bias.double()) + res.double()
    tol = (2e-6 * K ** 0.5 * 4 + 1e-6) * max(1.0, (a.double() @ b.double()).abs().max().item() / 10)
    err = (out.double() - ref).abs().max().item()
    _report('gemm_f32<unaligned A>', err)
    assert err < tol


def _child(args, env_extra, timeout=900):
    env = dict(os.environ, REGTR_DEV='1', REGTR_VARIANT='dispatch', **env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'dispatch_worker.py')] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize('env', FORCED_ENVS, ids=lambda e: ','.join(f'{k[10:]}={v}' for k, v in e.items()) or 'default')
def test_gemm_forced_route_vs_fp64(env, tmp_path):
    """Every launch branch at small ragged shapes (M = 1, 63, 65, 127, 129; K % 32 != 0; a split-K last chunk shorter than the rest;
    statistics tiles straddling one-row and empty clouds): a child on the dispatch variant with the planner forced by `env` checks each
    case against float64 as test_gemm_route_vs_fp64 does; its plan queries must agree with tests/dispatch.py under the same setting."""
    out = tmp_path / 'verdicts.json'
    r = _child(['gemm', str(out)], env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    verdicts = json.loads(out.read_text())
    assert len(verdicts) == len(dw.forced_cases())
    bad = []
    for v in verdicts:
        ldc = v['N'] if v['M'] == 1 else v['ldc']
        route = dispatch.route_x3(v['M'], v['N'], v['K'], v['planes'], v['a_stats'], v['want_stats'], env, ldc=ldc)
        tile, splits, _, _ = dispatch.x3_plan(v['M'], v['N'], v['K'], env)
        if v.get('plan') != [64 if tile == 2 else 128, splits * v['M'] * v['N'] * 4 if splits > 1 else 0]:
            bad.append(('plan query disagrees with tests/dispatch.py', route, v))
        if not v['pass']:
            bad.append((route, v))
        elif 'err' in v:
            _report(route, v['err'])
    assert not bad, f'{len(bad)} of {len(verdicts)} cases failed; first: {bad[:3]}'


def _check_mha(lens, precision, peak, out_by_kv=None):
    qkv, kvs = dw.mha_inputs(lens, seed=sum(lens), peak=peak)
    q = qkv.cuda()
    E = q.shape[1] // 3
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    worst = 0.0
    for i, kv in enumerate(kvs):
        out = dw.run_mha(lens, precision, qkv, kv) if out_by_kv is None else out_by_kv[i].cuda()
        ref = dw.mha_ref(q[:, :E], q[:, E:2 * E], q[:, 2 * E:], lens, kv, 8)
        for c, n in enumerate(lens):
            if n and not lens[kv[c]]:
                assert out[off[c]:off[c + 1]].abs().max() == 0, 'an empty partner cloud must give zeros'
        assert torch.isfinite(out).all()
        worst = max(worst, (out.double() - ref).abs().max().item())
    return worst


@pytest.mark.parametrize('lens,precision,peak,route', MHA_NATURAL,
                         ids=[f'{len(c[0])}clouds-p{c[1]}' + ('-peak' if c[2] else '') for c in MHA_NATURAL])
def test_mha_route_vs_fp64(lens, precision, peak, route):
    """regtr_mha_fwd on each of its kernels at the launch sizes that select them -- eight-wave workgroups at the real threshold
    (MHA_WIDE_MIN_WG), clouds of 129 / 255 / 256 / 257 / 1 / 0 tokens, an empty partner cloud, peaked logits -- vs float64."""
    assert dispatch.route_mha(lens, precision) == route
    worst = _check_mha(lens, precision, peak)
    _report(route, worst)
    assert worst < MHA_TOL[precision]


def test_mha_eight_waves_bit_identical_to_four(tmp_path):
    """k_mha_fwd_bf16 with eight waves (dispatch variant: MHA_WIDE_MIN_WG = 1) gives the very bits of the four-wave kernel (product
    library, fewer than 4096 eight-wave workgroups) for every precision, as csrc/attention.hip states; both against float64 as well."""
    lens = MHA_8V4_LENS
    for p in (0, 1, 3):
        assert dispatch.route_mha(lens, p) == f'mha_bf16<BW4>/p{p}' and dispatch.route_mha(lens, p, min_wg=1) == f'mha_bf16<BW8>/p{p}'
    path = tmp_path / 'mha8.pt'
    r = _child(['mha', str(path), json.dumps(lens)], {})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    wide = torch.load(path)
    qkv, kvs = dw.mha_inputs(lens, seed=sum(lens))
    for p in (0, 1, 3):
        for i, kv in enumerate(kvs):
            four = dw.run_mha(lens, p, qkv, kv).cpu()
            assert torch.equal(four, wide[f'{p}/{i}']), (p, i, (four - wide[f'{p}/{i}']).abs().max().item())
        worst = _check_mha(lens, p, 0.0, out_by_kv=[wide[f'{p}/{i}'] for i in range(len(kvs))])
        _report(f'mha_bf16<BW8>/p{p} (dispatch variant)', worst)
        assert worst < MHA_TOL[p]
