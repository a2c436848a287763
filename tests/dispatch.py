"""Which kernel instantiation the host-side dispatchers launch for a shape: a restatement of the C++ policy, for the tests.

route_x3 mirrors csrc/gemm_x3.hip (x3_plan, x3_plan_f16 and the launch ladder at the end of regtr_gemm_x3) as regtr_amd/ops.py:gemm
drives it, route_stream csrc/gemm_stream.hip (sg_cols_per_wg, the SG_L2 / SG_L3 ladder), route_mha csrc/attention.hip (regtr_mha_fwd),
route_attn_xyz its regtr_attn_xyz (the correspondence decoder's coordinate attention, one instantiation per head dimension).
tests/test_dispatch_routes.py checks the mirror against the host-only plan queries of the library and asserts that the GPU cases
(tests/test_gpu_dispatch.py, tests/test_gpu_ops.py, tests/test_gpu_pose.py) reach every instantiation listed in X3_KERNELS / STREAM_KERNELS /
MHA_KERNELS / ATTN_XYZ_KERNELS.  route_gather / route_maxpool mirror csrc/kpconv.hip
(regtr_kpconv_gather with the flag decision of ops.kpconv, regtr_maxpool_gather); their cases are in tests/test_gpu_gather.py and their
universes GATHER_KERNELS / MAXPOOL_KERNELS.  route_instnorm / route_finalize_tiles mirror csrc/norm.hip (in_rows, the finalize split at
n_clouds C = 4096) and route_block_tail csrc/block_tail.hip; their cases are in tests/test_gpu_norm.py and their universes NORM_KERNELS
((C, rows) pairs), FINALIZE_KERNELS and TAIL_KERNELS.

The backward launchers follow at the end: route_infonce / route_gemm_tn (csrc/losses.hip), route_layernorm_bwd / route_bias_relu_bwd
(csrc/layer_bwd.hip, bwd_chunk_rows) and route_gather_bwd / route_nbr_transpose / route_gemm_tn_any (csrc/kpconv_bwd.hip); their cases are in
tests/test_gpu_bwd_routes.py and the four tests/test_gpu_*_grads.py files, their universes LN_BWD_KERNELS, BIAS_RELU_KERNELS,
GATHER_BWD_KERNELS, NBR_TRANSPOSE_KERNELS, GEMM_TN_KERNELS (+ TN_ANY_EDGES) and INFONCE_KERNELS.

The preprocessing section (csrc/preprocess.hip) closes the file: live_table / table_capacity, the two workspace carvers, route_scan,
route_subsample, route_cellgrid, radius_cap, route_radius_query, route_radius_self, and the regimes of one query row (rank_path, shrinks
-- which needs K beside the capacity --, staged, row_labels); cases in tests/test_gpu_preprocess_routes.py, universe PREPROCESS_KERNELS =
PREPROCESS_SHAPE_KERNELS (from launch sizes) | PREPROCESS_ROW_KERNELS (from a reference's counts).

The exact-f32 GEMM (csrc/gemm.hip: choose_splits, the alignment ladder of regtr_gemm_f32) follows the preprocessing section:
gemm_f32_splits, gemm_f32_ws_bytes, route_gemm_f32 (instantiation + regime tags), universe F32_KERNELS; cases in
tests/test_gpu_f32_routes.py.

A route is '+'-joined kernel names: the product kernel, then for split-K its reduction ('reduce', 'reduce_stats/vec' or
'reduce_stats/novec'), then 'stats_pass' when ops.gemm hands C to regtr_instnorm_stats for the statistics instead (split-K with N / 4 not a power of
two <= 256, where that pass refuses the width as well: tests/test_gpu_dispatch.py asserts the error)."""

XBK = 32


def cdiv(a, b):
    return -(-a // b)


def x3_supported(M, N, K):                                              # regtr_gemm_x3_supported
    if M < 0:
        return False
    if N == 32:
        return K >= 64 and K % XBK == 0
    return N >= 64 and N % 64 == 0 and K >= 16 and K % 4 == 0


def x3_rs_ok(N):                                                        # x3_rs_ok: N / 4 a power of two <= 256
    c4 = N >> 2
    return N % 4 == 0 and 1 <= c4 <= 256 and c4 & (c4 - 1) == 0


def x3_rs_rows(N):
    return 1 if N >= 1024 else 1024 // N


def x3_plan(M, N, K, dev_env={}):
    """x3_plan -> (tile, splits, k_chunk, strip); tile 0 = 128 x 128, 1 = 128 x 64, 2 = 64 x 64."""
    if N == 32:
        return 1, 1, K, True                                            # the thin strip form
    strip_on = int(dev_env.get('REGTR_X3_STRIP', 1))
    forced = int(dev_env.get('REGTR_X3_TILE', -1))
    forced_s = int(dev_env.get('REGTR_X3_SPLITS', 0))
    if 0 <= forced <= 2 and (forced != 0 or N % 128 == 0):             # development: forced tile (and split count)
        splits, k_chunk = 1, K
        if forced_s >= 2 and K // forced_s >= 64:
            k_chunk = cdiv(cdiv(K, forced_s), XBK) * XBK
            splits = cdiv(K, k_chunk)
        return forced, splits, k_chunk, bool(strip_on) and forced != 2

    def tiles(bm, bn):
        return cdiv(M, bm) * (N // bn)
    tile = 2
    if tiles(128, 64) >= 512 and (K >= 960 or tiles(128, 64) >= 2048):
        tile = 1
    if N % 128 == 0 and tiles(128, 128) >= 1536:
        tile = 0
    if strip_on and N % 128 == 0 and K >= 1536 and K % XBK == 0 and tiles(128, 128) >= 512:
        tile = 0
    tl = tiles(128, 128) if tile == 0 else tiles(128, 64) if tile == 1 else tiles(64, 64)
    splits, k_chunk = 1, K
    if tl < 384 and K >= 512:
        s = min(cdiv(768, tl), K // 256, 8)
        if s >= 2:
            k_chunk = cdiv(cdiv(K, s), XBK) * XBK
            splits = cdiv(K, k_chunk)
    return tile, splits, k_chunk, bool(strip_on) and tile != 2


def x3_stat_tile_rows(M, N, K, dev_env={}):                             # regtr_gemm_x3_stat_tile_rows
    if not x3_supported(M, N, K) or M < 1:
        return 0
    tile, splits, _, _ = x3_plan(M, N, K, dev_env)
    if splits > 1:
        return x3_rs_rows(N) if x3_rs_ok(N) else 0
    return 64 if tile == 2 else 128


def x3_f16_supported(M, N, K, with_stats, dev_env={}):                 # regtr_gemm_x3_f16_supported (the plan always exists)
    return x3_supported(M, N, K)


def route_x3(M, N, K, planes=3, a_stats=False, want_stats=False, dev_env={}, ldc=None):
    """The kernels ops.gemm(a, SplitWeight, planes=.., a_stats=.., want_stats=..) launches on the split kernel (force_x3_gemm; planes 4 =
    inside `with ops.f16_pair(True)`).  ldc: the leading dimension of C (default N; only the split-K statistics reduction cares)."""
    assert x3_supported(M, N, K) and M > 0 and planes in (1, 2, 3, 4)
    if planes in (1, 2):
        assert not a_stats and not want_stats, 'regtr_gemm_x3 refuses statistics / a folded operand with 1 or 2 planes'
    assert not (N == 32 and a_stats)
    stat = bool(want_stats) and x3_stat_tile_rows(M, N, K, dev_env) > 0   # ops.gemm: R > 0 -> stat_partial, else a pass over C
    tile, splits, k_chunk, strip = x3_plan(M, N, K, dev_env)
    if planes == 4:                                                     # x3_plan_f16: keep_rows = stat_partial | a_stats | tile_info
        if not strip and not (stat or a_stats) and splits == 1 and K % XBK == 0 and cdiv(M, 128) * (N // 64) >= 512:
            tile, strip = 1, True
        if tile == 0 and not int(dev_env.get('REGTR_F16_CW4', 1)):
            tile = 1
        if tile == 0 and (not strip or a_stats or K % XBK or k_chunk % XBK):
            tile = 1                                                    # the 8-wave tiled kernel has no f16 pair form
    sout = stat and splits == 1                                         # split-K: the statistics come from the reduction
    strip = strip and not a_stats and K % XBK == 0 and k_chunk % XBK == 0
    p = f'/p{planes}'
    st = '/stat' if sout else ''
    if strip:                                                           # X3D_LAUNCH(MW, CW, AR): planes != 3 take AR = 2
        cw = 4 if tile == 0 else 2
        if planes != 3:
            ar = 2
        elif tile == 0:
            ar = 4 if int(dev_env.get('REGTR_X3_IL', 1)) else 2
        else:
            ar = 3 if int(dev_env.get('REGTR_X3_ARING', 3)) == 3 else 2
        k = f'x3d<4,{cw},{ar}>{p}{st}'
    elif (int(dev_env.get('REGTR_X3_DEEP', 1)) and tile == 2 and not a_stats and planes in (3, 4) and K % XBK == 0 and k_chunk % XBK == 0
          and cdiv(M, 64) * (N // 64) * splits <= 512):
        k = f'x3q{p}{st}'
    elif planes == 4 and tile == 0:
        k = 'none'                                                      # X3_LAUNCH(2, 4, ..) has no f16 pair form: nothing runs
    else:
        k = f'x3/tile{tile}{p}' + ('/astats' if a_stats else '') + st
    if splits > 1:
        vec = (N if ldc is None else ldc) % 4 == 0
        k += ('+reduce_stats/' + ('vec' if vec else 'novec')) if stat else '+reduce'
    if want_stats and not stat:
        k += '+stats_pass'
    return k


def route_stream(M, N, K, a_stats=False):
    """regtr_gemm_stream: k_gemm_strip<K / 16, columns per workgroup / 32, fold>."""
    nb = sg_cols_per_wg(N, K)
    assert M >= 0 and K in (32, 64, 128) and 32 <= N <= 512 and N % 32 == 0 and nb > 0 and not (a_stats and K > 64)
    kt = K // 16
    return f'strip<{kt},{nb // 32},{int(bool(a_stats) and kt <= 4)}>'


def sg_cols_per_wg(N, K):
    for nb in (128, 64, 32):
        if nb <= N and N % nb == 0 and nb * K * 6 + 8 * nb * 16 <= 64 * 1024:
            return nb
    return 0


def route_mha(lens, precision, min_wg=4096, heads=8):
    """regtr_mha_fwd: the exact-f32 kernel k_mha_fwd<1 | 4> or k_mha_fwd_bf16 with 4 or 8 waves (BW / BW8); min_wg = MHA_WIDE_MIN_WG."""
    TQ, TK, BW, BW8 = 32, 32, 4, 8
    n, max_len = len(lens), max(lens)
    if max_len == 0:
        return 'none'
    small = cdiv(max_len, BW * TQ) * heads * n < 512
    if precision == 2 or (precision in (0, 3) and small):
        return 'mha_f32<4>' if cdiv(max_len, TQ) * heads * n <= 1024 and max_len > 4 * TK else 'mha_f32<1>'
    wide = max_len > BW * TQ and cdiv(max_len, BW8 * TQ) * heads * n >= min_wg
    return f"mha_bf16<{'BW8' if wide else 'BW4'}>/p{precision}"


def kernels(route):
    """The instantiations of a route: a gather kernel's '/qpw<n>' or '/g<n>' suffix (queries or groups per wave) is a launch argument."""
    return {k.split('/')[0] if k.startswith(('mfma<', 'c1p<', 'f32<')) else k for k in route.split('+')}


def _x3_kernels():
    ks = set()
    for planes in (1, 2, 3, 4):
        sts = ('', '/stat') if planes >= 3 else ('',)
        for st in sts:
            for cw, ars in ((4, (4, 2)), (2, (3, 2))):
                for ar in (ars if planes == 3 else (2,)):
                    ks.add(f'x3d<4,{cw},{ar}>/p{planes}{st}')
            if planes >= 3:
                ks.add(f'x3q/p{planes}{st}')
        for tile in ((0, 1, 2) if planes != 4 else (1, 2)):
            for fold in (('', '/astats') if planes >= 3 else ('',)):
                for st in sts:
                    ks.add(f'x3/tile{tile}/p{planes}{fold}{st}')
    return ks | {'reduce', 'reduce_stats/vec', 'reduce_stats/novec', 'stats_pass'}


# every instantiation the launch ladders can reach (the 'none' of an f16 pair launch on the 8-wave tiled kernel is not one of them)
X3_KERNELS = _x3_kernels()
STREAM_KERNELS = {f'strip<{K // 16},{nb // 32},{fold}>' for K in (32, 64, 128) for nb in (32, 64, 128) for fold in ((0, 1) if K <= 64 else (0,))
                  if sg_cols_per_wg(nb, K) == nb}
MHA_KERNELS = {'mha_f32<1>', 'mha_f32<4>'} | {f'mha_bf16<{w}>/p{p}' for w in ('BW4', 'BW8') for p in (0, 1, 3)}


def route_attn_xyz(lens, head_dim):
    """regtr_attn_xyz: k_attn_xyz<HDX> for HDX = head_dim.  No launch without a query row or a token, a check the launcher makes before
    it looks at the head dimension; any other head dimension is refused (RG_ERR_ARG)."""
    if max(lens, default=0) == 0 or sum(lens) == 0:
        return 'none'
    return f'attn_xyz<{head_dim}>' if head_dim in (32, 64, 128, 256) else 'refused'


ATTN_XYZ_KERNELS = {f'attn_xyz<{hd}>' for hd in (32, 64, 128, 256)}


# ------------------------------------------------------------------------------------------------ KPConv gather, max-pool (csrc/kpconv.hip)
GATHER_WAVES, KP_PAD, MG_QPW = 4, 16, 8
LDS_LIMIT = 160 * 1024


def gather_computes_flag(Cin, H):                                       # regtr_kpconv_gather_computes_flag
    return Cin == 1 or (Cin % 32 == 0 and H <= 64)


def ops_flag_pass(ns, Cin, H, x_aligned=True, stats_aligned=True):
    """ops.kpconv runs regtr_rowsum_positive (and hands the gather a flag) unless the gather derives the flags itself."""
    return not (gather_computes_flag(Cin, H) and x_aligned and ns > 0 and ns * Cin < (1 << 29) and stats_aligned)


def generic_lds(Cin, H):
    """Dynamic LDS of k_kpconv_gather<LQ>: GATHER_WAVES tiles of QW queries x H neighbours x (KP_PAD + 6) floats."""
    LQ = 16 if Cin <= 16 else (32 if Cin <= 32 else 64)
    QW = 64 // LQ
    return LQ, GATHER_WAVES * ((QW * H * (KP_PAD + 6) + 3) & ~3) * 4


def mfma_qpw(nq):
    return min(max(cdiv(nq, 256 * 12), 1), MG_QPW)


def c1p_groups(nq):
    return min(max(cdiv(nq, 256 * 8 * GATHER_WAVES * 4), 1), 8)


def route_gather(nq, ns, Cin, H, KP=15, flag_given=False, xyzf=False, x_stats=False, aligned16=True, ld_wf=0):
    """regtr_kpconv_gather's launch for these arguments, after the flag pass 'rowsum' (or 'rowsum/stats' with x_stats) when the caller
    hands it a flag: 'c1', 'c1p<NS>/g<groups per wave>', 'mfma<J,V[,pre]>/qpw<queries per wave>', 'lq<LQ>' (the generic LDS-tile kernel),
    or 'refused' (RG_ERR_ARG).  aligned16: x, wf and x_stats 16-byte aligned; xyzf: packed support records given (assumed aligned)."""
    assert nq > 0
    if ld_wf and ld_wf != KP * Cin and not (Cin == 1 and ld_wf == KP_PAD):
        return 'refused'
    if ns < 0 or H < 1 or Cin < 1 or not 1 <= KP <= KP_PAD or (xyzf and (x_stats or ns * 16 >= 1 << 31)):
        return 'refused'
    if not flag_given and not gather_computes_flag(Cin, H):
        return 'refused'
    pre = ['rowsum/stats' if x_stats else 'rowsum'] if flag_given else []
    if Cin == 1:
        if x_stats:
            return 'refused'
        HP1 = (H + 1) & ~1
        groups = c1p_groups(nq)
        if xyzf and 4 * HP1 <= 4 * 64 and ns > 0 and groups >= 2:
            NS = 2 if 4 * HP1 <= 128 else (3 if 4 * HP1 <= 192 else 4)
            return '+'.join(pre + [f'c1p<{NS}>/g{groups}'])
        return '+'.join(pre + ['c1'])
    fits = aligned16 and ns > 0 and ns * Cin < (1 << 29)
    if not flag_given and not fits:
        return 'refused'
    if gather_computes_flag(Cin, H) and fits:
        J = 10 if H <= 40 else (13 if H <= 52 else 16)
        V = 4 if Cin % 64 == 0 else 2
        return '+'.join(pre + [f"mfma<{J},{V}{',pre' if xyzf else ''}>/qpw{mfma_qpw(nq)}"])
    LQ, lds = generic_lds(Cin, H)
    if lds > LDS_LIMIT:
        return 'refused'
    return '+'.join(pre + [f'lq<{LQ}>'])


def route_maxpool(ns, C, aligned16=True):
    """regtr_maxpool_gather: the branch-free k_maxpool_gather_buf<QW, 8> while the table fits 32-bit byte offsets (and x is 16-byte
    aligned), else the predicated k_maxpool_gather<QW>; QW queries per wave."""
    assert C >= 4 and C % 4 == 0 and ns >= 0
    QW = 4 if C <= 64 else (2 if C <= 128 else 1)
    buf = ns > 0 and ns * C * 4 < 0xffffff00 and aligned16
    return f"{'mp_buf' if buf else 'mp'}<{QW}>"


GATHER_KERNELS = ({'c1', 'c1p<2>', 'c1p<3>', 'c1p<4>', 'lq<16>', 'lq<32>', 'lq<64>', 'rowsum', 'rowsum/stats'}
                  | {f"mfma<{J},{V}{p}>" for J in (10, 13, 16) for V in (2, 4) for p in ('', ',pre')})
MAXPOOL_KERNELS = {f'{k}<{qw}>' for k in ('mp_buf', 'mp') for qw in (4, 2, 1)}


# ------------------------------------------------------------------------------------------------ InstanceNorm, block tail (csrc/norm.hip, csrc/block_tail.hip)
IN_ROWS = 128
NORM_WIDTHS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)                 # C / 4 float4 columns a power of two <= 256


def in_rows(n_clouds, max_len, C):
    """in_rows: rows of one cloud per workgroup of k_instnorm_partial / k_instnorm_apply, halved from 128 while the launch is small."""
    TR = 256 // (C >> 2)
    rows = IN_ROWS
    while rows > 4 * TR and rows > 8 and cdiv(max(max_len, 1), rows) * n_clouds < 1024:
        rows >>= 1
    return rows


def instnorm_ws_bytes(n_clouds, max_len, C):                            # regtr_instnorm_ws_bytes
    if n_clouds < 1 or C not in NORM_WIDTHS:
        return 256
    return cdiv(max(max_len, 1), in_rows(n_clouds, max_len, C)) * n_clouds * C * 16 + 256


def route_instnorm(n_clouds, max_len, C, apply=False):
    """regtr_instnorm_stats ('in_partial/r<rows>+in_finalize') or regtr_instnorm_apply ('in_apply/r<rows>'); 'none' when max_len = 0
    launches nothing, 'refused' for a width the kernels do not take.  The kernels are not templated: the rows are the launch regime."""
    if n_clouds < 1 or C not in NORM_WIDTHS or max_len < 0:
        return 'refused'
    if max_len == 0:
        return 'none'
    r = in_rows(n_clouds, max_len, C)
    return f'in_apply/r{r}' if apply else f'in_partial/r{r}+in_finalize'


def route_finalize_tiles(n_clouds, C):
    """regtr_instnorm_finalize_tiles: a wave per (cloud, channel) while n_clouds C <= 4096, else a thread per channel in blocks of 64 / 128 / 256."""
    if n_clouds * C <= 4096:
        return 'fin_wave'
    return f"fin_thread<{256 if C >= 256 else (128 if C >= 128 else 64)}>"


def _norm_kernels():
    """Every reachable (C, rows): rows halves from 128 while rows > 4 TR and rows > 8 (and the launch is small), TR = 1024 / C."""
    out = set()
    for C in NORM_WIDTHS:
        r = IN_ROWS
        out.add((C, r))
        while r > 4 * (1024 // C) and r > 8:
            r >>= 1
            out.add((C, r))
    return out


def block_tail_supported(M, N, K1, K2):                                 # regtr_block_tail_supported
    return M >= 0 and ((K1, K2, N) in ((32, 64, 128), (16, 0, 64)))


def block_tail_ws_bytes(n_clouds, max_len, N, K1, K2):                  # regtr_block_tail_ws_bytes
    if n_clouds < 1 or not block_tail_supported(0, N, K1, K2):
        return 0

    def al(b):
        return (b + 255) & ~255
    nc = cdiv(max(max_len, 1), 2048)
    return (al(n_clouds * nc * (K1 * K1 + K1) * 8) + al(n_clouds * nc * (K2 * K2 + K2) * 8) + al(n_clouds * 3 * N * K1 * 2)
            + al(n_clouds * 3 * N * K2 * 2) + 2 * (al(n_clouds * K1 * 4) + al(n_clouds * K2 * 4)))


def route_block_tail(M, N, K1, K2):
    """regtr_block_tail's four launches: k_moments<KC, INFOLD, ROWDIV> per source, k_tail_prepare<K1, K2>, k_tail_strip<KT1, KT2, NT, NPASS,
    FOLD1>; 'none' for M = 0, 'refused' for an unserved shape."""
    if not block_tail_supported(M, N, K1, K2):
        return 'refused'
    if M == 0:
        return 'none'
    if K2:
        return 'moments<1,1,0>+moments<2,0,0>+prepare<32,64>+tail_strip<2,4,2,2,1>'
    return 'moments<1,0,1>+prepare<16,0>+tail_strip<1,0,2,1,0>'


NORM_KERNELS = _norm_kernels()
FINALIZE_KERNELS = {'fin_wave', 'fin_thread<64>', 'fin_thread<128>', 'fin_thread<256>'}
TAIL_KERNELS = set().union(*(set(route_block_tail(1, N, K1, K2).split('+')) for N, K1, K2 in ((128, 32, 64), (64, 16, 0))))


# ------------------------------------------------------------------------------------------------ backward launchers
# (csrc/layer_bwd.hip, csrc/kpconv_bwd.hip, csrc/losses.hip; cases in tests/test_gpu_bwd_routes.py and the four *_grads files)
LN_MAX_D = 1024
TN_TILE = 64
SCAN_ITEMS = 1024


def bwd_chunk_rows(n):
    """bwd_chunk_rows: rows per workgroup of both first passes of layer_bwd.hip, a function of n only."""
    return max(32, 4 * cdiv(n if n > 0 else 1, 4096))


def layernorm_bwd_ws_bytes(n, D):                                       # regtr_layernorm_bwd_ws_bytes
    if n <= 0 or D < 4 or D % 4 or D > LN_MAX_D:
        return 0
    return cdiv(n, bwd_chunk_rows(n)) * 2 * D * 4


def bias_relu_bwd_ws_bytes(n, N):                                       # regtr_bias_relu_bwd_ws_bytes
    if n <= 0 or N < 4 or N % 4:
        return 0
    return cdiv(n, bwd_chunk_rows(n)) * N * 4


def route_layernorm_bwd(n, D):
    """regtr_layernorm_bwd: 'ln_bwd<NG>/{full|edge}/{rows32|rowsN}'.  NG float4 column groups per lane (256 columns each); 'edge' when
    some lane's group lies outside the row (the `c < D` branches; 'full': D == 256 NG); 'rowsN' once bwd_chunk_rows leaves 32 rows per
    workgroup (n > 32768).  The rows are a kernel argument, not an instantiation: the gate holds them to be reached on their own."""
    if n < 0 or D < 4 or D % 4 or D > LN_MAX_D:
        return 'refused'
    if n == 0:
        return 'none'
    NG = 1 if D <= 256 else (2 if D <= 512 else 4)
    return f"ln_bwd<{NG}>/{'full' if D == 256 * NG else 'edge'}/{'rows32' if bwd_chunk_rows(n) == 32 else 'rowsN'}"


def bias_relu_cw(N):
    return 64 if N // 4 >= 64 else (32 if N // 4 >= 32 else 16)


def route_bias_relu_bwd(n, N, with_h):
    """regtr_bias_relu_bwd: 'bias_relu<CW>/{full|edge}/{grouped|tail_only}/{sum|relu}'.  CW float4 columns per workgroup; 'edge' when the
    last workgroup's columns are partly outside (N / 4 no multiple of CW); 'grouped' when the unrolled loop over four row groups runs its
    body for at least one thread: row lane 0 of the first chunk has r + 3 TR < r1, TR = 256 / CW, i.e. min(n, chunk rows) > 3 TR."""
    if n < 0 or N < 4 or N % 4:
        return 'refused'
    if n == 0:
        return 'none'
    CW = bias_relu_cw(N)
    TR = 256 // CW
    grouped = min(n, bwd_chunk_rows(n)) > 3 * TR
    return (f"bias_relu<{CW}>/{'full' if (N // 4) % CW == 0 else 'edge'}/{'grouped' if grouped else 'tail_only'}/"
            f"{'relu' if with_h else 'sum'}")


def route_gather_bwd(Cin, KP):
    """regtr_kpconv_gather_bwd: 'gather_bwd<LC,NC>/{full|edge}/{kp15|kp_lt|kp16}'.  LC lanes x NC channels per lane serve an entry; 'edge'
    when some lane's channel is outside (Cin < LC NC: the dummy-address steering for c >= Cin); kp_lt: KP < 15 (more than one padding
    lane of the 16 per entry), kp16: none."""
    if not 1 <= Cin <= 256 or not 1 <= KP <= KP_PAD:
        return 'refused'
    LC, NC = (1, 1) if Cin == 1 else (32, 1) if Cin <= 32 else (64, 1) if Cin <= 64 else (64, 2) if Cin <= 128 else (64, 4)
    return f"gather_bwd<{LC},{NC}>/{'full' if Cin == LC * NC else 'edge'}/{'kp15' if KP == 15 else ('kp16' if KP == 16 else 'kp_lt')}"


def nbr_transpose_ws_bytes(nq, H, ns):                                  # regtr_nbr_transpose_ws_bytes
    if nq < 0 or ns < 0 or H < 1 or nq * H >= 1 << 31:
        return 0

    def al(b):
        return (b + 255) & ~255
    return al(max(ns, 1) * 4) + al((cdiv(ns, SCAN_ITEMS) + 1) * 4) + al(max(nq, 1) * H * 4)


def route_nbr_transpose(ns):
    """regtr_nbr_transpose: 'scan/{per1|perN}' -- block sums per thread of the one-workgroup k_scan_bsums (256 threads over
    cdiv(ns, 1024) sums: perN from ns > 262144).  The launcher has no other regime: its six kernels are not templated and every launch
    size follows from (nq H, ns) alone.  'none' for an empty table (a memset only)."""
    if ns == 0:
        return 'none'
    return 'scan/per1' if cdiv(cdiv(ns, SCAN_ITEMS), 256) <= 1 else 'scan/perN'


def _tn_plan(M, tiles):
    """gemm_tn_splits / tn_any_splits -> (splits, chunk): rows per split, a multiple of 4 and at least 64, aiming at 2048 workgroups."""
    target = cdiv(2048, tiles) if tiles > 0 else 1
    chunk = max(cdiv(cdiv(M if M > 0 else 1, target), 4) * 4, 64)
    return (cdiv(M, chunk) if M > 0 else 1), chunk


def gemm_tn_plan(M, N1, N2):
    return _tn_plan(M, (N1 // TN_TILE) * (N2 // TN_TILE))


def tn_any_plan(M, N1, N2):
    return _tn_plan(M, cdiv(N1, TN_TILE) * cdiv(N2, TN_TILE))


def gemm_tn_ws_bytes(M, N1, N2):                                        # regtr_gemm_tn_ws_bytes
    if M < 0 or N1 <= 0 or N2 <= 0 or N1 % TN_TILE or N2 % TN_TILE:
        return 0
    return gemm_tn_plan(M, N1, N2)[0] * N1 * N2 * 4


def gemm_tn_any_ws_bytes(M, N1, N2):                                    # regtr_gemm_tn_any_ws_bytes
    if M < 0 or N1 <= 0 or N2 <= 0 or N1 * N2 >= 1 << 28:
        return 0
    return tn_any_plan(M, N1, N2)[0] * N1 * N2 * 4


def _tn_regime(splits, chunk):
    return 'one_split' if splits == 1 else ('chunk64' if chunk == 64 else 'chunk_scaled')


def route_gemm_tn(M, N1, N2, fold):
    """regtr_gemm_tn: 'tn/{one_split|chunk64|chunk_scaled}[/fold]' (M = 0 launches too: one split of no rows, a zero result)."""
    if M < 0 or N1 <= 0 or N2 <= 0 or N1 % TN_TILE or N2 % TN_TILE or (fold and N1 != N2):
        return 'refused'
    return 'tn/' + _tn_regime(*gemm_tn_plan(M, N1, N2)) + ('/fold' if fold else '')


def route_gemm_tn_any(M, N1, N2):
    """regtr_gemm_tn_any: 'tn_any/{one_split|chunk64|chunk_scaled}[/edge_n1][/edge_n2]', an edge where the width is no multiple of the
    64-wide tile (the a_ok / b_ok guards)."""
    if M < 0 or N1 <= 0 or N2 <= 0 or N1 * N2 >= 1 << 28:
        return 'refused'
    return ('tn_any/' + _tn_regime(*tn_any_plan(M, N1, N2)) + ('/edge_n1' if N1 % TN_TILE else '') + ('/edge_n2' if N2 % TN_TILE else ''))


def tn_last_chunk(M, plan):
    """Rows of the last split."""
    splits, chunk = plan
    return M - (splits - 1) * chunk


def route_infonce(D):
    """regtr_infonce / regtr_infonce_rows (one kernel, k_infonce<D>) and regtr_infonce_bwd's two launches k_infonce_bwd<D, anchor rows>,
    k_infonce_bwd<D, positive rows>: what InfoNCELossFull's forward + backward runs."""
    if D <= 0 or D % 64 or D > 512:
        return 'refused'
    return f'infonce<{D}>+infonce_bwd<{D},anc>+infonce_bwd<{D},pos>'


LN_BWD_KERNELS = {f'ln_bwd<{NG}>/{e}' for NG in (1, 2, 4) for e in ('full', 'edge')}
BWD_ROW_REGIMES = {'rows32', 'rowsN'}
BIAS_RELU_KERNELS = {f'bias_relu<{CW}>/{e}/{g}/{m}' for CW in (16, 32, 64) for e in ('full', 'edge') for g in ('grouped', 'tail_only')
                     for m in ('sum', 'relu')}
GATHER_BWD_KERNELS = {f'gather_bwd<{LC},{NC}>/{e}/{k}' for LC, NC in ((1, 1), (32, 1), (64, 1), (64, 2), (64, 4))
                      for e in (('full',) if LC == 1 else ('full', 'edge')) for k in ('kp15', 'kp_lt', 'kp16')}
NBR_TRANSPOSE_KERNELS = {'scan/per1', 'scan/perN'}
GEMM_TN_KERNELS = ({f'tn/{r}{f}' for r in ('one_split', 'chunk64', 'chunk_scaled') for f in ('', '/fold')}
                   | {f'tn_any/{r}' for r in ('one_split', 'chunk64', 'chunk_scaled')})
TN_ANY_EDGES = {'tn_any', 'tn_any/edge_n1', 'tn_any/edge_n2', 'tn_any/edge_n1/edge_n2'}
INFONCE_KERNELS = set().union(*(set(route_infonce(D).split('+')) for D in range(64, 513, 64)))


# ------------------------------------------------------------------------------------------------ preprocessing (csrc/preprocess.hip)
# The grid subsample, the cell grid and both radius-search kernels.  Their regimes are chosen by launch sizes (capacities, known to the
# host) and by live sizes and ball contents (known to the device only): the shape routes take both, the row regimes take numbers a
# reference supplies.  Cases in tests/test_gpu_preprocess_routes.py, universe PREPROCESS_KERNELS.
PRE_SCAN_TILE = 1024                  # SCAN_THREADS * SCAN_ITEMS
SCAN_CHAIN_TILES = 64
QUERY_WAVES = 4
SELF_CAND = 256
RQ_MAX_GRID = 256 * 64
SELF_MAX_GRID = 256 * 32
RADIUS_MAX_K = 448


def live_table(n):
    """rg_live_table: the power of two >= 1.5 n, at least 64 -- the hash-table length the kernels size on the device."""
    want = max(n + (n >> 1), 64)
    return 1 << (want - 1).bit_length()


def table_capacity(n_cap):
    """rg_table_capacity: the host twin over the capacity (the allocated table)."""
    return live_table(n_cap)


def _carve(sizes):
    """RgCarver: every array starts on a 256-byte boundary; the total is rounded up to 256 bytes."""
    off = 0
    for b in sizes:
        off = (off + 255) & ~255
        off += b
    return (off + 255) & ~255


def cellgrid_ws_bytes(ns_cap):                                          # regtr_cellgrid_ws_bytes (carve_grid + 4096)
    n = max(ns_cap, 1)
    T = table_capacity(n)
    return _carve([8 * n, 4 * n, 4 * n, 4 * T, 4 * T, 4 * T, 8 * T, 4 * T, 8 * T, 8 * T, 8 * (cdiv(T, PRE_SCAN_TILE) + 2), 16 * n,
                   32 * T]) + 4096


def umap_before_offset(base, c):                                        # rg_umap_before_offset
    return base * 11 // 5 + 16 * c


def grid_subsample_ws_bytes(n_cap, n_clouds, row_order):                # regtr_grid_subsample_ordered_ws_bytes (carve_subsample + 4096)
    n, nc = max(n_cap, 1), max(n_clouds, 1)
    T = table_capacity(n)
    sizes = [8 * n, 8 * n, 8 * n, 4 * n, 4 * n, 4 * n, 4 * T, 4 * T, 4 * T, 4 * T, 8 * (cdiv(n, PRE_SCAN_TILE) + 1), 4 * 6 * nc]
    if row_order == 1:
        sizes += [8 * n, 4 * (n + nc), 4 * (umap_before_offset(n, nc) + 16), 4 * n, 4 * n]
    return _carve(sizes) + 4096


def route_scan(items_cap):
    """scan_u64 over a capacity of items: the one-launch chained scan up to 64 tiles of 1024 ('scan/chained1': one tile, no look-back),
    else reduce / block sums / apply, k_scan_bsums taking one sum per thread ('per1', up to 256 tiles) or looping with a carry."""
    nb = cdiv(items_cap, PRE_SCAN_TILE)
    if nb <= SCAN_CHAIN_TILES:
        return 'scan/chained1' if nb <= 1 else 'scan/chained'
    return 'scan/three/per1' if nb <= 256 else 'scan/three/perN'


def route_subsample(n_cap, row_order=0):
    """regtr_grid_subsample_ordered: its scan runs over the point capacity; row_order 1 adds k_rank_keys + k_umap_order."""
    assert n_cap >= 1 and row_order in (0, 1)
    return 'sub/' + route_scan(n_cap) + ('+sub/ref_order' if row_order else '')


def route_cellgrid(ns_cap):
    """regtr_cellgrid_build: its scan runs over the allocated table (the live length stays on the device)."""
    return 'grid/' + route_scan(table_capacity(max(ns_cap, 1)))


def radius_cap(K):
    """The LDS list capacity of both radius kernels: 2 K rounded up to 64, held in [256, 512]; K + 64 must fit (K <= 448)."""
    if K < 1 or K > RADIUS_MAX_K:
        return 'refused'
    cap = min(max((2 * K + 63) // 64 * 64, 256), 512)
    assert cap >= K + 64
    return cap


def xcd_grid(nblocks):
    return (nblocks + 7) // 8 * 8


def route_radius_query(nq_cap, nq_live):
    """regtr_radius_query -> (label, trailing waves empty): min(xcd_grid(cdiv(nq_cap, 4)), 16384) workgroups of 4 waves, every wave a
    contiguous run of cdiv(nq_live, waves) queries.  Trailing waves are empty when the runs of the first waves cover the live queries."""
    assert nq_cap >= 1 and 0 <= nq_live <= nq_cap
    waves = min(xcd_grid(cdiv(nq_cap, QUERY_WAVES)), RQ_MAX_GRID) * QUERY_WAVES
    per_wave = cdiv(nq_live, waves)
    label = 'rq/per_wave1' if per_wave <= 1 else 'rq/per_waveN'
    return label, per_wave * (waves - 1) >= nq_live


def self_plan(ns_cap, ns_live):
    """k_radius_query_self -> (slots per wave and step, steps): the launch has waves for 16 slots each of the allocated table (at most
    8192 workgroups); the kernel sizes the chunk for the live table, 4 .. 64, and loops when 64 slots per wave do not cover it."""
    assert ns_cap >= 1 and 0 <= ns_live <= ns_cap
    chunks = cdiv(table_capacity(ns_cap), 16)
    waves = min(cdiv(chunks, QUERY_WAVES), SELF_MAX_GRID) * QUERY_WAVES
    T = live_table(ns_live)
    spw = 4
    while spw < 64 and spw * waves < T:
        spw <<= 1
    return spw, cdiv(T, spw * waves)


def route_radius_self(ns_cap, ns_live):
    spw, steps = self_plan(ns_cap, ns_live)
    return f"self/spw{spw}/pass{'1' if steps <= 1 else 'N'}"


# ---- the regimes of one query row, from numbers a reference supplies
def rank_path(n_listed):
    """for_each_ranked over the n keys left in the list -> (label, n % 8 == 0): two lanes per key up to 32 keys, else the general
    path over the list padded to a multiple of 8."""
    return ('rank/two_lane' if n_listed <= 32 else 'rank/general'), n_listed % 8 == 0


def shrinks(count_sequence, cap, K):
    """How often a row's list is cut back to the K best: count_sequence[i] supports of candidate round i (64 candidates) lie in the
    ball; after a round the list shrinks when it has no room for 64 more."""
    n = times = 0
    for add in count_sequence:
        n += add
        if n + 64 > cap:
            n = min(n, K)
            times += 1
    return times, n


def cell_index(x, radius):
    """cell_of, per axis: floor(double(x) * inv), inv = 1 / (double(float32 radius) * (1 + 1e-6)); a support's cell key is
    (cloud, cx, cy, cz).  Takes a scalar or a numpy array.  The tests use it to LABEL cases only, never for a result."""
    import numpy as np
    inv = 1.0 / (float(np.float32(radius)) * (1.0 + 1e-6))
    return np.floor(np.asarray(x, np.float64) * inv).astype(np.int64)


def staged(total_candidates):
    """k_radius_query_self stages the 27-cell candidates of a cell in LDS when there are at most 256 of them."""
    return 'cand/staged' if total_candidates <= SELF_CAND else 'cand/unstaged'


def row_labels(n_candidates, count_sequence, K):
    """Every data-dependent label of one row: staged or not (self kernel), shrink count with the capacity class, final rank path."""
    cap = radius_cap(K)
    times, n = shrinks(count_sequence, cap, K)
    path, mult8 = rank_path(n)
    out = {path + ('' if path == 'rank/two_lane' else ('/pad0' if mult8 else '/pad')), staged(n_candidates)}
    if times:
        capc = 'cap_limit' if cap == K + 64 else ('cap256' if cap == 256 else ('cap512' if cap == 512 else 'cap_mid'))
        out.add(f"shrink{min(times, 2)}/{capc}")
        if n_candidates > SELF_CAND:
            out.add('cand/unstaged/shrink')
    return out


_SCANS = ('scan/chained1', 'scan/chained', 'scan/three/per1', 'scan/three/perN')
PREPROCESS_SHAPE_KERNELS = ({f'sub/{s}' for s in _SCANS} | {f'grid/{s}' for s in _SCANS} | {'sub/ref_order'}
                            | {'rq/per_wave1', 'rq/per_waveN', 'rq/empty_waves'}
                            | {f'self/spw{s}/pass1' for s in (4, 8, 16, 32, 64)} | {'self/spw64/passN'})
PREPROCESS_ROW_KERNELS = ({'rank/two_lane', 'rank/general/pad0', 'rank/general/pad', 'cand/staged', 'cand/unstaged', 'cand/unstaged/shrink'}
                          | {f'shrink{t}/{c}' for t in (1, 2) for c in ('cap256', 'cap_mid', 'cap512', 'cap_limit')})
PREPROCESS_KERNELS = PREPROCESS_SHAPE_KERNELS | PREPROCESS_ROW_KERNELS


# ------------------------------------------------------------------------------------------------ the exact-f32 GEMM (csrc/gemm.hip)
F32_BK = 32


def gemm_f32_tile(N):
    """(bm, bn): the 4 x 1 wave tile for thin outputs (N <= 32), else 2 x 2."""
    return (128, 32) if N <= 32 else (64, 64)


def gemm_f32_splits(M, N, K):
    """choose_splits: the K splits asked for (1 = none): none from 384 tiles or below K = 512, else towards 768 workgroups with at least
    128 of K per split, 16 at most."""
    bm, bn = gemm_f32_tile(N)
    tiles = cdiv(M, bm) * cdiv(N, bn)
    if tiles >= 384 or K < 512:
        return 1
    s = min(cdiv(768, tiles), K // 128, 16)
    return 1 if s < 2 else s


def gemm_f32_ws_bytes(M, N, K):                                         # regtr_gemm_f32_ws_bytes
    s = gemm_f32_splits(M, N, K)
    return s * M * N * 4 if s > 1 else 0


def gemm_f32_plan(M, N, K):
    """-> (S asked, k_chunk, S_eff): the chunk is rounded up to 32, so fewer chunks than splits may cover K."""
    S = gemm_f32_splits(M, N, K)
    k_chunk = cdiv(cdiv(K, S), F32_BK) * F32_BK if S > 1 else K
    return S, k_chunk, cdiv(K, k_chunk)


def gemm_f32_fold_tags(M, N, lens):
    """Which row tiles of a folded launch lie in one cloud (one wave-parallel lookup serves the tile) and which straddle clouds (a search
    per row).  A row's cloud is the last one that starts at or before it: empty clouds own no row."""
    bm, _ = gemm_f32_tile(N)
    starts = [0]
    for n in lens:
        starts.append(starts[-1] + n)
    assert starts[-1] == M
    seg = lambda i: max(b for b in range(len(lens)) if starts[b] <= i)
    tags = set()
    for m0 in range(0, M, bm):
        tags.add('fold_one_cloud' if seg(m0) == seg(min(m0 + bm, M) - 1) else 'fold_straddle')
    return tags


def route_gemm_f32(M, N, K, lda=None, ldb=None, a_aligned16=True, b_aligned16=True, lens=None):
    """regtr_gemm_f32's launch: 'f32<ALIGNED_A,ALIGNED_B,WMW,WNW>/tag/..' and '+splitk_reduce' after a split launch; 'none' for M = 0,
    'refused' for what the launcher refuses.  Tags (regimes of one instantiation, none of them a template argument):
      nosplit | split [split_short: S_eff < S]          the launch; a split launch writes raw partials and reduces them in split order
      nk1, nk_odd, nk_even                              32-deep tiles of a chunk, over all chunks: the two-stage pipeline leaves its loop
                                                        after the even or after the odd half, and never enters the second for one tile
      ktail [ktail_lt4]                                 a chunk whose length is no multiple of 32 [its last tile holds fewer than 4 k]
      fold_one_cloud, fold_straddle                     (lens given: the folded InstanceNorm operand) see gemm_f32_fold_tags"""
    lda = K if lda is None else lda
    ldb = N if ldb is None else ldb
    if M < 0 or N < 1 or K < 1 or lda < K or ldb < N:
        return 'refused'
    if M == 0:
        return 'none'
    S, k_chunk, S_eff = gemm_f32_plan(M, N, K)
    aligned_a = K % 4 == 0 and lda % 4 == 0 and a_aligned16 and k_chunk % 4 == 0
    aligned_b = N % 4 == 0 and ldb % 4 == 0 and b_aligned16
    if N <= 32:
        k = 'f32<1,1,4,1>' if aligned_a and aligned_b else ('f32<1,0,4,1>' if aligned_a else 'f32<0,0,4,1>')
    else:
        k = 'f32<1,1,2,2>' if aligned_a and aligned_b else 'f32<0,0,2,2>'
    tags = ['nosplit'] if S_eff == 1 else (['split', 'split_short'] if S_eff < S else ['split'])
    chunks = sorted({min(k_chunk, K - s * k_chunk) for s in range(S_eff)})
    nks = {cdiv(c, F32_BK) for c in chunks}
    tags += [t for t, hit in (('nk1', 1 in nks), ('nk_odd', any(n > 1 and n % 2 for n in nks)), ('nk_even', any(n % 2 == 0 for n in nks))) if hit]
    tails = [c % F32_BK for c in chunks if c % F32_BK]
    if tails:
        tags.append('ktail')
        if any(t < 4 for t in tails):
            tags.append('ktail_lt4')
    if lens is not None:
        tags += sorted(gemm_f32_fold_tags(M, N, lens))
    return '/'.join([k] + tags) + ('+splitk_reduce' if S_eff > 1 else '')


def f32_tags(route):
    """(instantiation, set of regime tags) of a route_gemm_f32 route."""
    parts = route.split('+')[0].split('/')
    return parts[0], set(parts[1:])


F32_KERNELS = {'f32<1,1,4,1>', 'f32<1,0,4,1>', 'f32<0,0,4,1>', 'f32<1,1,2,2>', 'f32<0,0,2,2>', 'splitk_reduce'}
