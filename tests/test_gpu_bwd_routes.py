"""GPU: every instantiation and split regime the backward launchers can launch (csrc/losses.hip, csrc/layer_bwd.hip,
csrc/kpconv_bwd.hip), against float64 -- the widths beside the model's own and the row counts beyond a few hundred, which the four
*_grads files do not reach.

Every parametrized case carries the route tests/dispatch.py derives for it; tests/test_dispatch_routes.py cross-checks the routes and
fails when an instantiation of a backward universe (dispatch.LN_BWD_KERNELS, BIAS_RELU_KERNELS, GATHER_BWD_KERNELS,
NBR_TRANSPOSE_KERNELS, GEMM_TN_KERNELS, INFONCE_KERNELS) is reached by no case.  Outputs go into sentinel-filled buffers with guard rows
past the last row (and a wider leading dimension where the entry point takes one).  Bars: err <= the restatement's per-element bound and
max err <= 1e-4 max |ref|; where the arithmetic is exact in float32 (integer-valued operands, IEEE division, per-operation rounding)
the result must equal the restatement bit for bit.  Every test prints its worst err / bound and flat ratio; docs/PARITY.md has them."""
import numpy as np
import pytest
import torch

from tests import cross_encoder_grads_ref as CR
from tests import kpconv_grads_ref as KR

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24
FLAT = 1e-4
SENTINEL = 777.0
ISENTINEL = -777
GUARD = 5


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def _lib():
    from regtr_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device='cuda')


def _ratio(err, bound):
    """max err / bound; a zero bound (exact zeros) admits a zero error only."""
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max())


def _flat(err, ref):
    return float(err.max() / max(np.abs(ref).max(), 1e-300)) if err.size else 0.0


# ------------------------------------------------------------------------------------------------ InfoNCE: the other five widths
INFONCE_SIZES = [(1, 1), (1, 40), (40, 1), (300, 77), (33, 129), (130, 257)]


@pytest.mark.parametrize('D,route', [(D, f'infonce<{D}>+infonce_bwd<{D},anc>+infonce_bwd<{D},pos>') for D in (128, 192, 320, 384, 448)])
def test_infonce_widths_vs_float64(D, route):
    """Forward (regtr_infonce with rows, sentinel-bounded outputs) against _infonce_ref, gradients (InfoNCELossFull) against
    loss_grads_ref.infonce_grads: the assertions of the D = 64 / 256 / 512 tests."""
    from tests.test_gpu_loss_grads import infonce_grads_case
    from tests.test_gpu_losses import R_N, R_P, _infonce_ref, _make_pairs, _pack, _run_infonce
    rng = np.random.default_rng(300 + D)
    pairs = _make_pairs(rng, INFONCE_SIZES, D)
    A, P, ax, px, a_off, p_off = _pack(pairs)
    po, rl, rm = _run_infonce(A, P, ax, px, a_off, p_off, R_P, R_N)
    worst = 0.0
    for b, (Ab, Pb, axb, pxb) in enumerate(pairs):
        loss, mask, bound = _infonce_ref(Ab, Pb, axb, pxb, R_P, R_N)
        sl = slice(a_off[b], a_off[b + 1])
        assert np.array_equal(rm[sl], mask.astype(F32)), f'pair {b}: mask'
        err = np.abs(rl[sl].astype(np.float64) - loss)
        assert np.all(err <= bound), (b, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        assert po[b, 1] == mask.sum(), b
        assert abs(po[b, 0] - loss[mask].sum()) <= bound[mask].sum() + 4 * U * np.abs(loss[mask]).sum() * len(loss) + 1e-5, b
    nan_pair, zero_pair = len(pairs) - 3, len(pairs) - 2
    assert po[nan_pair, 1] == 0 and po[nan_pair, 0] == 0
    assert np.all(rl[a_off[zero_pair]:a_off[zero_pair + 1]] == 0.0)
    n_pairs, worst_g = infonce_grads_case(np.random.default_rng(400 + D), INFONCE_SIZES, D)
    print(f'infonce D={D}: {n_pairs} pairs, forward worst err/bound {worst:.3f}, grads worst err/bound {worst_g:.3f}')


# ------------------------------------------------------------------------------------------------ layernorm_bwd
LN_FORMS = {4: 'ln_bwd<1>/edge', 68: 'ln_bwd<1>/edge', 252: 'ln_bwd<1>/edge', 260: 'ln_bwd<2>/edge', 512: 'ln_bwd<2>/full',
            516: 'ln_bwd<4>/edge', 1020: 'ln_bwd<4>/edge', 1024: 'ln_bwd<4>/full'}
LN_CASES = ([(n, D, LN_FORMS[D] + '/rows32') for D in LN_FORMS for n in (1, 5, 257)]
            + [(32769, 64, 'ln_bwd<1>/edge/rowsN'), (4099, 1024, 'ln_bwd<4>/full/rows32')])


@pytest.mark.parametrize('n,D,route', LN_CASES)
def test_layernorm_bwd_vs_float64(n, D, route):
    from regtr_amd import ops
    rng = np.random.default_rng(1000 * D + n)
    x, dy, dres = (rng.normal(0, 1, (n, D)).astype(F32) for _ in range(3))
    gamma = rng.normal(1, 0.1, D).astype(F32)
    worst = {}
    for with_dres in (False, True):
        r = CR.layernorm_bwd(x, gamma, dy, dres if with_dres else None)
        buf = torch.full((n + GUARD, D), SENTINEL, device='cuda')
        dx, dg, db = ops.layernorm_bwd(_dev(x), _dev(gamma), _dev(dy), dres=_dev(dres) if with_dres else None, out=buf[:n])
        torch.cuda.synchronize()
        assert dx.data_ptr() == buf.data_ptr() and torch.all(buf[n:] == SENTINEL), 'rows past n were written'
        for name, got in (('dx', dx), ('dgamma', dg), ('dbeta', db)):
            got = got.double().cpu().numpy()
            assert np.all(np.isfinite(got)), name
            err = np.abs(got - r[name])
            ratio, flat = _ratio(err, r['b_' + name]), _flat(err, r[name])
            worst[name] = tuple(max(a, b) for a, b in zip(worst.get(name, (0.0, 0.0)), (ratio, flat)))
            assert ratio <= 1.0 and flat <= FLAT, (with_dres, name, ratio, flat)
    print(f'layernorm_bwd n={n} D={D} {route}: ' + ', '.join(f'{k} err/bound {v[0]:.3f} flat {v[1]:.2e}' for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ bias_relu_bwd
def _br_form(N):
    cw = 64 if N >= 256 else (32 if N >= 128 else 16)
    return f"bias_relu<{cw}>/{'full' if N % (4 * cw) == 0 else 'edge'}", 256 // cw


# (n, N, route of the call without h); the call with h has '/relu' in place of '/sum'.  'grouped': n (or 52, the chunk of 49153 rows)
# beyond three times the row lanes.  N = 60 at 49153 rows is what reaches the narrow kernel's grouped loop on an edge workgroup; the
# full-width forms at few rows (N = 64, 768, 1024) are tests/test_gpu_cross_encoder_grads.py's.
BR_CASES = ([(n, N, f"{_br_form(N)[0]}/{'grouped' if min(n, 32) > 3 * _br_form(N)[1] else 'tail_only'}/sum")
             for N in (4, 60, 68, 128, 132, 252, 260) for n in (1, 5, 257, 4099)]
            + [(49153, N, f'{_br_form(N)[0]}/grouped/sum') for N in (60, 64, 128)])
BR_PAD = 16


@pytest.mark.parametrize('kind', ['normal', 'exact'])
@pytest.mark.parametrize('n,N,route', BR_CASES)
def test_bias_relu_bwd_vs_float64(n, N, route, kind):
    """kind 'exact': g integer-valued in [-3, 3] -- every partial and total sum is an exact float32 integer (at most 3 x 49153 < 2^24), so
    db must equal the float64 sum bit for bit: no row dropped, repeated or misplaced."""
    from regtr_amd import ops
    rng = np.random.default_rng(7 * N + n + (0 if kind == 'normal' else 1))
    shape = (n + GUARD, N + 2 * BR_PAD)
    wide = (rng.normal(0, 1, shape) if kind == 'normal' else rng.integers(-3, 4, shape)).astype(F32)
    h = np.maximum(rng.normal(0, 1, (n, N)), 0).astype(F32)                   # exact zeros where the ReLU cut
    h[0, :4] = [0.0, -0.0, 1e-30, -1.0]
    g_np = wide[:n, BR_PAD:BR_PAD + N]
    worst = (0.0, 0.0)

    def check_db(db, r, what):
        nonlocal worst
        got = db.double().cpu().numpy()
        if kind == 'exact':
            assert np.array_equal(got, r['db']), (what, int(np.abs(got - r['db']).max()))
            return
        err = np.abs(got - r['db'])
        ratio, flat = _ratio(err, r['b_db']), _flat(err, r['db'])
        worst = (max(worst[0], ratio), max(worst[1], flat))
        assert ratio <= 1.0 and flat <= FLAT, (what, ratio, flat)

    for strided in (False, True):
        make_g = lambda: _dev(wide)[:n, BR_PAD:BR_PAD + N] if strided else _dev(g_np.copy())
        check_db(ops.bias_relu_bwd(make_g()), CR.bias_relu_bwd(g_np), ('sum', strided))
        r = CR.bias_relu_bwd(g_np, h)
        for inplace in (False, True):
            g = make_g()
            dh, db = ops.bias_relu_bwd(g, _dev(h), inplace=inplace)
            torch.cuda.synchronize()
            assert (dh.data_ptr() == g.data_ptr()) == inplace
            assert np.array_equal(dh.cpu().numpy(), r['dh'].astype(F32)), 'dh is a selection: exact'
            assert torch.all(dh[_dev(h) == 0] == 0) and not torch.signbit(dh[_dev(h) <= 0]).any()
            check_db(db, r, ('relu', strided, inplace))
            if strided and inplace:                           # the columns beside g and the guard rows below it are untouched
                base = g._base.cpu().numpy()
                assert np.array_equal(base[:, :BR_PAD], wide[:, :BR_PAD]) and np.array_equal(base[:, BR_PAD + N:], wide[:, BR_PAD + N:])
                assert np.array_equal(base[n:], wide[n:])
    print(f'bias_relu_bwd n={n} N={N} {kind} {route}: ' + ('db bit-exact' if kind == 'exact' else f'err/bound {worst[0]:.3f} flat {worst[1]:.2e}'))


# ------------------------------------------------------------------------------------------------ kpconv_gather_bwd
GB_NS, GB_H, GB_RADIUS = 203, 21, 0.30
_GB = {}


def _gb_geometry():
    """One table for every case, drawn as kpconv_grads_ref.draw_case draws its own: Ns = Nq = 203 points in the unit cube, H = 21 nearest
    within 0.30; support 3 put into EVERY row (a hub: in-degree 203, beyond one wave's 64 entries), support 5 removed from every row (an
    orphan); 16 kernel points (the centre and 15 directions at 0.6 R, influence radius 0.5 R), of which a case takes the first KP."""
    if not _GB:
        rng = np.random.default_rng(46)
        s_pts = rng.uniform(0, 1, (GB_NS, 3)).astype(F32)
        nbr = KR._edit_rows(KR.neighbours(s_pts, s_pts, GB_RADIUS, GB_H), GB_NS, drop=KR.ORPHAN, first=KR.HUB)
        v = rng.normal(0, 1, (16, 3))
        kp = 0.6 * GB_RADIUS * v / np.linalg.norm(v, axis=1, keepdims=True)
        kp[0] = 0
        deg = np.diff(KR.transpose_table(nbr, GB_NS)[0])
        assert deg[KR.HUB] == GB_NS > 64 and deg[KR.ORPHAN] == 0 and (nbr == GB_NS).any()
        _GB.update(s_pts=s_pts, nbr=nbr, kp=kp.astype(F32), extent=float(F32(0.5 * GB_RADIUS)), deg=deg)
    return _GB


def _gb_rung(Cin):
    lc, nc = (32, 1) if Cin <= 32 else (64, 1) if Cin <= 64 else (64, 2) if Cin <= 128 else (64, 4)
    return f"gather_bwd<{lc},{nc}>/{'full' if Cin == lc * nc else 'edge'}"


GB_KP = {1: 'kp_lt', 7: 'kp_lt', 15: 'kp15', 16: 'kp16'}
GB_CASES = ([(Cin, 15, _gb_rung(Cin) + '/kp15') for Cin in (2, 17, 31, 33, 48, 65, 96, 127, 129, 192, 255)]
            + [(Cin, KP, f'{_gb_rung(Cin)}/{GB_KP[KP]}') for Cin in (32, 96) for KP in (1, 7, 16)]
            + [(1, KP, f'gather_bwd<1,1>/full/{GB_KP[KP]}') for KP in (7, 16)]
            + [(Cin, KP, f'{_gb_rung(Cin)}/{GB_KP[KP]}') for Cin in (17, 48, 64, 128, 192, 256) for KP in (7, 16)])


@pytest.mark.parametrize('Cin,KP,route', GB_CASES)
def test_gather_bwd_widths_vs_float64(Cin, KP, route):
    from regtr_amd import ops
    c = _gb_geometry()
    ns, kp = GB_NS, c['kp'][:KP]
    dwf = np.random.default_rng(100 * Cin + KP).normal(0, 1, (ns, KP, Cin)).astype(F32)
    table = ops.nbr_transpose(_dev(c['nbr'], torch.int32), ns)
    buf = torch.full((ns + GUARD, Cin), SENTINEL, dtype=torch.float32, device='cuda')
    args = (_dev(dwf.reshape(ns, -1)), _dev(c['s_pts']), _dev(c['s_pts']), GB_H, _dev(kp), c['extent'], table)
    dx = ops.kpconv_gather_bwd(*args, out=buf[:ns])
    again = ops.kpconv_gather_bwd(*args)
    torch.cuda.synchronize()
    assert dx.data_ptr() == buf.data_ptr() and torch.equal(dx, again)      # bit equality of two calls
    got = buf.cpu().numpy()
    assert np.all(got[ns:] == SENTINEL)                                    # nothing past row Ns
    assert np.all(np.isfinite(got[:ns]))
    ref, bound = KR.gather_bwd(c['s_pts'], c['s_pts'], c['nbr'], kp, c['extent'], dwf, ns)
    err = np.abs(got[:ns].astype(np.float64) - ref)
    ratio, flat = _ratio(err, bound), _flat(err, ref)
    print(f'kpconv_gather_bwd Cin={Cin} KP={KP} {route}: err/bound {ratio:.4f} flat {flat:.2e}')
    assert ratio <= 1.0 and flat <= FLAT, (ratio, flat)
    zero = got[:ns][c['deg'] == 0]
    assert len(zero) and np.all(zero == 0) and not np.signbit(zero).any()  # the orphan: an exact +0 row


# ------------------------------------------------------------------------------------------------ nbr_transpose
@pytest.mark.parametrize('ns,nq,H,route', [(1024, 3000, 5, 'scan/per1'), (4096, 3000, 5, 'scan/per1'), (300001, 20000, 5, 'scan/perN')])
def test_nbr_transpose_scan_regimes(ns, nq, H, route):
    """Indices uniform over [-1, ns]: shadows on both sides.  ns = 1024: the total is written by the last thread of a full workgroup;
    ns = 300001: more than one block sum per thread of the block-sum scan."""
    L = _lib()
    nbr = np.random.default_rng(ns).integers(-1, ns + 1, (nq, H)).astype(np.int32)
    nbr[0, 0], nbr[nq - 1, H - 1], nbr[nq // 2, 1] = -1, ns, ns - 1         # both shadows and the last support, whatever was drawn
    ref_off, ref_ent = KR.transpose_table(nbr, ns)
    t_nbr = _dev(nbr, torch.int32)
    nb = L.regtr_nbr_transpose_ws_bytes(nq, H, ns)
    outs = []
    for _ in range(2):
        row_off = torch.full((ns + 1 + GUARD,), ISENTINEL, dtype=torch.int32, device='cuda')
        ent = torch.full((nq * H + GUARD,), ISENTINEL, dtype=torch.int32, device='cuda')
        ws = _ws(nb)
        assert L.regtr_nbr_transpose(t_nbr.data_ptr(), nq, H, ns, row_off.data_ptr(), ent.data_ptr(), ws.data_ptr(), nb, _stream()) == 0
        torch.cuda.synchronize()
        outs.append((row_off.cpu().numpy(), ent.cpu().numpy()))
    (row_off, ent), (row_off2, ent2) = outs
    assert np.array_equal(row_off[:ns + 1], ref_off) and np.all(row_off[ns + 1:] == ISENTINEL)
    assert np.array_equal(ent[:len(ref_ent)], ref_ent) and np.all(ent[len(ref_ent):] == ISENTINEL)   # nothing past row_off[ns]
    assert np.array_equal(row_off, row_off2) and np.array_equal(ent, ent2)
    print(f'nbr_transpose ns={ns} ({nq}, {H}) {route}: {len(ref_ent)} entries, exact')


# ------------------------------------------------------------------------------------------------ gemm_tn, gemm_tn_any
TN_MS = (0, 1, 3, 4, 64, 65, 203)
TN_EDGES = {(64, 64): '', (256, 256): '', (15, 64): '/edge_n1', (64, 50): '/edge_n2', (480, 32): '/edge_n1/edge_n2',
            (70, 50): '/edge_n1/edge_n2', (130, 17): '/edge_n1/edge_n2', (480, 96): '/edge_n1/edge_n2'}


def _tn_cases():
    out = []
    for (N1, N2), edge in TN_EDGES.items():
        if (N1, N2) == (480, 96):
            continue
        for M in TN_MS:
            regime = 'one_split' if M <= 64 else 'chunk64'
            if not edge:
                out += [('tn', M, N1, N2, f'tn/{regime}'), ('tn_fold', M, N1, N2, f'tn/{regime}/fold')]
            out.append(('tn_any', M, N1, N2, f'tn_any/{regime}{edge}'))
    # the scaled-chunk regime: 68 rows per split, a last split of 37 (8197 rows) or 41 (131077) rows
    out += [('tn', 8197, 256, 256, 'tn/chunk_scaled'), ('tn_fold', 8197, 256, 256, 'tn/chunk_scaled/fold'),
            ('tn_any', 8197, 256, 256, 'tn_any/chunk_scaled'), ('tn_any', 8197, 480, 96, 'tn_any/chunk_scaled/edge_n1/edge_n2'),
            ('tn_any', 131077, 15, 64, 'tn_any/chunk_scaled/edge_n1')]
    return out


TN_CASES = _tn_cases()


def _run_tn(kind, a, b):
    """The entry point on host operands, into an (N1 + GUARD, N2 + 8) sentinel buffer -> the (N1, N2) result, numpy."""
    L = _lib()
    M, N1 = a.shape
    N2 = b.shape[1]
    ldo = N2 + 8
    ta, tb = (_dev(a), _dev(b)) if M else (None, None)
    pa, pb = (ta.data_ptr(), tb.data_ptr()) if M else (None, None)
    buf = torch.full((N1 + GUARD, ldo), SENTINEL, dtype=torch.float32, device='cuda')
    if kind == 'tn_any':
        nb = L.regtr_gemm_tn_any_ws_bytes(M, N1, N2)
        ws = _ws(nb)
        rc = L.regtr_gemm_tn_any(pa, N1, pb, N2, M, N1, N2, buf.data_ptr(), ldo, ws.data_ptr(), nb, _stream())
    else:
        nb = L.regtr_gemm_tn_ws_bytes(M, N1, N2)
        ws = _ws(nb)
        rc = L.regtr_gemm_tn(pa, N1, pb, N2, M, N1, N2, int(kind == 'tn_fold'), buf.data_ptr(), ldo, ws.data_ptr(), nb, _stream())
    assert rc == 0 and nb > 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[N1:] == SENTINEL) and np.all(got[:, N2:] == SENTINEL), 'write outside the (N1, N2) result'
    return got[:N1, :N2]


@pytest.mark.parametrize('kind,M,N1,N2,route', TN_CASES)
def test_gemm_tn_vs_float64(kind, M, N1, N2, route):
    """Exact run: integer operands in [-3, 3]; every sum stays below 9 x 131077 < 2^24 (twice that folded), so the result must equal the
    float64 product bit for bit, the fold's triangle rules and exact zeros below the diagonal included.  Bound run: N(0, 1) operands
    under (M + C_DW) U |a|^T |b| (kpconv_grads_ref's form for dW: M chain terms, the float64 combination of the splits, the final
    rounding; its allowance for g's rounding, unused by a direct call, is the fold's one float32 addition) and the flat 1e-4 bar.
    The fold: dW_ij = C_ij + C_ji above the diagonal, 2 C_ii on it, 0 below = triu(C + C^T)."""
    rng = np.random.default_rng(M + 1000 * N1 + N2)
    fold = lambda c: np.triu(c + c.T) if kind == 'tn_fold' else c
    ratio = flat = 0.0
    for exact in (True, False):
        if exact:
            a, b = (rng.integers(-3, 4, (M, n)).astype(F32) for n in (N1, N2))
        else:
            a, b = (rng.normal(0, 1, (M, n)).astype(F32) for n in (N1, N2))
        got, again = _run_tn(kind, a, b), _run_tn(kind, a, b)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), 'two calls differ'
        ref = fold(a.astype(np.float64).T @ b.astype(np.float64))
        if M == 0:
            assert np.all(got == 0)
        if kind == 'tn_fold':
            low = got[np.tril_indices(N1, -1)]
            assert np.all(low == 0) and not np.signbit(low).any()
        if exact:
            assert np.array_equal(got.astype(np.float64), ref), int(np.abs(got - ref).max())
            continue
        bound = (M + KR.C_DW) * U * fold(np.abs(a).astype(np.float64).T @ np.abs(b).astype(np.float64))
        err = np.abs(got.astype(np.float64) - ref)
        ratio, flat = _ratio(err, bound), (_flat(err, ref) if M else 0.0)
        assert ratio <= 1.0 and flat <= FLAT, (ratio, flat)
    print(f'gemm_tn {kind} M={M} ({N1}, {N2}) {route}: integer run bit-exact, err/bound {ratio:.3f} flat {flat:.2e}')


# ------------------------------------------------------------------------------------------------ row_div, corr_l1_bwd, se3_transform
POINT_NS = [0, 1, 255, 257, 1000]


def _seven_clouds(n):
    """seg_off (8,) int32 of seven clouds holding n rows: the first, the middle one and the last are empty, the rows go to the other four
    as evenly as they divide (n < 4 leaves more of them empty)."""
    lens = [0] * 7
    for k, c in enumerate((1, 2, 4, 5)):
        lens[c] = n // 4 + (k < n % 4)
    assert sum(lens) == n
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def _poses(rng, stride):
    """(7, 3, 4) or (7, 4, 4) float32: a different matrix per cloud; the fourth row of the 16-float form is never read."""
    T = rng.normal(0, 1, (7, 4, 4)).astype(F32)
    T[:, 3] = [0, 0, 0, 1]
    return np.ascontiguousarray(T if stride == 16 else T[:, :3])


def _transform_clouds(T, seg, x):
    from tests.test_gpu_losses import _transform_f32
    out = np.zeros((len(x), 3), F32)
    for c in range(7):
        out[seg[c]:seg[c + 1]] = _transform_f32(T[c][:3], x[seg[c]:seg[c + 1]])
    return out


@pytest.mark.parametrize('n', POINT_NS)
def test_row_div_is_ieee_division(n):
    L = _lib()
    rng = np.random.default_rng(50 + n)
    N, ldx, ldo = 45, 48, 52
    x = rng.normal(0, 1, (max(n, 1), ldx)).astype(F32)
    div = rng.integers(1, 40, max(n, 1)).astype(F32)
    buf = torch.full((n + GUARD, ldo), SENTINEL, dtype=torch.float32, device='cuda')
    tx, td = _dev(x), _dev(div)
    assert L.regtr_row_div(tx.data_ptr(), ldx, td.data_ptr(), n, N, buf.data_ptr(), ldo, _stream()) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[n:] == SENTINEL) and np.all(got[:, N:] == SENTINEL)
    assert np.array_equal(got[:n, :N], (x[:n, :N] / div[:n, None]).astype(F32))
    print(f'row_div n={n}: equals float32 division exactly')


@pytest.mark.parametrize('stride', [12, 16])
@pytest.mark.parametrize('n', POINT_NS)
def test_se3_transform_is_per_operation_float32(n, stride):
    L = _lib()
    rng = np.random.default_rng(60 + n)
    seg, T = _seven_clouds(n), _poses(rng, stride)
    x = rng.uniform(-2, 2, (max(n, 1), 3)).astype(F32)
    buf = torch.full((n + GUARD, 3), SENTINEL, dtype=torch.float32, device='cuda')
    tx, ts, tT = _dev(x), _dev(seg, torch.int32), _dev(T)
    assert L.regtr_se3_transform(tx.data_ptr(), ts.data_ptr(), 7, n, tT.data_ptr(), stride, buf.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[n:] == SENTINEL)
    assert np.array_equal(got[:n], _transform_clouds(T, seg, x[:n]))
    print(f'se3_transform n={n} stride={stride}: equals the per-operation float32 restatement exactly')


@pytest.mark.parametrize('stride', [12, 16])
@pytest.mark.parametrize('n', POINT_NS)
def test_corr_l1_bwd_is_exact(n, stride):
    """d warped = ((g / den) w) sgn(e), e = warped - T kp, every operation rounded to float32; e == 0 -> 0."""
    L = _lib()
    rng = np.random.default_rng(70 + n)
    seg, T = _seven_clouds(n), _poses(rng, stride)
    kp = rng.uniform(-2, 2, (max(n, 1), 3)).astype(F32)
    tkp = _transform_clouds(T, seg, kp[:n])
    warped = kp.copy()
    warped[:n] = (tkp + rng.normal(0, 0.1, (n, 3))).astype(F32)
    warped[:n:3] = tkp[::3]                                   # e == 0 on every third row
    w = rng.uniform(0, 1, max(n, 1)).astype(F32)
    w[1::4] = 0.0
    g, den = F32(-0.37), F32(w[:n].sum() if n else 1.0)
    buf = torch.full((n + GUARD, 3), SENTINEL, dtype=torch.float32, device='cuda')
    t = [_dev(kp), _dev(warped), _dev(w), _dev(seg, torch.int32), _dev(T), _dev(np.array([g])), _dev(np.array([den]))]
    assert L.regtr_corr_l1_bwd(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 7, n, t[4].data_ptr(), stride,
                               t[5].data_ptr(), t[6].data_ptr(), buf.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[n:] == SENTINEL)
    e = (warped[:n] - tkp).astype(F32)
    sw = ((g / den).astype(F32) * w[:n]).astype(F32)
    ref = (sw[:, None] * np.sign(e)).astype(F32)
    assert n == 0 or (e == 0).any()
    assert np.array_equal(got[:n], ref) and np.all(got[:n][e == 0] == 0)
    print(f'corr_l1_bwd n={n} stride={stride}: equals the float32 restatement exactly')
