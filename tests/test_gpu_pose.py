"""GPU (-m gpu): the two kernels that turn conditioned features into the pose, against float64 on the same float32 inputs.

k_attn_xyz (csrc/attention.hip, CorrespondenceDecoder.simple_attention): softmax(q k^T / sqrt(D)) @ xyz_partner for every head dimension
it is instantiated for, at the 32-row tile edges, with empty clouds, peaked and tied scores and coordinates far from the origin.  The bound
is per row (attn_bound); tests/test_pose_bounds_host.py shows on the CPU that it catches a kernel that drops one key or reads the wrong cloud.

k_procrustes (csrc/procrustes.hip, the weighted Kabsch of RegTR.forward and se3.compute_rigid_transform): exact motions, repeated and
vanishing singular values, zero covariances, saturated and clamped weights, pair sizes around the 256-thread stride, the non-finite pose
status bit, and the branch of RegTR.forward that reacts to it.  Poses are compared within C u kappa scale (pose_bound); where the rotation
is not unique (rank-deficient covariances) the weighted objective is compared with the float64 optimum instead.

Case builders and references are CPU-only: this module imports without a GPU (tests/test_dispatch_routes.py reads its parameters)."""
import logging
import math

import numpy as np
import pytest
import torch

U32 = 2.0 ** -24
C_ATTN = 8           # attn_bound's constant
C_POSE = 16          # pose_bound's constant
STATUS_NONFINITE_POSE = 2      # include/regtr_hip.h REGTR_STATUS_NONFINITE_POSE
RG_ERR_ARG = -2


def _seg(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ coordinate attention: cases
def _cross(lens):
    B = len(lens) // 2
    return [B + c if c < B else c - B for c in range(2 * B)]


def _many_pairs(n, seed):
    g = np.random.default_rng(seed)
    return [int(x) for x in g.integers(1, 70, 2 * n)]


# (name, head_dim, lens, kv_of, layers, kind, route); kind shapes the scores / coordinates (attn_case)
ATTN_CASES = [
    ('tiny', 32, [1, 31], [1, 0], 1, 'plain', 'attn_xyz<32>'),
    ('edge32', 64, [32, 33], [1, 0], 2, 'plain', 'attn_xyz<64>'),
    ('edges', 128, [63, 64, 65, 1], [2, 3, 0, 1], 6, 'plain', 'attn_xyz<128>'),
    ('long_short', 256, [1037, 65], [1, 0], 2, 'plain', 'attn_xyz<256>'),
    ('self', 128, [33, 1001], [0, 1], 1, 'plain', 'attn_xyz<128>'),
    ('many_to_one', 32, [31, 64, 65], [2, 2, 0], 2, 'plain', 'attn_xyz<32>'),
    ('pairs42', 64, _many_pairs(42, 3), _cross([0] * 84), 2, 'plain', 'attn_xyz<64>'),
    ('peak_last', 256, [65, 1001], [1, 0], 2, 'peak_last', 'attn_xyz<256>'),
    ('peak_first', 32, [1001, 97], [1, 0], 2, 'peak_first', 'attn_xyz<32>'),
    ('peak_last64', 64, [40, 95], [1, 0], 6, 'peak_last', 'attn_xyz<64>'),
    ('ties', 64, [65, 97], [1, 0], 2, 'ties', 'attn_xyz<64>'),
    ('ties256', 256, [33, 32], [1, 0], 1, 'ties', 'attn_xyz<256>'),
    ('offset', 128, [300, 257], [1, 0], 2, 'offset', 'attn_xyz<128>'),
    ('empty_partner', 32, [40, 70, 0, 33], [2, 3, 0, 1], 2, 'plain', 'attn_xyz<32>'),
    ('empty_query', 256, [0, 31, 64, 5], [2, 3, 0, 1], 1, 'plain', 'attn_xyz<256>'),
]
ATTN_IDS = [c[0] for c in ATTN_CASES]


def attn_case(name, head_dim, lens, kv, layers, kind):
    """float32 q, k (L, N, D) and xyz (N, 3) for a case; scores q.k / sqrt(D) of order 1-3 unless the kind says otherwise."""
    g = torch.Generator().manual_seed(sum(map(ord, name)) + head_dim)
    N, D = sum(lens), head_dim
    seg = _seg(lens)
    q = torch.randn(layers, N, D, generator=g) * 1.2
    k = torch.randn(layers, N, D, generator=g)
    xyz = (torch.rand(N, 3, generator=g) - 0.5) * 4
    if kind in ('peak_last', 'peak_first'):
        # one key of every partner cloud aligned with every query of the attending cloud: |score| up to ~80, its arg-max in the last partial
        # (or the first) 32-row key tile
        for c, kc in enumerate(kv):
            nq, nk = lens[c], lens[kc]
            if nq == 0 or nk == 0:
                continue
            j = seg[kc] + (nk - 1 - (nk % 32) // 2 if kind == 'peak_last' else 5 % nk)
            d = torch.randn(layers, D, generator=g)
            d = d / d.norm(dim=-1, keepdim=True)
            k[:, j] = d * math.sqrt(D) * 9
            q[:, seg[c]:seg[c + 1]] = d[:, None, :] * torch.linspace(-9, 9, nq)[None, :, None] + 0.05 * q[:, seg[c]:seg[c + 1]]
    elif kind == 'ties':
        # q rows constant, k in {-1, 0, 1}: every score is an exact multiple of the row's q * scale, and many keys tie exactly
        q = (torch.randint(-8, 9, (layers, N, 1), generator=g).float() / 8 * 12 / math.sqrt(D)).expand(layers, N, D).contiguous()
        k = torch.randint(-1, 2, (layers, N, D), generator=g).float()
    elif kind == 'offset':
        xyz = xyz + torch.tensor([1000.0, -1000.0, 1000.0])
        q = q * 2.0
    return q.contiguous(), k.contiguous(), xyz.contiguous()


def attn_ref(q, k, xyz, lens, kv, drop=None, keys_of=None):
    """float64 softmax(q k^T / sqrt(D)) @ xyz per (layer, cloud); empty partner -> zeros.  drop: {key cloud: key row (absolute)} removed;
    keys_of: a kv_of to read the keys and coordinates from instead (the wrong-cloud defect)."""
    L, N, D = q.shape
    seg = _seg(lens)
    q64, k64, x64 = q.double(), k.double(), xyz.double()
    out = torch.zeros(L, N, 3, dtype=torch.float64)
    src = kv if keys_of is None else keys_of
    for c, kc in enumerate(src):
        if lens[c] == 0 or lens[kc] == 0:
            continue
        rows = torch.arange(seg[kc], seg[kc + 1])
        if drop is not None and kc in drop:
            rows = rows[rows != drop[kc]]
            if len(rows) == 0:
                continue
        s = q64[:, seg[c]:seg[c + 1]] @ k64[:, rows].transpose(1, 2) / math.sqrt(D)
        out[:, seg[c]:seg[c + 1]] = torch.softmax(s, -1) @ x64[rows]
    return out


def attn_bound(q, k, xyz, lens, kv, ref):
    """Per-row bound on |out - ref| (max over x, y, z):
        C_ATTN u [ (A + 1) max_s |xyz_s - out| + sqrt(n_k) max_s |xyz_s| ]
    A = max_s sum_d |q_d k_sd| / sqrt(D) bounds the float32 rounding of every score (the kernel rounds q / sqrt(D), accumulates D products,
    and the reference's scale is exact); a score error d_s moves a convex combination by sum_s p_s (d_s - d_mean)(xyz_s - out), and the
    + 1 takes the rounding of exp into the same term.  The second term is the float32 accumulation of the n_k-term sums of p and p xyz
    (including the online-softmax rescales), whose rounding adds like a random walk.  Rows of an empty partner: 0 (exact zeros)."""
    L, N, D = q.shape
    seg = _seg(lens)
    bound = torch.zeros(L, N, dtype=torch.float64)
    q64, k64, x64 = q.double(), k.double(), xyz.double()
    for c, kc in enumerate(kv):
        if lens[c] == 0 or lens[kc] == 0:
            continue
        ks = slice(seg[kc], seg[kc + 1])
        A = (q64[:, seg[c]:seg[c + 1]].abs() @ k64[:, ks].abs().transpose(1, 2)).amax(-1) / math.sqrt(D)      # (L, nq)
        spread = (x64[ks][None, None] - ref[:, seg[c]:seg[c + 1], None]).abs().amax((-1, -2))                  # (L, nq)
        xmax = x64[ks].abs().max()
        bound[:, seg[c]:seg[c + 1]] = C_ATTN * U32 * ((A + 1) * spread + math.sqrt(lens[kc]) * xmax)
    return bound


def attn_ratio(out, ref, bound, lens, kv):
    """max over rows of |out - ref| / bound; rows of an empty partner must be exact zeros."""
    seg = _seg(lens)
    err = (out.double() - ref).abs().amax(-1)
    zero = torch.zeros(out.shape[1], dtype=torch.bool)
    for c, kc in enumerate(kv):
        if lens[kc] == 0:
            zero[seg[c]:seg[c + 1]] = True
    assert (out[:, zero] == 0).all(), 'rows of an empty partner cloud are not exact zeros'
    live = ~zero
    if not live.any():
        return 0.0
    return (err[:, live] / bound[:, live]).max().item()


def attn_defects(q, k, xyz, lens, kv, ref):
    """float64 outputs of two subtly wrong kernels: one that drops, for every partner cloud, the key of its last (partial) 32-row tile that
    carries the most attention, and one that reads keys / coordinates from the query cloud itself (kv_of ignored; None for self-attention)."""
    seg = _seg(lens)
    L, N, D = q.shape
    drop = {}
    for kc in sorted(set(kv)):
        nk = lens[kc]
        if nk == 0 or not any(kv[c] == kc and lens[c] for c in range(len(kv))):
            continue
        t0 = seg[kc] + (nk - 1) // 32 * 32
        mass = torch.zeros(seg[kc + 1] - t0, dtype=torch.float64)
        for c in range(len(kv)):
            if kv[c] == kc and lens[c]:
                s = q.double()[:, seg[c]:seg[c + 1]] @ k.double()[:, t0:seg[kc + 1]].transpose(1, 2)
                sf = q.double()[:, seg[c]:seg[c + 1]] @ k.double()[:, seg[kc]:seg[kc + 1]].transpose(1, 2)
                lse = torch.logsumexp(sf / math.sqrt(D), -1, keepdim=True)
                mass += torch.exp(s / math.sqrt(D) - lse).sum((0, 1))
        drop[kc] = t0 + int(mass.argmax())
    dropped = attn_ref(q, k, xyz, lens, kv, drop=drop)
    wrong = None
    if any(kv[c] != c and lens[c] and lens[kv[c]] for c in range(len(kv))):
        wrong = attn_ref(q, k, xyz, lens, kv, keys_of=list(range(len(kv))))
    return dropped, wrong


# ------------------------------------------------------------------------------------------------ coordinate attention: GPU
def _ops():
    from regtr_amd import ops
    return ops


@pytest.mark.gpu
@pytest.mark.parametrize('name,head_dim,lens,kv,layers,kind,route', ATTN_CASES, ids=ATTN_IDS)
def test_attn_xyz_vs_fp64(name, head_dim, lens, kv, layers, kind, route):
    ops = _ops()
    q, k, xyz = attn_case(name, head_dim, lens, kv, layers, kind)
    seg = torch.tensor(_seg(lens), dtype=torch.int32).cuda()
    kvt = torch.tensor(kv, dtype=torch.int32).cuda()
    out = ops.attn_xyz(q.cuda(), k.cuda(), xyz.cuda(), seg, kvt, max(lens)).cpu()
    ref = attn_ref(q, k, xyz, lens, kv)
    r = attn_ratio(out, ref, attn_bound(q, k, xyz, lens, kv, ref), lens, kv)
    print(f'attn_xyz {name} D {head_dim} lens {lens[:6]} L {layers}: worst err/bound {r:.3f}')
    assert r <= 1, r


@pytest.mark.gpu
@pytest.mark.parametrize('head_dim', [32, 64, 128, 256])
def test_attn_xyz_cabi_writes_every_row(head_dim):
    """Through the C ABI with a NaN-filled output: every row of every query cloud is written (zeros for the empty partner)."""
    from regtr_amd import _lib
    lens, kv, layers = [65, 33, 0, 1, 1000, 31], [3, 4, 5, 0, 1, 2], 2
    q, k, xyz = attn_case('cabi', head_dim, lens, kv, layers, 'plain')
    qd, kd, xd = q.cuda(), k.cuda(), xyz.cuda()
    seg = torch.tensor(_seg(lens), dtype=torch.int32).cuda()
    kvt = torch.tensor(kv, dtype=torch.int32).cuda()
    out = torch.full((layers, sum(lens), 3), float('nan')).cuda()
    rc = _lib.lib().regtr_attn_xyz(qd.data_ptr(), kd.data_ptr(), xd.data_ptr(), out.data_ptr(), seg.data_ptr(), kvt.data_ptr(), len(lens),
                                   sum(lens), layers, max(lens), head_dim, 1.0 / math.sqrt(head_dim), _lib.stream())
    assert rc == 0
    out = out.cpu()
    assert torch.isfinite(out).all(), 'rows left unwritten'
    ref = attn_ref(q, k, xyz, lens, kv)
    r = attn_ratio(out, ref, attn_bound(q, k, xyz, lens, kv, ref), lens, kv)
    print(f'attn_xyz C ABI D {head_dim}: worst err/bound {r:.3f}')
    assert r <= 1, r


@pytest.mark.gpu
def test_attn_xyz_refusals():
    """Head dims other than 32 / 64 / 128 / 256 and a q view off 16-byte alignment are refused (RG_ERR_ARG); max_len == 0 launches
    nothing.  The output is left untouched in every case."""
    from regtr_amd import _lib
    L = _lib.lib()
    lens, kv = [40, 37], [1, 0]
    seg = torch.tensor(_seg(lens), dtype=torch.int32).cuda()
    kvt = torch.tensor(kv, dtype=torch.int32).cuda()
    N = sum(lens)
    xyz = torch.randn(N, 3).cuda()

    def call(q, k, out, max_len, D):
        rc = L.regtr_attn_xyz(q.data_ptr(), k.data_ptr(), xyz.data_ptr(), out.data_ptr(), seg.data_ptr(), kvt.data_ptr(), len(lens), N, 1,
                              max_len, D, 1.0 / math.sqrt(D), _lib.stream())
        torch.cuda.synchronize()
        return rc

    for D in (16, 48):
        q, k = torch.randn(1, N, D).cuda(), torch.randn(1, N, D).cuda()
        out = torch.full((1, N, 3), 7.0).cuda()
        assert call(q, k, out, max(lens), D) == RG_ERR_ARG, D
        assert (out == 7.0).all()
    D = 64
    buf = torch.randn(N * D + 4).cuda()
    k = torch.randn(1, N, D).cuda()
    out = torch.full((1, N, 3), 7.0).cuda()
    assert buf.data_ptr() % 16 == 0
    assert call(buf[1:1 + N * D].view(1, N, D), k, out, max(lens), D) == RG_ERR_ARG
    assert (out == 7.0).all()
    assert call(buf[:N * D].view(1, N, D), k, out, 0, D) == 0
    assert (out == 7.0).all()
    assert call(buf[:N * D].view(1, N, D), k, out, max(lens), D) == 0
    assert torch.isfinite(out).all() and not (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ weighted Procrustes: references
def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def pair_views(kp, corr, logit, lens, B):
    """Per (pair): a, b (L, n, 3) and logit (L, n) in the kernel's concatenation a = [src_kp ; tgt_corr], b = [src_corr ; tgt_kp]."""
    seg = _seg(lens)
    L = corr.shape[0]
    out = []
    for b in range(B):
        s, t = slice(seg[b], seg[b + 1]), slice(seg[B + b], seg[B + b + 1])
        a = torch.cat([kp[s].expand(L, -1, -1), corr[:, t]], 1)
        bb = torch.cat([corr[:, s], kp[t].expand(L, -1, -1)], 1)
        lg = torch.cat([logit[:, s], logit[:, t]], 1)
        out.append((a, bb, lg))
    return out


def kabsch64(a, b, w):
    """float64 weighted Kabsch (oracle.regtr_ref.compute_rigid_transform) and, per problem, kappa = s1 / (s2 + s3) of the covariance and
    scale = extent of the centred points + offset of the centroids from the origin."""
    from oracle import regtr_ref
    a, b, w = a.double(), b.double(), w.double()
    T = regtr_ref.compute_rigid_transform(a, b, w)
    wn = w[..., None] / torch.clamp_min(w.sum(-1, keepdim=True)[..., None], 1e-6)
    ca, cb = (a * wn).sum(-2), (b * wn).sum(-2)
    cov = (a - ca[..., None, :]).transpose(-2, -1) @ ((b - cb[..., None, :]) * wn)
    s = torch.linalg.svdvals(cov)
    kappa = s[..., 0] / (s[..., 1] + s[..., 2])
    ext = (a - ca[..., None, :]).norm(dim=-1).amax(-1) if a.shape[-2] else torch.zeros(a.shape[:-2], dtype=torch.float64)
    scale = ext + torch.maximum(ca.norm(dim=-1), cb.norm(dim=-1))
    return T, kappa, scale


def objective(T, a, b, w):
    """sum_i w_i |R a_i + t - b_i|^2 in float64."""
    T, a, b, w = T.double(), a.double(), b.double(), w.double()
    r = a @ T[..., :3].transpose(-1, -2) + T[..., None, :, 3] - b
    return (w * (r * r).sum(-1)).sum(-1)


def pose_ratio(pose, T, kappa, scale):
    """max |pose - T| / bound with bound C_POSE u kappa for R and C_POSE u kappa scale for t (kappa >= 1/2 always)."""
    eR = (pose[..., :3].double() - T[..., :3]).abs().amax((-1, -2))
    et = (pose[..., 3].double() - T[..., 3]).abs().amax(-1)
    bR = C_POSE * U32 * kappa
    bt = C_POSE * U32 * kappa * torch.clamp_min(scale, 1.0)
    return torch.maximum(eR / bR, et / bt).max().item()


def objective_ratio(pose, T, a, b, w, kappa, scale):
    """Rank-deficient covariances (R not unique): sqrt of the weighted objective at the kernel's pose against the float64 optimum, per
    unit weight, within C_POSE u scale min(sqrt(kappa), u^-1/2).  A rotation error theta ~ u kappa about the ill-determined axis moves the
    points by theta times their extent off that axis, ~ extent / sqrt(kappa): min(u sqrt(kappa), 1 / sqrt(kappa)) <= sqrt(u)."""
    sw = torch.clamp_min(w.double().sum(-1), 1e-300)
    rk = torch.sqrt(objective(pose, a, b, w) / sw)
    r0 = torch.sqrt(objective(T, a, b, w) / sw)
    k = torch.nan_to_num(kappa, nan=math.inf, posinf=math.inf)
    bound = C_POSE * U32 * torch.clamp_min(scale, 1.0) * torch.clamp(torch.sqrt(k), max=U32 ** -0.5)
    return ((rk - r0) / bound).max().item()


def assert_rotation(pose):
    R = pose[..., :3].double()
    assert (R @ R.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6
    assert (torch.det(R) - 1).abs().max() < 1e-6


# ------------------------------------------------------------------------------------------------ weighted Procrustes: cases
def _motion(a, R, t, noise=0.0, g=None):
    b = a.double() @ torch.from_numpy(R).T + torch.tensor(t, dtype=torch.float64)
    if noise:
        b = b + torch.randn(b.shape, generator=g, dtype=torch.float64) * noise
    return b.float()


def _cube():
    return torch.tensor([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=torch.float32)


def _tetra():
    return torch.tensor([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=torch.float32)


def _sphere(n, g):
    """n points whose second moment is isotropic: antipodal pairs of an orthonormal frame's +-axes, rotated copies."""
    pts = []
    for _ in range(n // 6):
        Q = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
        pts += [Q[:, i] * s for i in range(3) for s in (1, -1)]
    return torch.stack(pts).float()


def _near_line(n, rho, g):
    """Points along a line with an off-axis spread sigma2 / sigma1 ~ rho (second moments)."""
    s = torch.linspace(-2, 2, n, dtype=torch.float64)
    d = torch.tensor([0.6, -0.48, 0.64], dtype=torch.float64)
    d = d / d.norm()
    e = torch.linalg.qr(torch.stack([d, torch.randn(3, generator=g, dtype=torch.float64), torch.randn(3, generator=g, dtype=torch.float64)], 1))[0]
    off = torch.randn(n, 2, generator=g, dtype=torch.float64) * math.sqrt(rho) * s.std()
    return (s[:, None] * d + off[:, :1] * e[:, 1] + off[:, 1:] * e[:, 2] + torch.tensor([0.3, 1.1, -0.2], dtype=torch.float64)).float()


ANGLES = [0.0, 1e-4, math.pi / 2, math.radians(179.9), math.pi]


def motion_cases():
    """(name, a (n, 3), b (n, 3), logit (n,), the motion's R for noise-free cases) single problems, all through one launch."""
    g = torch.Generator().manual_seed(11)
    cases = []
    pts = (torch.rand(300, 3, generator=g) - 0.5) * torch.tensor([4.0, 2.0, 1.0])
    for ang in ANGLES:
        R = rot([0.3, -0.5, 0.8], ang)
        cases.append((f'exact{ang:.4g}', pts, _motion(pts, R, [0.5, -2.0, 1.0]), torch.randn(300, generator=g) * 2, R))
    kitti = (torch.rand(2000, 3, generator=g) - 0.5) + torch.tensor([100.0, 0.0, 0.0])
    R = rot([0.1, 0.1, 1.0], 0.3)
    cases.append(('kitti100m', kitti, _motion(kitti, R, [1.0, 0.2, 0.0], 0.01, g), torch.randn(2000, generator=g), None))
    R = rot([1.0, 2.0, 3.0], 1.0)
    for nm, p in (('cube', _cube()), ('tetra', _tetra()), ('sphere', _sphere(120, g))):
        cases.append((nm, p, _motion(p, R, [0.0, 1.0, 2.0]), torch.zeros(len(p)), R))
    return cases


def degenerate_cases():
    """Rank-deficient covariances: the objective is compared, not R."""
    g = torch.Generator().manual_seed(12)
    R = rot([0.2, 0.9, -0.4], 2.0)
    out = []
    line = torch.linspace(-1, 1, 50)[:, None] * torch.tensor([[0.3, 0.5, -0.8]]) + torch.tensor([1.0, 2.0, 3.0])
    out.append(('collinear', line, _motion(line, R, [1, 1, 1]), torch.randn(50, generator=g)))
    plane = torch.cat([(torch.rand(80, 2, generator=g) - 0.5) * 3, torch.zeros(80, 1)], 1)
    out.append(('coplanar', plane, _motion(plane, R, [0, 0, 1], 0.05, g), torch.randn(80, generator=g)))
    # the same plane seen mirrored: the unconstrained optimum is a reflection, the det flip must fire
    mir = plane.clone()
    mir[:, 0] *= -1
    out.append(('coplanar_flip', plane, _motion(mir, R, [0, 0, 1]), torch.zeros(80)))
    for rho in (1e-6, 1e-9, 1e-13):
        p = _near_line(64, rho, g)
        out.append((f'near_line{rho:g}', p, _motion(p, R, [0.5, 0, -1]), torch.zeros(64)))
    return out


def _launch_singles(cases, L=1):
    """Every case a pure-source pair of one launch (targets empty): returns pose (L, B, 3, 4) and the float32 inputs."""
    kp = torch.cat([c[1] for c in cases])
    corr = torch.cat([c[2] for c in cases])[None].expand(L, -1, -1).contiguous()
    logit = torch.cat([c[3] for c in cases])[None].expand(L, -1).contiguous()
    lens = [len(c[1]) for c in cases] + [0] * len(cases)
    return kp, corr, logit, lens


def _run(kp, corr, logit, lens, B, status=None):
    from regtr_amd import context
    ops = _ops()
    seg = torch.tensor(_seg(lens), dtype=torch.int32).cuda()
    with context.current().derive(status=status):
        pose = ops.weighted_procrustes(kp.cuda(), corr.cuda(), logit.cuda(), seg, B)
    return pose.cpu()


def _status():
    return torch.zeros(1, dtype=torch.int32).cuda()


# ------------------------------------------------------------------------------------------------ weighted Procrustes: GPU
@pytest.mark.gpu
def test_procrustes_exact_motions_and_repeated_singular_values():
    """Noise-free b = R a + t (angles 0 .. 180 degrees), a KITTI-like cloud 100 m out, cube / tetrahedron / isotropic sphere (s1 = s2 = s3)."""
    cases = motion_cases()
    kp, corr, logit, lens = _launch_singles(cases)
    st = _status()
    pose = _run(kp, corr, logit, lens, len(cases), st)
    assert int(st.item()) == 0
    worst = 0.0
    for i, (nm, a, b, lg, Rt) in enumerate(cases):
        T, kappa, scale = kabsch64(a, b, torch.sigmoid(lg.double()))
        r = pose_ratio(pose[0, i], T, kappa, scale)
        print(f'procrustes {nm}: kappa {kappa.item():.3g}, err/bound {r:.3f}')
        worst = max(worst, r)
        assert_rotation(pose[0, i])
        if Rt is not None:                     # noise-free: the motion itself is recovered (b was rounded to float32)
            assert (pose[0, i, :, :3].double() - torch.from_numpy(Rt)).abs().max() < 1e-5, nm
    print(f'procrustes exact motions: worst err/bound {worst:.3f}')
    assert worst <= 1


@pytest.mark.gpu
def test_procrustes_rank_deficient_by_objective():
    cases = degenerate_cases()
    kp, corr, logit, lens = _launch_singles(cases)
    st = _status()
    pose = _run(kp, corr, logit, lens, len(cases), st)
    assert int(st.item()) == 0
    worst = 0.0
    for i, (nm, a, b, lg) in enumerate(cases):
        w = torch.sigmoid(lg.double())
        T, kappa, scale = kabsch64(a, b, w)
        assert_rotation(pose[0, i])
        r = objective_ratio(pose[0, i], T, a, b, w, kappa, scale)
        print(f'procrustes {nm}: kappa {kappa.item():.3g}, objective excess/bound {r:.3f}')
        worst = max(worst, r)
    assert worst <= 1


@pytest.mark.gpu
def test_procrustes_zero_covariance_gives_identity():
    """One point, all weights exactly 0 (logit -inf) or underflowing float32's sigmoid (logit -100), coincident points: the covariance is
    exactly zero, and R = I, t = c_b - c_a as the float64 reference (torch.linalg.svd of a zero matrix: U = V = I)."""
    g = torch.Generator().manual_seed(13)
    pts = (torch.rand(40, 3, generator=g) - 0.5) * 3
    far = _motion(pts, rot([1, 0, 0], 0.7), [3, 2, 1])
    same = torch.tensor([[1.25, -0.5, 3.0]]).expand(8, 3).contiguous()
    cases = [('one_point', pts[:1], far[:1], torch.tensor([0.7])),
             ('minus_inf', pts, far, torch.full((40,), -math.inf)),
             ('minus_100', pts, far, torch.full((40,), -100.0)),
             ('coincident', same, same + torch.tensor([0.5, 1.0, -2.0]), torch.zeros(8)),
             ('coincident256', same[:1].expand(256, 3).contiguous(), same[:1].expand(256, 3) * 2, torch.full((256,), 1.5))]
    kp, corr, logit, lens = _launch_singles(cases, L=2)
    st = _status()
    pose = _run(kp, corr, logit, lens, len(cases), st)
    assert int(st.item()) == 0
    for i, (nm, a, b, lg) in enumerate(cases):
        T, _, scale = kabsch64(a, b, torch.sigmoid(lg.double()))
        assert torch.equal(pose[:, i, :, :3], torch.eye(3).expand(2, 3, 3)), (nm, pose[0, i])
        err = (pose[:, i, :, 3].double() - T[:, 3]).abs().max().item()
        print(f'procrustes zero covariance {nm}: R = I, |t - t_ref| {err:.2e}')
        assert err <= C_POSE * U32 * max(scale.item(), 1.0), nm
        # the float64 reference meets an exactly zero covariance too, except where float32 is what makes it zero: sigmoid(-100) = 4e-44
        # in float64, and 256 copies of float64's sigmoid(1.5) do not sum to exactly 256 times it (the reference's centroid is off by an ulp)
        if nm not in ('minus_100', 'coincident256'):
            assert torch.equal(T[:, :3], torch.eye(3, dtype=torch.float64)), nm


def _weight_cases():
    g = torch.Generator().manual_seed(14)
    n = 200
    a = (torch.rand(n, 3, generator=g) - 0.5) * 2
    b = _motion(a, rot([0.4, 0.1, -0.3], 0.9), [0.1, 0.2, 0.3], 0.02, g)
    sat = torch.tensor([20.0, -20.0, 90.0, -90.0, math.inf, -math.inf])[torch.randint(0, 6, (n,), generator=g)]
    one = torch.full((n,), -100.0)
    one[17] = 10.0
    low = torch.full((100,), -18.5)                       # sum w = 100 sigmoid(-18.5) = 9.2e-7 < 1e-6: the clamp is active
    return [('saturated', a, b, sat, 'pose'), ('one_hot', a, b, one, 'objective'),
            ('clamped', a[:100], b[:100], low, 'pose'), ('mixed', a, b, torch.randn(n, generator=g) * 4, 'pose')]


@pytest.mark.gpu
def test_procrustes_weights():
    """Logits +-20, +-90, +-inf; one point at +10 with the rest at -100 (a zero covariance in float32; the objective is compared);
    sum w below 1e-6 so that the clamp is active."""
    cases = _weight_cases()
    kp, corr, logit, lens = _launch_singles([c[:4] for c in cases])
    st = _status()
    pose = _run(kp, corr, logit, lens, len(cases), st)
    assert int(st.item()) == 0
    for i, (nm, a, b, lg, how) in enumerate(cases):
        w = torch.sigmoid(lg.double())
        T, kappa, scale = kabsch64(a, b, w)
        assert_rotation(pose[0, i])
        r = pose_ratio(pose[0, i], T, kappa, scale) if how == 'pose' else objective_ratio(pose[0, i], T, a, b, w, kappa, scale)
        print(f'procrustes weights {nm}: kappa {kappa.item():.3g}, {how} err/bound {r:.3f}')
        assert r <= 1, nm


@pytest.mark.gpu
@pytest.mark.parametrize('L', [1, 6])
def test_procrustes_model_layout_shapes(L):
    """seg_off of 2B + 1 entries, sources first: pair sizes 1, 2, 3, 255, 256, 257, 4097 split between both sides, one side empty, and
    B = 64 pairs of mixed sizes; every (layer, pair) against float64."""
    g = torch.Generator().manual_seed(15 + L)
    sizes = [(1, 0), (0, 2), (2, 1), (128, 127), (256, 0), (0, 256), (200, 57), (2048, 2049)]
    sizes += [(int(x), int(y)) for x, y in torch.randint(0, 40, (56, 2), generator=g)]
    sizes = [(s, t) if s + t else (1, 0) for s, t in sizes]
    B = len(sizes)
    lens = [s for s, _ in sizes] + [t for _, t in sizes]
    N = sum(lens)
    kp = (torch.rand(N, 3, generator=g) - 0.5) * 4
    corr = kp.unsqueeze(0) @ torch.from_numpy(rot([1, 1, 0], 0.4)).float().T + torch.randn(L, N, 3, generator=g) * 0.1
    logit = torch.randn(L, N, generator=g) * 2
    st = _status()
    pose = _run(kp, corr, logit, lens, B, st)
    assert int(st.item()) == 0
    worst, worst_obj = 0.0, 0.0
    for b, (a, bb, lg) in enumerate(pair_views(kp, corr, logit, lens, B)):
        w = torch.sigmoid(lg.double())
        T, kappa, scale = kabsch64(a, bb, w)
        assert_rotation(pose[:, b])
        n = a.shape[1]
        if n >= 4:
            worst = max(worst, pose_ratio(pose[:, b], T, kappa, scale))
        else:                                  # 1 - 3 points: rank <= 2, R not unique
            worst_obj = max(worst_obj, objective_ratio(pose[:, b], T, a, bb, w, kappa, scale))
    print(f'procrustes model layout L {L} B {B}: worst err/bound {worst:.3f}, small pairs objective {worst_obj:.3f}')
    assert worst <= 1 and worst_obj <= 1


@pytest.mark.gpu
def test_procrustes_drop_in_shapes_and_weights():
    """se3.compute_rigid_transform: shapes (N, 3) and (2, 3, N, 3), weights with exact 0 and 1 entries (the logit +-inf round trip) and
    weights=None (uniform)."""
    from regtr_amd.se3 import compute_rigid_transform
    g = torch.Generator().manual_seed(16)
    R = torch.from_numpy(rot([0.5, -1, 0.2], 2.5)).float()
    for shape in ((257,), (2, 3, 255)):
        a = (torch.rand(*shape, 3, generator=g) - 0.5) * 3
        b = a @ R.T + torch.tensor([1.0, -1.0, 0.5]) + torch.randn(*shape, 3, generator=g) * 0.05
        w = torch.rand(*shape, generator=g)
        w[..., ::7] = 0.0
        w[..., 3::5] = 1.0
        for weights in (w, None):
            T = compute_rigid_transform(a.cuda(), b.cuda(), None if weights is None else weights.cuda()).cpu()
            assert T.shape == (*shape[:-1], 3, 4)
            wd = torch.ones(shape, dtype=torch.float64) if weights is None else weights.double()
            Tr, kappa, scale = kabsch64(a, b, wd)
            r = pose_ratio(T, Tr, kappa, scale)
            print(f'drop-in {shape} weights {"given" if weights is not None else "None"}: err/bound {r:.3f}')
            assert r <= 1
            assert_rotation(T)


@pytest.mark.gpu
@pytest.mark.parametrize('where,value', [('corr', math.nan), ('corr', math.inf), ('corr', -math.inf), ('logit', math.nan), ('logit', math.inf)])
def test_procrustes_nonfinite_status(where, value):
    """B = 3: one non-finite corr entry or a NaN logit in pair 1 sets REGTR_STATUS_NONFINITE_POSE and leaves pairs 0 and 2 bit-identical
    to a clean run; the clean run leaves the status word at 0, and two identical launches give identical bits.  A logit of +inf is no
    fault: sigmoid(+inf) = 1 is a valid weight (as in the reference), so that pose stays finite, matches float64, and raises no bit."""
    g = torch.Generator().manual_seed(17)
    lens, B, L = [300, 257, 41, 99, 256, 1], 3, 2
    N = sum(lens)
    kp = (torch.rand(N, 3, generator=g) - 0.5) * 4
    corr = kp.unsqueeze(0) + torch.randn(L, N, 3, generator=g) * 0.2
    logit = torch.randn(L, N, generator=g) * 2
    st = _status()
    clean = _run(kp, corr, logit, lens, B, st)
    assert int(st.item()) == 0 and torch.isfinite(clean).all()
    assert torch.equal(clean, _run(kp, corr, logit, lens, B, st)), 'two identical launches differ'
    seg = _seg(lens)
    row = seg[B + 1] + 17                  # a target row of pair 1
    if where == 'corr':
        corr = corr.clone()
        corr[1, row, 1] = value
    else:
        logit = logit.clone()
        logit[1, row] = value
    pose = _run(kp, corr, logit, lens, B, st)
    assert torch.equal(pose[0], clean[0])
    assert torch.equal(pose[1, 0], clean[1, 0]) and torch.equal(pose[1, 2], clean[1, 2])
    if where == 'logit' and value == math.inf:
        assert int(st.item()) == 0
        a, bb, lg = pair_views(kp, corr, logit, lens, B)[1]
        T, kappa, scale = kabsch64(a[1], bb[1], torch.sigmoid(lg[1].double()))
        assert pose_ratio(pose[1, 1], T, kappa, scale) <= 1
    else:
        assert int(st.item()) == STATUS_NONFINITE_POSE
        assert not torch.isfinite(pose[1, 1]).all()


# ------------------------------------------------------------------------------------------------ RegTR.forward's non-finite pose branch
@pytest.mark.gpu
def test_forward_nonfinite_pose_branch(caplog):
    """A NaN in the overlap head's bias (the weights, never the input clouds: a NaN coordinate would reach the voxel-grid hashing) makes
    the pose non-finite with every f16 pair product finite: the forward counts it, re-runs once in fp32x3, logs, returns the NaN pose."""
    from regtr_amd import RegTR
    from tests.util import gold, load_cfg, seeded_sd
    g = gold('modelnet_demo')
    cfg = load_cfg('modelnet')
    sd = dict(seeded_sd(cfg))
    m = RegTR(cfg)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    assert m._f16_pair and m._range_check, 'the status word is read only by the f16 pair forward with its range check'
    batch = lambda: {'src_xyz': [torch.from_numpy(g['src']).cuda()], 'tgt_xyz': [torch.from_numpy(g['tgt']).cuda()]}
    out = m(batch())
    assert torch.isfinite(out['pose']).all() and m.nonfinite_pose_forwards == 0
    fallbacks = m.f16_range_fallbacks
    sd['correspondence_decoder.conf_logits_decoder.bias'] = torch.full_like(sd['correspondence_decoder.conf_logits_decoder.bias'], math.nan)
    m.load_state_dict(sd, strict=True)
    with caplog.at_level(logging.WARNING, logger=m.logger.name):
        out = m(batch())
    assert not torch.isfinite(out['pose']).all()
    assert m.nonfinite_pose_forwards == 1
    assert m.f16_range_fallbacks == fallbacks
    assert any('non-finite pose' in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records]
