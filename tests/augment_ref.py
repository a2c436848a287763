"""Numpy float64 restatement of the training augmentation (regtr_amd/augment.py, csrc/augment.hip): the reference's chain RigidPerturb ->
Jitter -> ShufflePoints -> RandomSwap (data_loaders/transforms.py) and the random numbers that drive it on the device, for
tests/test_augment_host.py and tests/test_gpu_augment.py.

RANDOM NUMBERS -- the one convention of csrc/augment.hip:
    Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (index, cloud_or_pair, purpose, step)
    purpose 0: pair draws, 1: shuffle keys, 2: jitter;   uniform u = ((x >> 8) + 0.5) 2^-24   (never 0 or 1)
    normals: Box-Muller, z0 = sqrt(-2 ln u(xa)) cos(2 pi u(xb)), z1 = ... sin(...), words (x0, x1) -> (z0, z1), (x2, x3) -> (z2, z3)
    pair b:  block 0 (index 0): x0 x1 x2 the perturbation's uniforms;  block 1: z0 the angle, z1 z2 z3 the translation (small);
             block 2: x0 -> perturb_source = u > 0.5, x1 -> swap = u > 0.5
    shuffle key of input row r of input cloud slot c: (c << 32) | x0 of counter (r, c, 1, step); the permutation is the stable ascending
             sort, cloud c's output rows the first min(n_c, max_pts) of its sorted segment
    jitter of OUTPUT row i of OUTPUT cloud slot c': z0 z1 z2 of counter (i, c', 2, step)
Cloud slots: the src clouds of the B pairs, then the tgt clouds.

`draws` produces every decision of a batch; `apply` runs the chain on one pair from a set of decisions -- those of `draws`, or the ones
recorded from the reference's own generators (tests/golden/augment_ref_chain.npz, tools/make_golden_augment.py).  The chain is restated
once; the only difference between the two uses is where the jitter is added: the reference jitters every input row and then selects
(noise_on_output False), the device jitters the rows it keeps, keyed by where they land (True).

THE FLOAT32 BOUND (`bounds`).  `apply` takes the float32 inputs and the float32-rounded perturbation P (the reference's `.float()`) as
given and does everything else in float64, so |float32 chain - apply| is the float32 chain's own rounding.  With U = 2^-24, first order
in U, per component, in whatever order a float32 implementation adds: a 3-term dot product with a unit row of a rotation plus a
translation, fl(r . v + t), is within 4 U (|v| + |t|) of exact (three products, three additions; sum |r_k v_k| <= |v|).  For one pair,
with X = max |x| over the perturbed cloud's points, n its size, c its centroid, t the perturbation's own translation, g the translation
of the input pose:
    centroid       a float32 mean of n points, any order:                          e_c  = (n + 2) U X
    t' = R(-c) + (t + c)   the recentred translation (transforms.py:48-54); with rho = |I - R|_2 = 2 sin(angle(R) / 2) its size is
                   |t'| <= T' = |t| + rho |c|; the centroid's error enters as (I - R) dc, |.| <= rho sqrt(3) e_c; the dot product and
                   the two sums: 5 U (2 |c| + |t|)                                 e_t  = rho sqrt(3) e_c + 5 U (2 |c| + |t|)
    points         x' = R x + t', then + noise (one product, one sum):             e_x  = 4 U (X + T') + e_t + U (X + T' + 2 max|noise|)
    P'^-1          translation -R^T t':                                            e_ti = 3 U T' + sqrt(3) e_t
    pose           rotation G R^T or R G, entries:                                 e_R  = 3 U
                   translation G ti + g or R g + t' (the former is the larger):    e_g  = 4 U (T' + |g|) + sqrt(3) e_ti
    swap           pose^-1: the rotation transposed (no rounding), translation -R''^T t'' with |t''| <= T' + |g|:
                                                                                   e_gs = 3 U (T' + |g|) + sqrt(3) e_g + 3 e_R (T' + |g|)
The cloud that is not perturbed goes through the identity (device) or is not touched (reference): its bound is the jitter's sum alone,
U (X + 2 max|noise|).  On the device (`device=True`) the centroid is a float64 sum rounded once, like the restatement's: the two can differ
by the last float32 place only, e_c = 2 U X whatever n.  There P is formed by float64 library calls that may differ from numpy's in the last place, so its
float32 rounding may differ by one ulp: entries of R by U, of t by U |t|, which moves a point by at most
sqrt(3) U |x - c| + U |t| <= 2 sqrt(3) U X + U |t| and the pose terms by the same order; and the float32 Box-Muller adds
augment_noise * BOX_MULLER_ERR.
    BOX_MULLER_ERR: z = r cos(a), r = sqrt(-2 ln u1) <= R_MAX = sqrt(50 ln 2) < 5.9 (u1 >= 2^-25), a = 2 pi u2 < 6.3.  ln u1 is accurate
    to a few ulp by construction (logf below 1/2, log1pf(-(1 - u1)) above, both arguments exact), so r carries ~4 U relative; the angle
    carries u2's rounding to float32 (U / 2 relative), the constant's and the product's (2 U relative together): |da| <= 3 U 6.3 < 19 U;
    sincosf ~2 ulp: 4 U; the final product U.  |dz| <= R_MAX (19 U + 4 U) + (4 U + U) R_MAX < 28 U R_MAX.
"""
import numpy as np

U = 2.0 ** -24
SQ3 = np.sqrt(3.0)
R_MAX = np.sqrt(50.0 * np.log(2.0))
BOX_MULLER_ERR = 28.0 * U * R_MAX
SECOND_ORDER = 1.001
PERTURB_STD = 0.1

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xffffffff)
_S32 = np.uint64(32)


def philox4x32(counter, key):
    """Philox4x32-10: counter (..., 4), key (2,) -> (..., 4) uint32."""
    c0, c1, c2, c3 = (np.asarray(counter, dtype=np.uint64)[..., i] & _LO for i in range(4))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xffffffff, (k1 + _W1) & 0xffffffff
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _key(seed):
    seed = int(seed) & ((1 << 64) - 1)
    return seed & 0xffffffff, seed >> 32


def words(seed, step, index, slot, purpose):
    """Philox words of counter (index, slot, purpose, step), index and slot arrays of one shape -> (..., 4)."""
    index, slot = np.broadcast_arrays(np.asarray(index, dtype=np.uint64), np.asarray(slot, dtype=np.uint64))
    ctr = np.stack([index, slot, np.full(index.shape, purpose, dtype=np.uint64), np.full(index.shape, int(step) & 0xffffffff, dtype=np.uint64)],
                   axis=-1)
    return philox4x32(ctr, _key(seed))


def uniform(x):
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(w):
    """Four normals of a block of four words: (..., 4) -> (..., 4)."""
    r0, r1 = np.sqrt(-2.0 * np.log(uniform(w[..., 0]))), np.sqrt(-2.0 * np.log(uniform(w[..., 2])))
    a0, a1 = 2.0 * np.pi * uniform(w[..., 1]), 2.0 * np.pi * uniform(w[..., 3])
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def _hat(w):
    z = np.zeros(w.shape[:-1])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1), np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def euler_zyx(a, b, c):
    """scipy's Rotation.from_euler('zyx', [a, b, c]).as_matrix() (extrinsic: about z by a, then y by b, then x by c) = Rx(c) Ry(b) Rz(a);
    the fixture's recorded angles and matrices pin it (tests/test_augment_host.py)."""
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return np.stack([np.stack([cb * ca, -cb * sa, sb], -1),
                     np.stack([sc * sb * ca + cc * sa, -sc * sb * sa + cc * ca, -sc * cb], -1),
                     np.stack([-cc * sb * ca + sc * sa, cc * sb * sa + sc * ca, cc * cb], -1)], -2)


def pair_draws(seed, step, B, perturb_pose='small', swap=True):
    """The pair decisions: {'P' (B, 3, 4) float64 (before recentring), 'perturb_source', 'swap' (B,) bool, 'axis' (B, 3), 'z' (B, 4)}."""
    pairs = np.arange(B)
    q, g, f = (words(seed, step, np.full(B, blk), pairs, 0) for blk in (0, 1, 2))
    P = np.tile(np.eye(4)[:3], (B, 1, 1))
    out = {'axis': None, 'z': None}
    if perturb_pose == 'small':                            # cvhelpers/lie/numpy/so3.py:31-38,82-101, se3.py:38-44, so3_common.py:185-210
        z = normals(g)
        phi, th = 2.0 * np.pi * uniform(q[:, 0]), np.arccos(2.0 * uniform(q[:, 1]) - 1.0)
        axis = np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)], -1)
        omega = axis * (z[:, :1] * (PERTURB_STD * np.pi / np.sqrt(3.0)))
        theta = np.linalg.norm(omega, axis=-1, keepdims=True)
        near = np.isclose(theta, 0.0)[..., None]
        with np.errstate(divide='ignore', invalid='ignore'):
            H = _hat(omega / theta)
        rod = np.eye(3) + np.sin(theta)[..., None] * H + (1.0 - np.cos(theta))[..., None] * (H @ H)
        P[:, :, :3] = np.where(near, np.eye(3) + _hat(omega), rod)
        P[:, :, 3] = z[:, 1:] * (PERTURB_STD / np.sqrt(3.0))
        out.update(axis=axis, z=z)
    elif perturb_pose == 'large':                          # transforms.py:28-32
        P[:, :, :3] = euler_zyx(*(2.0 * np.pi * uniform(q[:, i]) for i in range(3)))
    elif perturb_pose != 'none':
        raise ValueError(perturb_pose)
    out['P'] = P
    out['perturb_source'] = (uniform(f[:, 0]) > 0.5) if perturb_pose != 'none' else np.zeros(B, dtype=bool)
    out['swap'] = (uniform(f[:, 1]) > 0.5) if swap else np.zeros(B, dtype=bool)
    return out


def shuffle_keys(seed, step, sizes):
    """int64 keys of the packed input rows of clouds of `sizes` (by slot)."""
    slot = np.repeat(np.arange(len(sizes)), sizes)
    row = np.concatenate([np.arange(n) for n in sizes]) if len(sizes) else np.zeros(0, dtype=np.int64)
    w = words(seed, step, row, slot, 1)[:, 0]
    return (slot.astype(np.int64) << 32) | w.astype(np.int64)


def shuffle_perm(seed, step, sizes):
    """The stable ascending sort of the keys: (N,) global input rows."""
    return np.argsort(shuffle_keys(seed, step, sizes), kind='stable')


def jitter_normals(seed, step, out_sizes):
    """(N_out, 3) normals of the packed output rows of clouds of `out_sizes` (by OUTPUT slot)."""
    slot = np.repeat(np.arange(len(out_sizes)), out_sizes)
    row = np.concatenate([np.arange(n) for n in out_sizes])
    return normals(words(seed, step, row, slot, 2))[:, :3]


def draws(seed, step, sizes, perturb_pose='small', swap=True, max_pts=30000, shuffle=True):
    """Every decision of a batch.  sizes: (src sizes, tgt sizes).  -> the pair draws plus, per pair b, 'src_idx' / 'tgt_idx' (the kept
    rows of the INPUT src / tgt cloud, in output order) and 'noise_src' / 'noise_tgt' (normals of the rows of the OUTPUT src / tgt
    cloud), 'perm' (N_in,) and 'in_slot' (2B,)."""
    src_n, tgt_n = list(sizes[0]), list(sizes[1])
    B = len(src_n)
    lens = src_n + tgt_n
    d = pair_draws(seed, step, B, perturb_pose, swap)
    off = np.concatenate([[0], np.cumsum(lens)])
    perm = shuffle_perm(seed, step, lens) if shuffle else np.arange(off[-1])
    idx = [perm[off[c]:off[c] + min(lens[c], max_pts)] - off[c] for c in range(2 * B)]
    in_slot = [b + B if d['swap'][b] else b for b in range(B)] + [b if d['swap'][b] else b + B for b in range(B)]
    out_sizes = [len(idx[s]) for s in in_slot]
    z = jitter_normals(seed, step, out_sizes)
    ooff = np.concatenate([[0], np.cumsum(out_sizes)])
    d.update(perm=perm, in_slot=in_slot, src_idx=idx[:B], tgt_idx=idx[B:],
             noise_src=[z[ooff[b]:ooff[b + 1]] for b in range(B)], noise_tgt=[z[ooff[B + b]:ooff[B + b + 1]] for b in range(B)])
    return d


def pair_of(d, b):
    """The decisions of pair b of `draws`' result, in `apply`'s form."""
    return {k: d[k][b] for k in ('P', 'perturb_source', 'swap', 'src_idx', 'tgt_idx', 'noise_src', 'noise_tgt')}


# ---------------------------------------------------------------------------------------------------------------- the chain
def se3_cat(a, b):
    return np.concatenate([a[:, :3] @ b[:, :3], a[:, :3] @ b[:, 3:] + a[:, 3:]], axis=1)


def se3_inv(a):
    return np.concatenate([a[:, :3].T, -a[:, :3].T @ a[:, 3:]], axis=1)


def se3_apply(T, x):
    return x @ T[:, :3].T + T[:, 3]


def apply(pair, d, augment_noise=0.005, perturb_pose='small', noise_on_output=True):
    """pair: 'src_xyz', 'tgt_xyz' (n, 3) float32, 'pose' (3, 4) / (4, 4), 'src_overlap', 'tgt_overlap' (n,) bool.
    d: 'P' (3, 4) / (4, 4), 'perturb_source', 'swap', 'src_idx', 'tgt_idx', 'noise_src', 'noise_tgt' (normals, before the scale).
    -> the augmented pair in float64 ('src_xyz', 'tgt_xyz', 'pose' (3, 4), masks) plus 'xform_src' / 'xform_tgt', the transform each
    INPUT cloud went through."""
    x = {'src': np.asarray(pair['src_xyz'], dtype=np.float64), 'tgt': np.asarray(pair['tgt_xyz'], dtype=np.float64)}
    m = {'src': np.asarray(pair['src_overlap']), 'tgt': np.asarray(pair['tgt_overlap'])}
    pose = np.asarray(pair['pose'], dtype=np.float64)[:3]
    eye = np.eye(4)[:3]
    T = {'src': eye, 'tgt': eye}
    if perturb_pose != 'none':                                                           # transforms.py:39-72
        P = np.asarray(d['P'])[:3].astype(np.float32).astype(np.float64)                 # :36-37 `.float()`
        which = 'src' if d['perturb_source'] else 'tgt'
        if perturb_pose == 'small':                                                      # :48-54
            cen = x[which].mean(axis=0).astype(np.float32).astype(np.float64)            # a float32 tensor in the reference
            C = np.concatenate([np.eye(3), -cen[:, None]], axis=1)
            P = se3_cat(se3_cat(se3_inv(C), P), C)
        pose = se3_cat(pose, se3_inv(P)) if d['perturb_source'] else se3_cat(P, pose)    # :57, :65
        T[which] = P
    for k in ('src', 'tgt'):
        x[k] = se3_apply(T[k], x[k])
        if not noise_on_output and augment_noise:                                        # :89-91, every input row
            x[k] = x[k] + np.asarray(d[f'noise_{k}'], dtype=np.float64) * augment_noise
        x[k], m[k] = x[k][d[f'{k}_idx']], m[k][d[f'{k}_idx']]                            # :124-127
    a, b = ('tgt', 'src') if d['swap'] else ('src', 'tgt')                               # :138-148
    if d['swap']:
        pose = se3_inv(pose)
    out = {'src_xyz': x[a], 'tgt_xyz': x[b], 'src_overlap': m[a], 'tgt_overlap': m[b], 'pose': pose, 'xform_src': T['src'], 'xform_tgt': T['tgt']}
    if noise_on_output and augment_noise:
        out['src_xyz'] = out['src_xyz'] + np.asarray(d['noise_src'], dtype=np.float64) * augment_noise
        out['tgt_xyz'] = out['tgt_xyz'] + np.asarray(d['noise_tgt'], dtype=np.float64) * augment_noise
    return out


def bounds(pair, d, augment_noise=0.005, perturb_pose='small', device=False):
    """Per-component bounds on |float32 chain - apply| for one pair (the derivation above): {'perturbed', 'other': the points of the
    perturbed / the other INPUT cloud, 'pose_R', 'pose_t'}."""
    which = 'src' if d['perturb_source'] else 'tgt'
    other = 'tgt' if d['perturb_source'] else 'src'
    nz = max(float(np.abs(d['noise_src']).max(initial=0.0)), float(np.abs(d['noise_tgt']).max(initial=0.0))) * abs(augment_noise)
    bm = abs(augment_noise) * BOX_MULLER_ERR if device else 0.0
    Xo = float(np.linalg.norm(np.asarray(pair[f'{other}_xyz'], dtype=np.float64), axis=1).max())
    g = float(np.linalg.norm(np.asarray(pair['pose'], dtype=np.float64)[:3, 3]))
    e_other = U * (Xo + 2 * nz) + bm
    if perturb_pose == 'none':
        e_x, e_R, e_g, e_gs = e_other, 0.0, 0.0, 3 * U * g
    else:
        xs = np.asarray(pair[f'{which}_xyz'], dtype=np.float64)
        X, n = float(np.linalg.norm(xs, axis=1).max()), len(xs)
        c = float(np.linalg.norm(xs.mean(axis=0))) if perturb_pose == 'small' else 0.0
        t = float(np.linalg.norm(np.asarray(d['P'], dtype=np.float64)[:3, 3]))
        e_c = ((2 if device else n + 2) * U * X) if perturb_pose == 'small' else 0.0
        Rm = np.asarray(d['P'], dtype=np.float64)[:3, :3]
        rho = 2.0 * np.sin(0.5 * np.arccos(np.clip((np.trace(Rm) - 1.0) / 2.0, -1.0, 1.0)))
        Tp = t + rho * c
        e_t = rho * SQ3 * e_c + 5 * U * (2 * c + t)
        e_P = (2 * SQ3 * U * X + U * t) if device else 0.0
        e_x = 4 * U * (X + Tp) + e_t + U * (X + Tp + 2 * nz) + e_P + bm
        e_ti = 3 * U * Tp + SQ3 * (e_t + e_P)
        e_R = 3 * U + (U if device else 0.0)
        e_g = 4 * U * (Tp + g) + SQ3 * e_ti + (SQ3 * U * g if device else 0.0)
        e_gs = 3 * U * (Tp + g) + SQ3 * e_g + 3 * e_R * (Tp + g)
    sw = bool(d['swap'])
    return {'perturbed': e_x * SECOND_ORDER, 'other': e_other * SECOND_ORDER, 'pose_R': e_R * SECOND_ORDER,
            'pose_t': (e_gs if sw else e_g) * SECOND_ORDER, 'which': which}


def nearest_dist(q, s):
    """Float64 distance from every q to its nearest s: |q|^2 + |s|^2 - 2 q.s by blocks of queries (the cancellation costs ~1e-15 |x|^2 of
    the squared distance: nothing next to the 1e-5 margin it is used with)."""
    q, s = np.asarray(q, dtype=np.float64), np.asarray(s, dtype=np.float64)
    s2 = (s * s).sum(1)
    out = np.empty(len(q))
    for lo in range(0, len(q), 2048):
        b = q[lo:lo + 2048]
        out[lo:lo + 2048] = np.sqrt(np.maximum(((b * b).sum(1)[:, None] + s2[None, :] - 2.0 * (b @ s.T)).min(axis=1), 0.0))
    return out
