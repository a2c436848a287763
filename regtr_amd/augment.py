"""The reference's 3DMatch training augmentation on the device (csrc/augment.hip): resident raw pairs in, an augmented batch with ground
truth out, ready for RegTR.training_step.

    batch = train_batch(src_list, tgt_list, poses, cfg, seed, step)        # level-0 masks on the clean clouds, then augment_batch
    pred, losses = model.training_step(batch, train_backbone=True)

The chain is the one data_loaders/__init__.py:18-23 applies to every 3DMatch training pair (data_loaders/transforms.py):
    RigidPerturb(perturb_pose) -> Jitter(augment_noise) -> ShufflePoints(max_pts) -> RandomSwap
with its pose bookkeeping (pose o P^-1 / P o pose, inverted on a swap) and the `small` perturbation recentred about the centroid of the
cloud it moves.  Every random decision comes from a counter-based generator, so a batch is a pure function of (inputs, seed, step):

    Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (index, cloud_or_pair, purpose, step)
    purpose 0: pair draws, 1: shuffle keys, 2: jitter (keyed by the OUTPUT row); uniform = ((x >> 8) + 0.5) 2^-24

(csrc/augment.hip states which word feeds which decision; tests/augment_ref.py restates it in numpy.)  Jitter and shuffle commute here
because the jitter of a row is keyed by where the row lands, not by where it came from.

Five launches and one radix sort per batch: centroids, pair draws, shuffle keys, torch.sort(stable=True), one gather pass over the points.
Nothing synchronises: the output lengths min(n, max_pts) depend on the swap decision, which the host takes from the same Philox words
(`swap_flags`) instead of reading the device's flags back.

The ModelNet chain (data_loaders/modelnet.py:102-109) is `modelnet_train_batch` below (csrc/augment_modelnet.hip, purposes 3-7 of the same
Philox convention).  Not built here: the `correspondences` key (no loss reads it).  (The optimiser: regtr_amd/optim.py;
the loop: harness.train_loop, train.py.)
Refused: CPU tensors, empty clouds, clouds that are not (n, 3), masks that do not match their cloud.
"""
import numpy as np
import torch

from . import _lib, ops
from .overlap import compute_overlap_masks

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32(counter, key):
    """Philox4x32-10 on the host: counter (..., 4) and key (2,) of uint32 values -> (..., 4) uint32.  The same function as the kernels'."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] for i in range(4)]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    lo32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + _W0) & 0xffffffff, (k1 + _W1) & 0xffffffff
    return np.stack(c, axis=-1).astype(np.uint32)


def swap_flags(seed, step, n_pairs):
    """RandomSwap's decisions of a batch, (n_pairs,) bool, from the words regtr_augment_draws reads: word 1 of counter (2, pair, 0, step),
    u > 0.5."""
    ctr = np.zeros((n_pairs, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 3] = 2, np.arange(n_pairs), int(step) & 0xffffffff
    seed = int(seed) & ((1 << 64) - 1)
    x = philox4x32(ctr, (seed & 0xffffffff, seed >> 32))
    return (x[:, 1] >> np.uint32(8)) >= np.uint32(1 << 23)


def _check_clouds(batch):
    src, tgt = list(batch['src_xyz']), list(batch['tgt_xyz'])
    if not src or len(src) != len(tgt):
        raise RuntimeError(f'augment_batch: src_xyz and tgt_xyz must be lists of the same non-zero length, got {len(src)} and {len(tgt)}')
    for name, clouds in (('src_xyz', src), ('tgt_xyz', tgt)):
        for b, c in enumerate(clouds):
            if not isinstance(c, torch.Tensor) or c.device.type != 'cuda':
                raise RuntimeError(f'augment_batch: {name}[{b}] must be a GPU tensor (got {getattr(c, "device", type(c))}); there is no CPU fallback')
            if c.dim() != 2 or c.shape[1] != 3 or c.dtype is not torch.float32:
                raise RuntimeError(f'augment_batch: {name}[{b}] must be a float32 (n, 3) cloud, got {c.dtype} {tuple(c.shape)}')
            if c.shape[0] == 0:
                raise RuntimeError(f'augment_batch: {name}[{b}] is empty; an empty cloud has no centroid and no overlap')
    return src, tgt


def augment_batch(batch, seed, step, *, augment_noise=0.005, perturb_pose='small', max_pts=30000, shuffle=True, swap=True):
    """batch: 'src_xyz' / 'tgt_xyz' (lists (B) of device (n, 3) float32 clouds), 'pose' ((B, 3, 4) or (B, 4, 4)), 'src_overlap' /
    'tgt_overlap' (lists (B) of per-point bool masks).  -> the same keys for the augmented pairs: lists of views into packed outputs
    (lengths min(n, max_pts) of the cloud that lands in the slot), 'pose' (B, 3, 4), and '_augment' = {'flags' (B, 2) int32
    (perturb_source, swap), 'xform' (2B, 3, 4): the transform of every INPUT cloud slot (src slots, then tgt slots), 'perm' (N_in,) int64:
    the stable sort's input rows (None with shuffle=False), 'in_slot': per output slot the input slot that lands there (host list)}.
    perturb_pose 'none' copies the points untransformed (bit for bit with augment_noise = 0); otherwise the unperturbed cloud of a pair
    goes through the identity transform like the perturbed one through P.  No host wait."""
    if perturb_pose not in ops.PERTURB_MODES:
        raise RuntimeError(f"augment_batch: perturb_pose must be 'none', 'small' or 'large', got {perturb_pose!r}")
    if int(max_pts) < 1:
        raise RuntimeError(f'augment_batch: max_pts must be positive, got {max_pts}')
    src, tgt = _check_clouds(batch)
    B = len(src)
    dev = src[0].device
    clouds = src + tgt
    masks = list(batch['src_overlap']) + list(batch['tgt_overlap'])
    if len(masks) != 2 * B:
        raise RuntimeError(f'augment_batch: src_overlap and tgt_overlap must hold one mask per cloud, got {len(masks)} for {2 * B} clouds')
    for c, (m, x) in enumerate(zip(masks, clouds)):
        if not isinstance(m, torch.Tensor) or m.device.type != 'cuda':
            raise RuntimeError(f'augment_batch: overlap mask {c} must be a GPU tensor (got {getattr(m, "device", type(m))}); there is no CPU fallback')
        if m.dim() != 1 or m.shape[0] != x.shape[0]:
            raise RuntimeError(f'augment_batch: overlap mask {c} must have one entry per point, got {tuple(m.shape)} for {x.shape[0]} points')
    pose = batch['pose']
    if not isinstance(pose, torch.Tensor) or pose.device.type != 'cuda':
        raise RuntimeError(f'augment_batch: pose must be a GPU tensor (got {getattr(pose, "device", type(pose))}); there is no CPU fallback')
    if pose.shape[0] != B or tuple(pose.shape[1:]) not in ((3, 4), (4, 4)):
        raise RuntimeError(f'augment_batch: pose must be ({B}, 3, 4) or ({B}, 4, 4), got {tuple(pose.shape)}')

    # the layout, on the host: input slots [src_0 .. src_{B-1}, tgt_0 .. tgt_{B-1}]; a swapped pair's clouds land in each other's slots
    lens = [int(c.shape[0]) for c in clouds]
    swapped = swap_flags(seed, step, B) if swap else np.zeros(B, dtype=bool)
    in_slot = [(b + B if swapped[b] else b) for b in range(B)] + [(b if swapped[b] else b + B) for b in range(B)]
    out_lens = [min(lens[s], int(max_pts)) for s in in_slot]
    in_off = np.concatenate([[0], np.cumsum(lens)])
    out_off = np.concatenate([[0], np.cumsum(out_lens)])
    n_in, n_out = int(in_off[-1]), int(out_off[-1])
    if n_in >= 2 ** 31:
        raise RuntimeError(f'augment_batch: {n_in} points exceed the int32 row index')
    with _lib.on_device(dev):
        meta = torch.from_numpy(np.concatenate([in_off, out_off, in_slot]).astype(np.int32)).to(dev, non_blocking=True)
        d_in_off, d_out_off, d_in_slot = meta[:2 * B + 1], meta[2 * B + 1:4 * B + 2], meta[4 * B + 2:]
        xyz = torch.cat(clouds, dim=0)
        mask = torch.cat([m.to(torch.bool) for m in masks], dim=0).view(torch.uint8)
        pose = pose.to(torch.float32)
        centroids = ops.cloud_centroids(xyz, d_in_off) if perturb_pose == 'small' else None
        xform, pose_out, flags = ops.augment_draws(pose, centroids, seed, step, perturb_pose, 0.1, swap)
        perm = None
        if shuffle:
            perm = torch.sort(ops.shuffle_keys(d_in_off, n_in, seed, step), stable=True)[1]
        out, out_mask = ops.augment_gather(xyz, mask, d_in_off, perm, d_out_off, d_in_slot, n_out,
                                           None if perturb_pose == 'none' else xform, augment_noise, seed, step)
    out_mask = out_mask.view(torch.bool)
    xs, ms = list(torch.split(out, out_lens)), list(torch.split(out_mask, out_lens))
    return {'src_xyz': xs[:B], 'tgt_xyz': xs[B:], 'pose': pose_out, 'src_overlap': ms[:B], 'tgt_overlap': ms[B:],
            '_augment': {'flags': flags, 'xform': xform, 'perm': perm, 'in_slot': in_slot}}


def train_batch(src_list, tgt_list, poses, cfg, seed, step):
    """One training batch from resident raw pairs: the level-0 ground-truth masks of the CLEAN clouds at cfg.overlap_radius
    (overlap.compute_overlap_masks; the reference computes them before its augmentation too, threedmatch.py:78-84), then augment_batch
    with cfg's augment_noise / perturb_pose (3dmatch.yaml; the reference's values when absent).  The result goes straight into
    RegTR.training_step."""
    batch = {'src_xyz': list(src_list), 'tgt_xyz': list(tgt_list)}
    _check_clouds(batch)
    if not isinstance(poses, torch.Tensor) or poses.device.type != 'cuda':
        raise RuntimeError(f'train_batch: poses must be a GPU tensor (got {getattr(poses, "device", type(poses))}); there is no CPU fallback')
    batch['pose'] = poses
    batch['src_overlap'], batch['tgt_overlap'] = compute_overlap_masks(batch['src_xyz'], batch['tgt_xyz'], poses, cfg.overlap_radius)
    return augment_batch(batch, seed, step, augment_noise=cfg.get('augment_noise', 0.005), perturb_pose=cfg.get('perturb_pose', 'small'))


# ---------------------------------------------------------------------------------------------------------------- the ModelNet chain
MODELNET_RESAMPLE = 717      # modelnet_transforms.py:92-93: both sizes, whatever num_points says, with a two-element `partial`
_quantile_cache = {}


def crop_quantile(n, p_keep):
    """np.percentile's position for RandomCrop.crop (modelnet_transforms.py:198) in a cloud of n points: (lo, t) with the threshold
    lerp(sorted[lo], sorted[lo + 1], t).  The reference's p_keep is a float32 (:186), so q = (1 - float32(p)) 100 is a float32 (30.000002
    for 0.7), and where numpy rounds on the way to the virtual index (n - 1) q / 100 is numpy's business: the position is read off
    np.percentile itself: lo from the ramp 0..n-1 (the answer there is lo + t), t from the step that is 0 up to rank lo and 1 above it (the
    answer there is lerp(0, 1, t) = t, exactly, in both branches of numpy's lerp)."""
    key = (int(n), float(np.float32(p_keep)))
    if key not in _quantile_cache:
        q = (np.float32(1.0) - np.float32(p_keep)) * np.float32(100)
        ramp = np.arange(int(n), dtype=np.float64)
        lo = min(int(np.floor(np.percentile(ramp, q))), int(n) - 2)
        _quantile_cache[key] = (lo, float(np.percentile((ramp > lo).astype(np.float64), q)))
    return _quantile_cache[key]


def _check_modelnet_cfg(cfg):
    noise_type = cfg.get('noise_type', 'crop')
    if noise_type != 'crop':
        raise NotImplementedError(f"modelnet_train_batch: noise_type {noise_type!r} is not built (only 'crop', the value modelnet.yaml uses)")
    partial = cfg.get('partial', [0.7, 0.7])
    if not isinstance(partial, (list, tuple)) or len(partial) != 2:
        raise NotImplementedError(f'modelnet_train_batch: partial {partial!r} is not built (only a two-element list, as in modelnet.yaml)')
    p = float(partial[0])                                   # :216-217: both clouds use p_keep[0]
    if not 0.0 < p < 1.0 or np.float32(p) == np.float32(0.5):
        raise NotImplementedError(f'modelnet_train_batch: partial[0] = {partial[0]!r} is not built (a proportion in (0, 1) other than 0.5, '
                                  'which the reference crops at the plane through the centroid instead of at a percentile)')
    if int(cfg.get('num_points', 1024)) < 1:
        raise RuntimeError(f"modelnet_train_batch: num_points must be positive, got {cfg.get('num_points')}")
    return p, float(cfg.get('rot_mag', 45.0)), float(cfg.get('trans_mag', 0.5))


def modelnet_train_batch(points, cfg, seed, step, *, jitter_scale=0.01, jitter_clip=0.05):
    """One ModelNet training batch from B resident raw clouds (csrc/augment_modelnet.hip): the chain data_loaders/modelnet.py:102-109
    composes for noise_type `crop` (data_loaders/modelnet_transforms.py),
        SplitSourceRef -> RandomCrop(partial) -> RandomTransformSE3_euler(rot_mag, trans_mag) -> Resampler(num_points) -> RandomJitter
        -> ShufflePoints
    with the ground-truth overlap masks the crop itself defines (:219-228: a source point overlaps iff the reference's crop kept the same
    raw point, and the other way round; no radius search).  The result goes straight into RegTR.training_step.

    points: list (B) of device float32 (n_b, 3) clouds, n_b >= 2, of any lengths.  cfg keys read: partial, num_points, rot_mag, trans_mag,
    noise_type (the reference's defaults when absent).  -> 'src_xyz', 'tgt_xyz', 'src_overlap', 'tgt_overlap' (lists (B) of views into
    packed outputs, every cloud MODELNET_RESAMPLE = 717 rows: the reference's Resampler sets both sizes to 717 with a two-element
    `partial`, :92-93, whatever num_points says, so no length has to be read back), 'pose' (B, 3, 4), and '_augment' = {'dirs' (2B, 3)
    float32 crop directions and 'centroid' (2B, 3) per slot (source slots, then reference slots), 'thr' (2B,) float64, 'count' (2B,)
    int32 kept rows, 'flag' (2B,) int32, 'keep' (list (2B) of bool masks over the raw rows), 'rows' (2B, 717) int32: the raw row of
    every output row, 'perm' the stable sort's indices (resample order of every slot's raw rows, then the shuffle of every slot's output
    rows), 'xform' (B, 3, 4) the source's transform, 'slot_off' (host)}.

    Random numbers: the Philox convention above with purposes 3-7 (csrc/augment_modelnet.hip states which word feeds which decision;
    tests/modelnet_augment_ref.py restates it).  Five launches and one radix sort: draws, crop select, keys, torch.sort(stable=True),
    gather.  Bit-reproducible, no floating-point atomics, no host wait.

    A crop that keeps nothing (possible only when every distance from the percentile's rank up ties at the maximum, e.g. coincident
    points) makes the reference raise inside np.random.choice (:127); the device cannot raise without a read-back, so it keeps the whole
    cloud and sets the slot's 'flag'.

    Not built: `correspondences`, `corr_xyz`, `tgt_raw` (no loss reads them); the test-time transforms (they re-seed numpy's generator per
    item); a one-element `partial`, partial[0] = 0.5 and noise_type other than `crop` (NotImplementedError naming the value).  The
    reference's own `clean` and `jitter` training chains cannot run under its dataset class: ModelNetHdf.__getitem__
    (data_loaders/modelnet.py:179-180) and Resampler (:111-112) read `src_overlap` / `ref_overlap`, which only RandomCrop writes.
    Refused: CPU tensors, empty clouds, clouds that are not (n, 3) float32, n < 2."""
    p_keep, rot_mag, trans_mag = _check_modelnet_cfg(cfg)
    points = list(points)
    if not points:
        raise RuntimeError('modelnet_train_batch: points must be a non-empty list of clouds')
    for b, c in enumerate(points):
        if not isinstance(c, torch.Tensor) or c.device.type != 'cuda':
            raise RuntimeError(f'modelnet_train_batch: points[{b}] must be a GPU tensor (got {getattr(c, "device", type(c))}); there is no CPU fallback')
        if c.dim() != 2 or c.shape[1] != 3 or c.dtype is not torch.float32:
            raise RuntimeError(f'modelnet_train_batch: points[{b}] must be a float32 (n, 3) cloud, got {c.dtype} {tuple(c.shape)}')
        if c.shape[0] == 0:
            raise RuntimeError(f'modelnet_train_batch: points[{b}] is empty; an empty cloud has no centroid and no crop')
        if c.shape[0] < 2:
            raise RuntimeError(f'modelnet_train_batch: points[{b}] has {c.shape[0]} point; the percentile of the crop needs n >= 2')
    B, k = len(points), MODELNET_RESAMPLE
    dev = points[0].device
    lens = [int(c.shape[0]) for c in points]
    raw_off = np.concatenate([[0], np.cumsum(lens)])
    slot_off = np.concatenate([[0], np.cumsum(lens + lens)])
    n_raw, n_slot_rows = int(raw_off[-1]), int(slot_off[-1])
    if n_slot_rows + 2 * B * k >= 2 ** 31:
        raise RuntimeError(f'modelnet_train_batch: {n_slot_rows + 2 * B * k} sort keys exceed the int32 row index')
    sel = [crop_quantile(n, p_keep) for n in lens]
    with _lib.on_device(dev):
        meta = torch.from_numpy(np.concatenate([raw_off, slot_off, [s[0] for s in sel] * 2]).astype(np.int32)).to(dev, non_blocking=True)
        d_raw_off, d_slot_off, d_lo = meta[:B + 1], meta[B + 1:3 * B + 2], meta[3 * B + 2:]
        d_t = torch.from_numpy(np.array([s[1] for s in sel] * 2, dtype=np.float64)).to(dev, non_blocking=True)
        xyz = torch.cat(points, dim=0)
        dirs, xform, pose = ops.modelnet_draws(B, seed, step, rot_mag, trans_mag, dev)
        centroid, thr, count, flag, keep = ops.crop_select(xyz, d_raw_off, max(lens), dirs, d_lo, d_t, d_slot_off, n_slot_rows)
        perm = torch.sort(ops.modelnet_keys(d_slot_off, n_slot_rows, k, keep, seed, step), stable=True)[1]
        out, out_mask, rows = ops.modelnet_gather(xyz, d_raw_off, d_slot_off, n_slot_rows, k, perm, count, keep, xform, jitter_scale,
                                                  jitter_clip, seed, step)
    xs, ms = list(out.view(2 * B, k, 3).unbind(0)), list(out_mask.view(torch.bool).view(2 * B, k).unbind(0))
    return {'src_xyz': xs[:B], 'tgt_xyz': xs[B:], 'pose': pose, 'src_overlap': ms[:B], 'tgt_overlap': ms[B:],
            '_augment': {'dirs': dirs, 'centroid': centroid, 'thr': thr, 'count': count, 'flag': flag,
                         'keep': list(torch.split(keep.view(torch.bool), lens + lens)), 'rows': rows.view(2 * B, k), 'perm': perm,
                         'xform': xform, 'slot_off': [int(v) for v in slot_off]}}
