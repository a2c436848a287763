"""Generates tests/golden/modelnet_augment_ref_chain.npz by running the REAL reference ModelNet training chain
(data_loaders/modelnet_transforms.py: SplitSourceRef -> RandomCrop -> RandomTransformSE3_euler -> Resampler -> RandomJitter -> ShufflePoints,
as data_loaders/modelnet.py:102-109 composes it for noise_type `crop`) on seeded toy clouds, recording every value its random generators
returned.  Runs where the reference tree is present (oracle/ref_loader.py: REF_SRC); the fixture holds inputs, recorded draws and outputs
-- data only.

modelnet_transforms.py is loaded by file path: the package's __init__ imports h5py, which the chain itself does not need.

Per case c: points_<c> (n, 3) float32, centroid_<c> (np.mean of it as RandomCrop.crop takes it, float32); the draws dir_src_<c>, dir_ref_<c> (what uniform_2_sphere returned, float64), angles_<c> (anglex,
angley, anglez), transform_<c> (what generate_transform returned, (3, 4) float32), src_rand_idx_<c>, ref_rand_idx_<c> (Resampler._resample's
rows of the CROPPED clouds), noise_src_<c>, noise_ref_<c> (np.random.normal's values, before the clip), perm_src_<c>, perm_ref_<c>
(np.random.permutation); what the chain computed on the way: src_mask_<c>, ref_mask_<c> (the masks RandomCrop.crop returned, over the raw rows); the outputs out_src_<c>, out_ref_<c>, out_pose_<c>,
out_src_overlap_<c>, out_ref_overlap_<c>.  Scalars: n_cases, p_keep, rot_mag, trans_mag, num_points, jitter_scale, jitter_clip.

A case is REJECTED (the next seed is tried) when any point's distance from the crop plane lies within 2 dist_bound(same_centroid) of the threshold in the
restatement (tests/modelnet_augment_ref.py) cropping with the recorded centroid: the dot product's rounding then cannot put a point on the other side, and the
fixture's mask comparison cannot hinge on a rounding.  tests/test_modelnet_augment_host.py asserts the margin.

    python tools/make_golden_modelnet_augment.py
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_loader import REF_SRC      # noqa: E402
from tests import modelnet_augment_ref as M      # noqa: E402

P_KEEP, ROT_MAG, TRANS_MAG, NUM_POINTS = [0.7, 0.7], 45.0, 0.5, 1024      # conf/modelnet.yaml
SIZES = [2048, 2048, 2048, 2047, 300, 301, 257, 320]      # kept count above 717 (resample without replacement) / below (with); odd n


def load_transforms():
    sys.path.insert(0, REF_SRC)
    spec = importlib.util.spec_from_file_location('ref_modelnet_transforms', os.path.join(REF_SRC, 'data_loaders', 'modelnet_transforms.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def toy_cloud(rng, n):
    """Seeded points on a box and a sphere, roughly ModelNet's normalisation (inside the unit ball)."""
    a = n // 2
    box = rng.uniform(-0.5, 0.5, (a, 3)) * np.array([1.0, 0.6, 0.3])
    face = rng.integers(0, 3, a)
    box[np.arange(a), face] = np.sign(box[np.arange(a), face]) * 0.5 * np.array([1.0, 0.6, 0.3])[face]
    v = rng.standard_normal((n - a, 3))
    ball = 0.35 * v / np.linalg.norm(v, axis=1, keepdims=True) + np.array([0.2, 0.1, 0.25])
    return np.concatenate([box, ball]).astype(np.float32)[rng.permutation(n)]


class Recorder:
    """Wraps the generators the chain draws from so that what they return is kept."""

    def __init__(self, T):
        self.T = T
        self.log = {'dirs': [], 'uniform': [], 'transform': None, 'rand_idx': [], 'normal': [], 'perm': [], 'crop_mask': []}

    def __enter__(self):
        T, log = self.T, self.log
        rnd = T.np.random
        self.saved = (T.uniform_2_sphere, rnd.uniform, rnd.normal, rnd.permutation, T.Resampler._resample, T.RandomCrop.crop,
                      T.RandomTransformSE3_euler.generate_transform)
        sphere, uniform, normal, permutation, resample, crop, gen = self.saved

        def rec_sphere(*a, **k):
            v = sphere(*a, **k)
            log['dirs'].append(np.array(v, dtype=np.float64))
            return v

        def rec_uniform(*a, **k):
            v = uniform(*a, **k)
            log['uniform'].append(np.array(v, dtype=np.float64))
            return v

        def rec_normal(*a, **k):
            v = normal(*a, **k)
            log['normal'].append(np.array(v, dtype=np.float64))
            return v

        def rec_perm(n):
            v = permutation(n)
            log['perm'].append(np.array(v))
            return v

        def rec_resample(points, k):
            p, idx = resample(points, k)
            log['rand_idx'].append(np.array(idx))
            return p, idx

        def rec_crop(points, p_keep):
            p, mask = crop(points, p_keep)
            log['crop_mask'].append(np.array(mask))
            return p, mask

        def rec_gen(self_):
            v = gen(self_)
            log['transform'] = np.array(v)
            return v
        T.uniform_2_sphere, rnd.uniform, rnd.normal, rnd.permutation = rec_sphere, rec_uniform, rec_normal, rec_perm
        T.Resampler._resample, T.RandomCrop.crop = staticmethod(rec_resample), staticmethod(rec_crop)
        T.RandomTransformSE3_euler.generate_transform = rec_gen
        return log

    def __exit__(self, *exc):
        T, rnd = self.T, self.T.np.random
        T.uniform_2_sphere, rnd.uniform, rnd.normal, rnd.permutation = self.saved[:4]
        T.Resampler._resample, T.RandomCrop.crop = staticmethod(self.saved[4]), staticmethod(self.saved[5])
        T.RandomTransformSE3_euler.generate_transform = self.saved[6]


def run_case(T, chain, points, seed):
    np.random.seed(seed)
    sample = {'points': points.copy(), 'label': 0, 'idx': np.array(0, dtype=np.int32)}
    with Recorder(T) as log:
        for t in chain:
            sample = t(sample)
    # the uniform calls, in order: crop src (phi, cos), crop ref (phi, cos), three angles, the translation
    assert len(log['uniform']) == 8 and len(log['dirs']) == 2 and len(log['rand_idx']) == 2 and len(log['normal']) == 2
    assert len(log['perm']) == 2 and len(log['crop_mask']) == 2
    angles = np.array([float(u) for u in log['uniform'][4:7]]) * np.pi * ROT_MAG / 180.0
    return {'points': points, 'centroid': np.mean(points[:, :3], axis=0),                   # :191, the float32 mean both crops take
            'dir_src': log['dirs'][0], 'dir_ref': log['dirs'][1], 'angles': angles, 'transform': log['transform'],
            'src_rand_idx': log['rand_idx'][0], 'ref_rand_idx': log['rand_idx'][1], 'noise_src': log['normal'][0], 'noise_ref': log['normal'][1],
            'perm_ref': log['perm'][0], 'perm_src': log['perm'][1],                          # :380-381: the reference's is drawn first
            'src_mask': log['crop_mask'][0], 'ref_mask': log['crop_mask'][1],
            'out_src': sample['points_src'], 'out_ref': sample['points_ref'], 'out_pose': sample['transform_gt'],
            'out_src_overlap': sample['src_overlap'], 'out_ref_overlap': sample['ref_overlap']}


def margin_ok(case):
    e = M.dist_bound(case['points'], same_centroid=True)
    for s in ('src', 'ref'):
        c = M.crop(case['points'], case[f'dir_{s}'], P_KEEP[0], centroid=case['centroid'])
        if np.abs(c['dist'] - c['thr']).min() <= 2 * e:
            return False
    return True


def main():
    T = load_transforms()
    chain = [T.SplitSourceRef(), T.RandomCrop(P_KEEP), T.RandomTransformSE3_euler(rot_mag=ROT_MAG, trans_mag=TRANS_MAG),
             T.Resampler(NUM_POINTS), T.RandomJitter(), T.ShufflePoints()]
    out = {'p_keep': P_KEEP[0], 'rot_mag': ROT_MAG, 'trans_mag': TRANS_MAG, 'num_points': NUM_POINTS,
           'jitter_scale': chain[4].scale, 'jitter_clip': chain[4].clip, 'n_cases': len(SIZES)}
    for c, n in enumerate(SIZES):
        points = toy_cloud(np.random.default_rng(c), n)
        seed = 100 * c
        while True:
            case = run_case(T, chain, points, seed)
            if margin_ok(case):
                break
            seed += 1
        print(f'case {c}: n {n}, seed {seed}, kept {int(case["src_mask"].sum())} / {int(case["ref_mask"].sum())}')
        out.update({f'{k}_{c}': v for k, v in case.items()})
    dst = os.path.join(ROOT, 'tests', 'golden', 'modelnet_augment_ref_chain.npz')
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), 'bytes,', len(SIZES), 'cases')


if __name__ == '__main__':
    main()
