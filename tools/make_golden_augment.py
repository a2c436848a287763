"""Generates tests/golden/augment_ref_chain.npz by running the REAL reference augmentation chain (data_loaders/transforms.py: RigidPerturb ->
Jitter -> ShufflePoints -> RandomSwap, as data_loaders/__init__.py:18-23 composes it for 3DMatch training) on seeded toy pairs, recording
every value its random generators returned.  Runs where the reference tree is present (oracle/ref_loader.py: REF_SRC); the fixture holds
inputs, recorded draws and outputs -- data only.

transforms.py is loaded by file path: the package's __init__ imports h5py, which the chain itself does not need.

Per case c (a perturb mode and a pair): src_<c>, tgt_<c> (n, 3) float32, pose_<c> (3, 4), src_overlap_<c>, tgt_overlap_<c>; the draws
P_<c> (what SE3.sample_small / _sample_pose_large returned, 4x4 / 3x4 float64), perturb_source_<c>, swap_<c> (the thresholded
random.random() values), euler_<c> (large: the three angles, np.random.rand(3) 2 pi), noise_src_<c>, noise_tgt_<c> (torch.randn's values, before the scale), src_idx_<c>, tgt_idx_<c> (np.random.permutation
truncated to max_pts); the outputs out_src_<c>, out_tgt_<c>, out_pose_<c>, out_src_overlap_<c>, out_tgt_overlap_<c>.  mode_<c>, plus the
scalars n_cases, max_pts, augment_noise.

    python tools/make_golden_augment.py
"""
import importlib.util
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_loader import REF_SRC      # noqa: E402

MAX_PTS = 100
NOISE = 0.005
N_PAIRS = 8
MODES = ('small', 'large', 'none')


def load_transforms():
    sys.path.insert(0, REF_SRC)
    spec = importlib.util.spec_from_file_location('ref_transforms', os.path.join(REF_SRC, 'data_loaders', 'transforms.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def toy_pair(rng):
    """A seeded pair of 40-300 points each with a rigid ground-truth pose and random masks."""
    ns, nt = int(rng.integers(40, 301)), int(rng.integers(40, 301))
    src = rng.uniform(-1.5, 1.5, (ns, 3)).astype(np.float32)
    tgt = rng.uniform(-1.5, 1.5, (nt, 3)).astype(np.float32)
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    pose = np.concatenate([R, rng.uniform(-1, 1, (3, 1))], axis=1).astype(np.float32)
    return src, tgt, pose, rng.random(ns) > 0.5, rng.random(nt) > 0.5


def pick_seed(mode, p):
    """The first seed from 1000 * mode + 10 * p on whose two random.random() values give pair p the combination p % 4 of (source / target
    perturbed) x (swapped / not): the eight pairs of a mode cover every combination twice."""
    seed = 1000 * MODES.index(mode) + 10 * p
    while mode != 'none':
        random.seed(seed)
        if (random.random() > 0.5, random.random() > 0.5) == (bool(p & 1), bool(p & 2)):
            break
        seed += 1
    return seed


class Recorder:
    """Wraps the generators the chain draws from so that what they return is kept."""

    def __init__(self, T):
        self.T = T
        self.log = {'P': None, 'euler': None, 'u': [], 'randn': [], 'perm': []}

    def __enter__(self):
        T, log = self.T, self.log
        self.saved = (T.SE3.sample_small, T.RigidPerturb._sample_pose_large, T.random.random, T.torch.randn, T.np.random.permutation, T.np.random.rand)
        sample_small, sample_large, rnd, randn, permutation, rand = self.saved

        def rec_small(*a, **k):
            out = sample_small(*a, **k)
            log['P'] = np.array(out.as_matrix(), dtype=np.float64)
            return out

        def rec_large():
            out = sample_large()
            log['P'] = out.numpy().astype(np.float64)
            return out

        def rec_random():
            v = rnd()
            log['u'].append(v)
            return v

        def rec_randn(*a, **k):
            v = randn(*a, **k)
            log['randn'].append(v.numpy().copy())
            return v

        def rec_perm(n):
            v = permutation(n)
            log['perm'].append(np.array(v))
            return v
        def rec_rand(*a):
            v = rand(*a)
            log['euler'] = np.array(v)
            return v
        T.np.random.rand = rec_rand
        T.SE3.sample_small = staticmethod(rec_small)
        T.RigidPerturb._sample_pose_large = staticmethod(rec_large)
        T.random.random, T.torch.randn, T.np.random.permutation = rec_random, rec_randn, rec_perm
        return log

    def __exit__(self, *exc):
        T = self.T
        T.SE3.sample_small, T.RigidPerturb._sample_pose_large = staticmethod(self.saved[0]), staticmethod(self.saved[1])
        T.random.random, T.torch.randn, T.np.random.permutation, T.np.random.rand = self.saved[2:]


def main():
    T = load_transforms()
    out = {'max_pts': MAX_PTS, 'augment_noise': NOISE}
    combos = set()
    c = 0
    for mode in MODES:
        chain = [T.RigidPerturb(perturb_mode=mode), T.Jitter(scale=NOISE), T.ShufflePoints(max_pts=MAX_PTS), T.RandomSwap()]
        for p in range(N_PAIRS):
            seed = pick_seed(mode, p)
            rng = np.random.default_rng(p)                 # the same eight pairs under every mode
            random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
            src, tgt, pose, so, to = toy_pair(rng)
            data = {'src_xyz': torch.from_numpy(src.copy()), 'tgt_xyz': torch.from_numpy(tgt.copy()), 'pose': torch.from_numpy(pose.copy()),
                    'src_overlap': torch.from_numpy(so.copy()), 'tgt_overlap': torch.from_numpy(to.copy()), 'src_path': 's', 'tgt_path': 't'}
            with Recorder(T) as log:
                for t in chain:
                    data = t(data)
            us = list(log['u'])
            perturb_source = (us.pop(0) > 0.5) if mode != 'none' else False
            swap = us.pop(0) > 0.5
            assert not us and len(log['randn']) == 2 and len(log['perm']) == 2
            if mode != 'none':
                combos.add((mode, perturb_source, swap))
            P = log['P'] if log['P'] is not None else np.eye(4)
            out.update({f'mode_{c}': mode, f'src_{c}': src, f'tgt_{c}': tgt, f'pose_{c}': pose, f'src_overlap_{c}': so, f'tgt_overlap_{c}': to,
                        f'P_{c}': P, f'perturb_source_{c}': perturb_source, f'swap_{c}': swap,
                        f'noise_src_{c}': log['randn'][0], f'noise_tgt_{c}': log['randn'][1],
                        f'src_idx_{c}': log['perm'][0][:MAX_PTS], f'tgt_idx_{c}': log['perm'][1][:MAX_PTS],
                        f'out_src_{c}': data['src_xyz'].numpy(), f'out_tgt_{c}': data['tgt_xyz'].numpy(), f'out_pose_{c}': data['pose'].numpy(),
                        f'out_src_overlap_{c}': data['src_overlap'].numpy(), f'out_tgt_overlap_{c}': data['tgt_overlap'].numpy()})
            if mode == 'large':
                out[f'euler_{c}'] = 2 * np.pi * log['euler']        # transforms.py:29: anglez, angley, anglex
            c += 1
    out['n_cases'] = c
    for mode in ('small', 'large'):
        assert {(ps, sw) for m, ps, sw in combos if m == mode} == {(a, b) for a in (False, True) for b in (False, True)}, (mode, combos)
    dst = os.path.join(ROOT, 'tests', 'golden', 'augment_ref_chain.npz')
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), 'bytes,', c, 'cases')


if __name__ == '__main__':
    main()
