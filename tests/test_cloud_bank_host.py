"""CPU: the host side of the cloud bank -- harness.plan_windows on hand-made key lists, the C ABI's declaration and binding of
regtr_gather_segments, the fragment protocol of the pair sources, synthetic.synth_fragments."""
import os
import pickle
import re

import numpy as np
import pytest

from tests.util import ROOT


def _keys(s):
    """'ab cd' -> [('a', 'b'), ('c', 'd')]."""
    return [(p[0], p[1]) for p in s.split()]


def _replay(pair_keys, batch, cap):
    """Runs a plan the way run_test_shared does, on key lists instead of clouds; checks every index against the bank as it stands."""
    from regtr_amd.harness import plan_windows
    bank, covered, encoded, plan = [], [], [], []
    for w in plan_windows(pair_keys, batch, cap):
        plan.append(w)
        if w['keep'] is not None:
            assert w['keep'] == sorted(set(w['keep'])) and all(0 <= i < len(bank) for i in w['keep'])
            assert sorted(w['evict']) == sorted(bank[i] for i in range(len(bank)) if i not in w['keep'])
            bank = [bank[i] for i in w['keep']]
        else:
            assert w['evict'] == []
        assert not set(w['encode']) & set(bank) and len(set(w['encode'])) == len(w['encode'])
        bank = bank + w['encode']
        encoded += w['encode']
        assert len(bank) <= cap
        win = pair_keys[w['first']:w['first'] + w['count']]
        assert len(w['src']) == len(w['tgt']) == len(win)
        for (s, t), i, j in zip(win, w['src'], w['tgt']):
            assert 0 <= i < len(bank) and 0 <= j < len(bank)
            assert bank[i] == s and bank[j] == t
        covered += list(range(w['first'], w['first'] + w['count']))
    assert covered == list(range(len(pair_keys)))            # every pair once, in order
    return plan, encoded


def test_plan_windows_covers_every_pair_and_encodes_each_fragment_once_when_the_bank_is_large():
    pairs = _keys('ab ac bc ad cd aa ea eb fa')
    for batch in (1, 2, 4, 9, 20):
        plan, encoded = _replay(pairs, batch, 1024)
        assert sorted(encoded) == list('abcdef') and all(w['evict'] == [] and w['keep'] is None for w in plan)
        assert [w['count'] for w in plan] == [min(batch, len(pairs) - s) for s in range(0, len(pairs), batch)]
    from regtr_amd.harness import plan_windows
    assert list(plan_windows([], 4, 8)) == []


def test_plan_windows_exact_plan_under_capacity_pressure():
    """Two pairs per window, a bank of four clouds:
         window 0  ab ac   encode a b c                                                                      bank a b c
         window 1  ad bd   encode d                                                                          bank a b c d
         window 2  ea eb   e is missing, over by one: c (last read in window 0) is the least recently used   bank a b d e
         window 3  ec cd   c is missing, over by one: a and b (both last read in window 2) may go, d and e
                           are read here; a stands earlier in the bank                                       bank b d e c"""
    pairs = _keys('ab ac ad bd ea eb ec cd')
    plan, encoded = _replay(pairs, 2, 4)
    assert plan == [
        {'first': 0, 'count': 2, 'evict': [], 'keep': None, 'encode': ['a', 'b', 'c'], 'src': [0, 0], 'tgt': [1, 2]},
        {'first': 2, 'count': 2, 'evict': [], 'keep': None, 'encode': ['d'], 'src': [0, 1], 'tgt': [3, 3]},
        {'first': 4, 'count': 2, 'evict': ['c'], 'keep': [0, 1, 3], 'encode': ['e'], 'src': [3, 3], 'tgt': [0, 1]},
        {'first': 6, 'count': 2, 'evict': ['a'], 'keep': [1, 2, 3], 'encode': ['c'], 'src': [2, 3], 'tgt': [3, 1]},
    ]
    assert encoded == ['a', 'b', 'c', 'd', 'e', 'c']         # c comes back after its eviction: encoded twice


def test_plan_windows_evicts_least_recently_used_and_only_what_it_must():
    pairs = _keys('ab cd ab ef gh')                          # a, b are read again in window 2: c, d are the older ones when e, f arrive
    plan, encoded = _replay(pairs, 1, 5)
    assert plan[3]['evict'] == ['c'] and plan[3]['encode'] == ['e', 'f']          # over by one: one eviction, the oldest
    assert plan[4]['evict'] == ['d', 'a'] and plan[4]['encode'] == ['g', 'h']
    assert len(encoded) == 8


def test_plan_windows_refuses_a_capacity_below_one_windows_need():
    from regtr_amd.harness import plan_windows
    pairs = _keys('ab cd ef')
    with pytest.raises(ValueError, match='at least 4'):
        list(plan_windows(pairs, 2, 3))
    assert len(list(plan_windows(pairs, 2, 4))) == 2
    with pytest.raises(ValueError):
        list(plan_windows(pairs, 0, 4))


def test_gather_segments_is_declared_and_bound_and_the_abi_version_stays():
    from regtr_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'regtr_hip.h')).read()
    assert re.search(r'#define REGTR_ABI_VERSION 11\b', header) and _lib.ABI_VERSION == 11
    m = re.search(r'int regtr_gather_segments\(([^;]*)\);', header)
    assert m, 'regtr_gather_segments is not declared in include/regtr_hip.h'
    n_args = len([a for a in m.group(1).split(',') if a.strip()])
    res, args = _lib.SIGNATURES['regtr_gather_segments']
    assert res is _lib._I and len(args) == n_args == 16
    assert 'cloud_bank.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'cloud_bank.hip'))


def test_threedmatch_pairs_fragment_protocol(tmp_path):
    from regtr_amd.harness import ThreeDMatchPairs
    rng = np.random.default_rng(0)
    frags = {f'test/scene-a/cloud_bin_{k}.npy': rng.standard_normal((5 + k, 3)) for k in range(3)}
    os.makedirs(tmp_path / 'test' / 'scene-a')
    for rel, arr in frags.items():
        np.save(tmp_path / rel, arr)
    names = list(frags)
    infos = {'rot': [np.eye(3)] * 2, 'trans': [np.zeros((3, 1))] * 2, 'src': [names[1], names[2]], 'tgt': [names[0], names[1]], 'overlap': [0.5, 0.5]}
    with open(tmp_path / 'info.pkl', 'wb') as f:
        pickle.dump(infos, f)

    pairs = ThreeDMatchPairs(str(tmp_path / 'info.pkl'), str(tmp_path))
    assert pairs.fragment_keys(0) == (names[1], names[0]) and pairs.fragment_keys(1) == (names[2], names[1])
    for key, arr in frags.items():
        got = pairs.load_fragment(key)
        assert got.dtype == np.float32 and got.flags['C_CONTIGUOUS'] and np.array_equal(got, arr.astype(np.float32))
    item = pairs[0]
    assert np.array_equal(item['src_xyz'], pairs.load_fragment(pairs.fragment_keys(0)[0]))
    assert np.array_equal(item['tgt_xyz'], pairs.load_fragment(pairs.fragment_keys(0)[1]))


def test_synth_fragments_deterministic_with_consistent_poses():
    from regtr_amd.synthetic import synth_fragments
    frags, rel = synth_fragments(5, 4, 1500)
    again, rel2 = synth_fragments(5, 4, 1500)
    assert len(frags) == 4 and rel.shape == (4, 4, 4, 4) and np.array_equal(rel, rel2)
    assert all(a.dtype == np.float32 and a.shape[1] == 3 and len(a) > 500 and np.array_equal(a, b) for a, b in zip(frags, again))
    other, _ = synth_fragments(6, 4, 1500)
    assert not np.array_equal(other[0][:100], frags[0][:100])
    for a in range(4):
        assert np.abs(rel[a, a] - np.eye(4)).max() < 1e-12
        for b in range(4):
            R = rel[a, b, :3, :3]
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.allclose(rel[a, b, 3], [0, 0, 0, 1])
            for c in range(4):
                assert np.abs(rel[b, c] @ rel[a, b] - rel[a, c]).max() < 1e-6        # a -> b, then b -> c == a -> c
    # the poses are the clouds': neighbouring fragments moved into one frame lie on one another where they overlap
    from scipy.spatial import cKDTree
    moved = frags[0].astype(np.float64) @ rel[0, 1, :3, :3].T + rel[0, 1, :3, 3]
    d, _ = cKDTree(frags[1]).query(moved)
    assert np.mean(d < 0.03) > 0.3


def test_synthetic_scene_pairs_layout():
    from regtr_amd.harness import SyntheticScenePairs
    sp = SyntheticScenePairs(2, 4, 6, points=1500)
    assert len(sp) == 12
    keys = [sp.fragment_keys(i) for i in range(12)]
    assert len({k for pair in keys for k in pair}) == 8 and all(s != t for s, t in keys)
    assert keys[0] == ('test/synthetic-scene000/cloud_bin_0.pth', 'test/synthetic-scene000/cloud_bin_1.pth')
    assert keys[1][0].split('/')[1] == 'synthetic-scene001'
    it = sp[3]
    assert it['idx'] == 3 and (it['src_path'], it['tgt_path']) == keys[3] and it['pose'].shape == (3, 4) and it['pose'].dtype == np.float32
    assert np.array_equal(it['src_xyz'], sp.load_fragment(keys[3][0]))
    with pytest.raises(IndexError):
        sp.fragment_keys(12)


def test_synthetic_scene_pairs_pickles_and_reads_back_the_same_pairs():
    """LoaderPool.set_source pickles the pair source for its loader processes: the lock and the generated scenes stay behind."""
    from regtr_amd.harness import SyntheticScenePairs
    sp = SyntheticScenePairs(2, 4, 6, points=1500)
    before = sp[5]                                           # (a scene is generated and cached: the cache must not travel)
    blob = pickle.dumps(sp)
    assert len(blob) < 4096
    back = pickle.loads(blob)
    assert len(back) == len(sp) and back.cache_scenes == sp.cache_scenes
    for i in (0, 5, 11):
        a, b = sp[i], back[i]
        assert set(a) == set(b) == {'src_xyz', 'tgt_xyz', 'pose', 'idx', 'src_path', 'tgt_path'}
        assert (a['idx'], a['src_path'], a['tgt_path']) == (b['idx'], b['src_path'], b['tgt_path'])
        assert all(np.array_equal(a[k], b[k]) for k in ('src_xyz', 'tgt_xyz', 'pose'))
    assert np.array_equal(before['src_xyz'], back[5]['src_xyz'])


def test_synthetic_scene_pairs_meta_and_scene_numbers_beyond_three_digits():
    from regtr_amd.harness import SyntheticScenePairs
    from regtr_amd.synthetic import synth_fragment_poses, synth_fragments
    sp = SyntheticScenePairs(1002, 2, 1, points=600, cache_scenes=2)
    sk, tk = sp.fragment_keys(1000)                           # pair 0 of scene 1000
    assert (sk, tk) == ('test/synthetic-scene1000/cloud_bin_0.pth', 'test/synthetic-scene1000/cloud_bin_1.pth')
    frags, rel = synth_fragments(1000, 2, 600)
    assert np.array_equal(sp.load_fragment(sk), frags[0]) and np.array_equal(sp.load_fragment(tk), frags[1])
    assert not np.array_equal(sp.load_fragment(sk)[:50], sp.load_fragment('test/synthetic-scene000/cloud_bin_0.pth')[:50])
    m = sp.meta(1000)
    assert set(m) == {'pose', 'idx', 'src_path', 'tgt_path'} and np.array_equal(m['pose'], rel[0, 1, :3].astype(np.float32))
    assert np.array_equal(synth_fragment_poses(1000, 2)[1], rel)
    assert len(sp._scenes) <= 2                               # the cache is bounded: least recently used scenes go
    for bad in ('test/synthetic-scene1002/cloud_bin_0.pth', 'test/synthetic-scene000/cloud_bin_2.pth', 'test/other-scene000/cloud_bin_0.pth'):
        with pytest.raises(KeyError):
            sp.load_fragment(bad)
    sp2 = SyntheticScenePairs(3, 2, 1, points=600, cache_scenes=2)
    for s in (0, 1, 0, 2):                                    # 0 is used again before 2 arrives: 1 is the one dropped
        sp2.load_fragment(f'test/synthetic-scene{s:03d}/cloud_bin_0.pth')
    assert sorted(sp2._scenes) == [0, 2]
