"""CPU: the training augmentation's restatement (tests/augment_ref.py) -- the Philox known answers, the chain against the REAL reference
chain's recorded run (tests/golden/augment_ref_chain.npz, tools/make_golden_augment.py), the statistics of the draws -- and the host side
of regtr_amd/augment.py."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.util import gold, load_cfg

# the published Philox4x32-10 known-answer vectors (Random123 kat_vectors): counter, key, output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    from regtr_amd import augment
    for ctr, key, want in KAT:
        for f in (R.philox4x32, augment.philox4x32):
            got = f(np.array(ctr, dtype=np.uint64), key)
            assert [int(v) for v in got] == list(want), (f.__module__, ctr)
    # vectorised: the three at once under one key each
    got = R.philox4x32(np.array([KAT[0][0], KAT[0][0]], dtype=np.uint64), KAT[0][1])
    assert got.shape == (2, 4) and [int(v) for v in got[1]] == list(KAT[0][2])
    # the counter layout (index, slot, purpose, step) and the key split of a 64-bit seed
    seed = (KAT[2][1][1] << 32) | KAT[2][1][0]
    w = R.words(seed, KAT[2][0][3], np.array([KAT[2][0][0]]), np.array([KAT[2][0][1]]), KAT[2][0][2])
    assert [int(v) for v in w[0]] == list(KAT[2][2])


def test_uniforms_never_reach_the_ends():
    u = R.uniform(np.array([0, 0xff, 0x100, 0xffffffff], dtype=np.uint32))
    assert u[0] == u[1] == 2.0 ** -25 and u[2] == 1.5 * 2.0 ** -24 and u[3] == 1.0 - 2.0 ** -25


def _cases():
    g = gold('augment_ref_chain')
    for c in range(int(g['n_cases'])):
        pair = {'src_xyz': g[f'src_{c}'], 'tgt_xyz': g[f'tgt_{c}'], 'pose': g[f'pose_{c}'], 'src_overlap': g[f'src_overlap_{c}'],
                'tgt_overlap': g[f'tgt_overlap_{c}']}
        d = {'P': g[f'P_{c}'], 'perturb_source': bool(g[f'perturb_source_{c}']), 'swap': bool(g[f'swap_{c}']),
             'src_idx': g[f'src_idx_{c}'], 'tgt_idx': g[f'tgt_idx_{c}'], 'noise_src': g[f'noise_src_{c}'], 'noise_tgt': g[f'noise_tgt_{c}']}
        out = {k: g[f'out_{k}_{c}'] for k in ('src', 'tgt', 'pose', 'src_overlap', 'tgt_overlap')}
        yield c, str(g[f'mode_{c}']), pair, d, out, float(g['augment_noise']), int(g['max_pts'])


def test_fixture_covers_the_chain():
    cases = list(_cases())
    assert len(cases) >= 8
    for mode in ('small', 'large'):
        combos = {(d['perturb_source'], d['swap']) for _, m, _, d, _, _, _ in cases if m == mode}
        assert combos == {(a, b) for a in (False, True) for b in (False, True)}, mode
    assert {m for _, m, *_ in cases} == {'small', 'large', 'none'}
    sizes = [len(p[k]) for _, _, p, *_ in cases for k in ('src_xyz', 'tgt_xyz')]
    max_pts = cases[0][6]
    assert min(sizes) >= 40 and max(sizes) <= 300 and min(sizes) < max_pts < max(sizes)      # truncated and untruncated clouds


def test_chain_equals_the_reference_run():
    """apply(pair, recorded draws) against what the reference's four transforms returned: selection, masks and swap exactly, clouds and
    pose within the derived float32 bound (augment_ref.bounds).  Pins the pose composition order and the recentring."""
    worst = 0.0
    for c, mode, pair, d, ref, noise, max_pts in _cases():
        got = R.apply(pair, d, augment_noise=noise, perturb_pose=mode, noise_on_output=False)
        bd = R.bounds(pair, d, augment_noise=noise, perturb_pose=mode)
        a, b = ('tgt', 'src') if d['swap'] else ('src', 'tgt')        # the INPUT cloud behind the output's src / tgt
        for out_key, in_key in (('src', a), ('tgt', b)):
            assert got[f'{out_key}_xyz'].shape == ref[out_key].shape == (min(len(pair[f'{in_key}_xyz']), max_pts), 3), (c, out_key)
            assert np.array_equal(got[f'{out_key}_overlap'], ref[f'{out_key}_overlap']), (c, out_key)
            tol = bd['perturbed'] if (mode != 'none' and in_key == bd['which']) else bd['other']
            err = np.abs(got[f'{out_key}_xyz'] - ref[out_key].astype(np.float64)).max()
            worst = max(worst, err / tol)
            assert err <= tol, (c, mode, out_key, err, tol)
        eR = np.abs(got['pose'][:, :3] - ref['pose'][:, :3].astype(np.float64)).max()
        et = np.abs(got['pose'][:, 3] - ref['pose'][:, 3].astype(np.float64)).max()
        worst = max(worst, et / max(bd['pose_t'], 1e-30) if bd['pose_t'] else 0.0)
        assert eR <= bd['pose_R'] and et <= bd['pose_t'], (c, mode, eR, bd['pose_R'], et, bd['pose_t'])
        assert ref['pose'].shape == (3, 4)
    print(f'largest error / bound over the fixture: {worst:.3f}')
    # the bound is not slack enough to hide a wrong composition: the other order of :57 / :65 misses it by orders of magnitude
    c, mode, pair, d, ref, noise, _ = next(x for x in _cases() if x[1] == 'small' and x[3]['perturb_source'] and not x[3]['swap'])
    P = R.apply(pair, d, noise, mode, False)['xform_src']
    wrong = R.se3_cat(R.se3_inv(P), np.asarray(pair['pose'], dtype=np.float64)[:3])
    assert np.abs(wrong - ref['pose']).max() > 1e2 * R.bounds(pair, d, noise, mode)['pose_t']


def test_draw_statistics():
    """1e5 samples each: normals N(0, 1), axes without a preferred direction, fair flags; every sorted-key segment a bijection."""
    n = 100000
    d = R.pair_draws(seed=2024, step=7, B=n, perturb_pose='small')
    z = d['z'].ravel()                                               # 4e5 normals: block 1 of every pair
    m = z.size
    assert abs(z.mean()) <= 4 / np.sqrt(m) and abs(z.var() - 1) <= 4 * np.sqrt(2.0 / m)
    zj = R.jitter_normals(2024, 7, [n // 4] * 4).ravel()             # the jitter's stream (purpose 2)
    assert abs(zj.mean()) <= 4 / np.sqrt(zj.size) and abs(zj.var() - 1) <= 4 * np.sqrt(2.0 / zj.size)
    ax = d['axis']
    assert np.allclose(np.linalg.norm(ax, axis=1), 1.0, atol=1e-12)
    assert (np.abs(ax.mean(axis=0)) <= 4 * np.sqrt(1.0 / 3.0 / n)).all()            # a uniform direction's component has variance 1/3
    for k in ('perturb_source', 'swap'):
        assert abs(d[k].mean() - 0.5) <= 4 * 0.5 / np.sqrt(n), k
    assert abs((d['perturb_source'] & d['swap']).mean() - 0.25) <= 4 * np.sqrt(0.25 * 0.75 / n)       # ... and independent of each other
    # the perturbation is a rotation of about std pi / sqrt(3) and a translation of std / sqrt(3) per axis
    P = d['P']
    assert np.allclose(P[:, :, :3] @ P[:, :, :3].transpose(0, 2, 1), np.eye(3), atol=1e-12)
    ang = np.arccos(np.clip((np.trace(P[:, :, :3], axis1=1, axis2=2) - 1) / 2, -1, 1))
    s_ang = R.PERTURB_STD * np.pi / np.sqrt(3.0)
    assert abs((ang ** 2).mean() / s_ang ** 2 - 1) <= 4 * np.sqrt(2.0 / n)
    assert abs(P[:, :, 3].var() / (R.PERTURB_STD ** 2 / 3) - 1) <= 4 * np.sqrt(2.0 / (3 * n))
    # shuffle: 100 clouds of 1000 rows and a few odd ones
    sizes = [1000] * 100 + [1, 2, 63, 65]
    perm = R.shuffle_perm(2024, 7, sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    fixed = 0
    for c, s in enumerate(sizes):
        seg = perm[off[c]:off[c + 1]]
        assert np.array_equal(np.sort(seg), np.arange(off[c], off[c + 1])), c
        fixed += int((seg == np.arange(off[c], off[c + 1])).sum()) if s == 1000 else 0
    assert fixed <= 100 + 4 * 10                                     # a random permutation has one fixed point on average (variance 1)
    assert not np.array_equal(perm, R.shuffle_perm(2024, 8, sizes)) and not np.array_equal(perm, R.shuffle_perm(2025, 7, sizes))


def test_large_perturbation_is_the_references_zyx():
    """The restated Euler composition against the angles and matrices recorded from the reference's _sample_pose_large."""
    g = gold('augment_ref_chain')
    seen = 0
    for c in range(int(g['n_cases'])):
        if str(g[f'mode_{c}']) == 'large':
            assert np.allclose(R.euler_zyx(*g[f'euler_{c}']), g[f'P_{c}'][:, :3], atol=2e-7) and not g[f'P_{c}'][:, 3].any()      # (stored as float32)
            seen += 1
    assert seen >= 4
    d = R.pair_draws(3, 1, 16, 'large')
    q = R.words(3, 1, np.zeros(16), np.arange(16), 0)
    assert np.array_equal(d['P'][:, :, :3], R.euler_zyx(*(2 * np.pi * R.uniform(q[:, i]) for i in range(3)))) and not d['P'][:, :, 3].any()


def test_draws_layout():
    d = R.draws(11, 3, ([1, 70, 300], [65, 257, 64]), max_pts=64)
    B = 3
    for b in range(B):
        ns, nt = [1, 70, 300][b], [65, 257, 64][b]
        assert len(d['src_idx'][b]) == min(ns, 64) and len(d['tgt_idx'][b]) == min(nt, 64)
        assert len(set(d['src_idx'][b])) == len(d['src_idx'][b]) and d['src_idx'][b].max() < ns
        lens = (len(d['tgt_idx'][b]), len(d['src_idx'][b])) if d['swap'][b] else (len(d['src_idx'][b]), len(d['tgt_idx'][b]))
        assert (len(d['noise_src'][b]), len(d['noise_tgt'][b])) == lens
    nos = R.draws(11, 3, ([5, 6], [7, 8]), shuffle=False, swap=False, max_pts=6)
    assert [list(i) for i in nos['tgt_idx']] == [list(range(6)), list(range(6))] and not nos['swap'].any()


def test_host_swap_flags_equal_the_restatement():
    from regtr_amd import augment
    for seed, step in ((0, 0), (5, 9), (2 ** 63 + 12345, 2 ** 31 + 1)):
        assert np.array_equal(augment.swap_flags(seed, step, 257), R.pair_draws(seed, step, 257, 'none')['swap'])


def test_refusals_and_config():
    from regtr_amd import augment, build
    assert 'augment.hip' in build.SOURCES and build.EXTRA['augment.hip'] == ['-ffp-contract=off']
    cfg = load_cfg('3dmatch')
    assert cfg.augment_noise == 0.005 and cfg.perturb_pose == 'small'            # the reference's conf/3dmatch.yaml values
    x = torch.rand(10, 3)
    cpu = {'src_xyz': [x], 'tgt_xyz': [x], 'pose': torch.eye(4)[None, :3], 'src_overlap': [x[:, 0] > 0.5], 'tgt_overlap': [x[:, 0] > 0.5]}
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        augment.augment_batch(cpu, 0, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        augment.train_batch([x], [x], torch.eye(4)[None, :3], cfg, 0, 0)
    with pytest.raises(RuntimeError, match='perturb_pose'):
        augment.augment_batch(cpu, 0, 0, perturb_pose='medium')
