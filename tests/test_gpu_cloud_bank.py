"""GPU (-m gpu): the cloud bank -- regtr_gather_segments against a numpy restatement, RegTR.encode_clouds + register against
RegTR.forward (bit for bit where the launches are the same, at forward's own batch-composition bar where they are not), against the
real reference module's golden, the bank's operations and refusals, and harness.run_test_shared against run_test."""
import os

import numpy as np
import pytest
import torch

from tests.util import gold, load_cfg, seeded_sd, seg_of, to_dev

pytestmark = pytest.mark.gpu

KEYS_LIST = ('src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp', 'src_kp_warped', 'tgt_kp_warped', 'src_overlap',
             'tgt_overlap')


def _model(cfg, sd=None):
    from regtr_amd import RegTR
    model = RegTR(cfg)
    model.load_state_dict(seeded_sd(cfg) if sd is None else sd, strict=True)
    return model.cuda().eval()


def _dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in clouds]


def _assert_dicts_equal(a, b):
    assert set(a) == set(b) == set(KEYS_LIST) | {'pose'}
    for k in KEYS_LIST:
        assert len(a[k]) == len(b[k]), k
        for x, y in zip(a[k], b[k]):
            assert x.shape == y.shape and torch.equal(x, y), f'{k} differs'
    assert torch.equal(a['pose'], b['pose']), 'pose differs'


# ------------------------------------------------------------------------------------------------ 1. the kernel against a restatement
BANK_LENS = [1, 31, 0, 33, 64, 65]
CLOUD_OF = [3, 3, 0, 5, 2, 1, 4, 0]          # repeats, the empty cloud, tile edges at 32, 64 and 65 rows


def _restate(x, seg, cloud_of):
    return np.concatenate([x[seg[c]:seg[c + 1]] for c in cloud_of])


@pytest.mark.parametrize('with_pe', [False, True])
@pytest.mark.parametrize('D', [64, 256])
def test_gather_segments_equals_the_numpy_restatement(D, with_pe):
    from regtr_amd import ops
    rng = np.random.default_rng(7 + D)
    seg = np.concatenate([[0], np.cumsum(BANK_LENS)]).astype(np.int32)
    N = int(seg[-1])
    x = rng.standard_normal((N, D)).astype(np.float32)
    pe = rng.standard_normal((N, D)).astype(np.float32) if with_pe else None
    xyz = rng.standard_normal((N, 3)).astype(np.float32)
    sel = [BANK_LENS[c] for c in CLOUD_OF]
    dst = np.concatenate([[0], np.cumsum(sel)]).astype(np.int32)
    n_out = int(dst[-1])
    nan = lambda w: torch.full((n_out, w), float('nan'), dtype=torch.float32, device='cuda')
    out = (nan(D), nan(D) if with_pe else None, nan(3))
    o_f, o_p, o_x = ops.gather_segments(to_dev(x), to_dev(seg), to_dev(np.asarray(CLOUD_OF, np.int32)), to_dev(dst), n_out, max(sel),
                                        pe=None if pe is None else to_dev(pe), xyz=to_dev(xyz), out=out)
    torch.cuda.synchronize()
    assert o_f.shape == (n_out, D) and o_x.shape == (n_out, 3) and (o_p is None) == (pe is None)
    for got, src in ((o_f, x), (o_p, pe), (o_x, xyz)):
        if src is None:
            continue
        got = got.cpu().numpy()
        assert not np.isnan(got).any()
        assert np.array_equal(got.view(np.uint32), _restate(src, seg, CLOUD_OF).view(np.uint32))
    # fresh outputs (no `out`): the same bits
    f2, _, x2 = ops.gather_segments(to_dev(x), to_dev(seg), to_dev(np.asarray(CLOUD_OF, np.int32)), to_dev(dst), n_out, max(sel), xyz=to_dev(xyz))
    assert torch.equal(f2, o_f) and torch.equal(x2, o_x)


def test_gather_segments_of_only_the_empty_cloud_launches_nothing():
    from regtr_amd import ops
    seg = np.concatenate([[0], np.cumsum(BANK_LENS)]).astype(np.int32)
    x = to_dev(np.ones((int(seg[-1]), 64), np.float32))
    o_f, o_p, o_x = ops.gather_segments(x, to_dev(seg), to_dev(np.asarray([2, 2], np.int32)), to_dev(np.zeros(3, np.int32)), 0, 0)
    torch.cuda.synchronize()
    assert o_f.shape == (0, 64) and o_p is None and o_x is None
    # ... with pe and xyz as well: the zero-row outputs have NULL bases, which a launch-free call must not look at
    pe, xyz = to_dev(np.ones((int(seg[-1]), 64), np.float32)), to_dev(np.ones((int(seg[-1]), 3), np.float32))
    for cloud_of in ([2, 2], []):
        dst = to_dev(np.zeros(len(cloud_of) + 1, np.int32))
        o_f, o_p, o_x = ops.gather_segments(x, to_dev(seg), to_dev(np.asarray(cloud_of, np.int32)), dst, 0, 0, pe=pe, xyz=xyz)
        assert o_f.shape == (0, 64) and o_p.shape == (0, 64) and o_x.shape == (0, 3)
    torch.cuda.synchronize()


def test_select_of_no_cloud_gives_an_empty_bank_that_cat_accepts(small):
    from regtr_amd import CloudBank
    _, model, clouds = small
    bank = model.encode_clouds(clouds[:2])
    none = bank.select([])
    assert len(none) == 0 and none.lens == () and none.feats.shape == (0, bank.feats.shape[1]) and none.xyz.shape == (0, 3)
    again = CloudBank.cat([none, bank])
    assert again.lens == bank.lens and torch.equal(again.seg_off, bank.seg_off)
    _assert_dicts_equal(model.register(again, [0], [1]), model.register(bank, [0], [1]))


def test_gather_segments_c_abi_refusals():
    """REGTR_ERR_ARG (-2), nothing launched: NULL pointers with work to do, D % 4 != 0, a misaligned wide base, pe without out_pe."""
    from regtr_amd import _lib
    L = _lib.lib()
    D = 64
    seg = seg_of([40, 24])
    x = torch.ones((64 + 1, D), dtype=torch.float32, device='cuda')
    out = torch.full((64 + 1, D), float('nan'), dtype=torch.float32, device='cuda')
    cloud_of = to_dev(np.asarray([1, 0], np.int32))
    dst = seg_of([24, 40])
    xp, op, sp, cp, dp = x.data_ptr(), out.data_ptr(), seg.data_ptr(), cloud_of.data_ptr(), dst.data_ptr()

    def call(feats=xp, pe=None, xyz=None, D=D, bank_seg=sp, cloud_of=cp, dst_seg=dp, out_feats=op, out_pe=None, out_xyz=None):
        return L.regtr_gather_segments(feats, pe, xyz, D, bank_seg, 2, 64, cloud_of, dst_seg, 2, 64, 40, out_feats, out_pe, out_xyz, None)
    assert call(feats=None) == -2 and call(out_feats=None) == -2
    assert call(bank_seg=None) == -2 and call(cloud_of=None) == -2 and call(dst_seg=None) == -2
    assert call(D=62) == -2 and call(D=0) == -2
    assert call(feats=xp + 4) == -2 and call(out_feats=op + 8) == -2
    assert call(pe=xp) == -2 and call(out_pe=op) == -2 and call(pe=xp + 4, out_pe=op) == -2
    assert call(xyz=xp) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), 'a refused call wrote'
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:64], torch.ones_like(out[:64])) and bool(torch.isnan(out[64:]).all())


# ------------------------------------------------------------------------------------------------ 2. the identity arrangement
def _identity_case(cfg, srcs, tgts, sd=None):
    model = _model(cfg, sd)
    batch = {'src_xyz': _dev(srcs), 'tgt_xyz': _dev(tgts)}
    ref = model(batch)
    B = len(srcs)
    bank = model.encode_clouds(batch['src_xyz'] + batch['tgt_xyz'])
    assert len(bank) == 2 * B and list(bank.lens) == [int(n) for n in batch['kpconv_meta']['_lens_host'][-1]]
    out = model.register(bank, list(range(B)), list(range(B, 2 * B)))
    torch.cuda.synchronize()
    _assert_dicts_equal(out, ref)
    return model, bank


def test_register_in_forwards_arrangement_equals_forward_bit_for_bit():
    """register(encode_clouds([s0, s1, t0, t1]), [0, 1], [2, 3]) == forward({src: [s0, s1], tgt: [t0, t1]}) on EVERY entry: the launches
    have the same shapes and the gather is a copy."""
    g = gold('3dmatch_crop_b2')
    _, bank = _identity_case(load_cfg('3dmatch'), [g['src_0'], g['src_1']], [g['tgt_0'], g['tgt_1']])
    assert bank.pe is not None and bank.nbytes == bank.xyz.numel() * 4 + 2 * bank.feats.numel() * 4 + 4 * 5


def test_register_identity_with_the_attention_valued_head():
    g = gold('modelnet_demo')
    cfg = load_cfg('modelnet')
    cfg.update({'direct_regress_coor': False})
    _identity_case(cfg, [g['src']], [g['tgt']])


def test_register_identity_with_the_learned_positional_embedding():
    g = gold('3dmatch_crop_b2')
    cfg = load_cfg('3dmatch')
    cfg.update({'pos_emb_type': 'learned'})
    from tests import posemb_mlp_ref as PR
    _identity_case(cfg, [g['src_0'], g['src_1']], [g['tgt_0'], g['tgt_1']], sd=PR.learned_state_dict(seeded_sd(cfg), cfg.d_embed))


# ------------------------------------------------------------------------------------------------ 3. composition and reuse
def test_register_composed_pairs_equal_forward_of_each_pair_alone():
    """A = src, B = tgt, C = tgt[:2500], D = src[:3000] of 3dmatch_crop, encoded in two calls ([D, B], [A, C]) and joined with cat; the
    pairs (A, B), (B, A), (A, C), (D, B), (C, D), (A, A) in ONE register against forward of each pair alone: key points bit-equal,
    warped points / overlap logits / pose within 1e-5 absolute -- the bar test_forward_batched_pairs_equal_single holds forward itself
    to across batch compositions.  Measured on an MI355X on these inputs (docs/PARITY.md): forward of the six pairs in one batch against
    forward of each pair alone differs by at most 3.1e-6 (the pose; 1.5e-6 on the warped points), the shared path by at most 2.4e-6
    (the pose; 8.3e-7 on the warped points)."""
    from regtr_amd import CloudBank
    g = gold('3dmatch_crop')
    cfg = load_cfg('3dmatch')
    model = _model(cfg)
    A, B, C, D = _dev([g['src'], g['tgt'], g['tgt'][:2500], g['src'][:3000]])
    bank = CloudBank.cat([model.encode_clouds([D, B]), model.encode_clouds([A, C])])
    assert len(bank) == 4
    at = {'D': 0, 'B': 1, 'A': 2, 'C': 3}
    clouds = {'A': A, 'B': B, 'C': C, 'D': D}
    pairs = ['AB', 'BA', 'AC', 'DB', 'CD', 'AA']
    out = model.register(bank, [at[p[0]] for p in pairs], [at[p[1]] for p in pairs])
    worst = 0.0
    for k, p in enumerate(pairs):
        one = model({'src_xyz': [clouds[p[0]]], 'tgt_xyz': [clouds[p[1]]]})
        assert torch.equal(out['src_kp'][k], one['src_kp'][0]) and torch.equal(out['tgt_kp'][k], one['tgt_kp'][0]), p
        for key in ('src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
            d = (out[key][k] - one[key][0]).abs().max().item()
            worst = max(worst, d)
            assert d < 1e-5, (p, key, d)
        d = (out['pose'][:, k] - one['pose'][:, 0]).abs().max().item()
        worst = max(worst, d)
        assert d < 1e-5, (p, 'pose', d)
    print(f'shared path vs forward of each pair alone: worst abs diff {worst:.2e}')


# ------------------------------------------------------------------------------------------------ 4. against the real reference
def test_register_vs_reference_golden_batch2_each_cloud_encoded_alone():
    """Parity mode on 3dmatch_crop_b2: each of the four clouds encoded in its OWN call, then one register, against the golden of the real
    reference module at test_forward_vs_reference_golden_batch2's bars: key points equal, the rest within 1e-4."""
    from regtr_amd import CloudBank
    g = gold('3dmatch_crop_b2')
    cfg = load_cfg('3dmatch')
    cfg.update({'kpconv_ref_row_order': True})
    model = _model(cfg)
    clouds = _dev([g['src_0'], g['src_1'], g['tgt_0'], g['tgt_1']])
    bank = CloudBank.cat([model.encode_clouds([c]) for c in clouds])
    out = model.register(bank, [0, 1], [2, 3])
    worst = {}
    for b in range(2):
        assert np.array_equal(out['src_kp'][b].cpu().numpy(), g[f'src_kp_{b}']) and np.array_equal(out['tgt_kp'][b].cpu().numpy(), g[f'tgt_kp_{b}'])
        for k in ('src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
            worst[k] = max(worst.get(k, 0.0), float(np.abs(out[k][b].cpu().numpy() - g[f'{k}_{b}']).max()))
    worst['pose'] = float(np.abs(out['pose'].cpu().numpy() - g['pose']).max())
    print('3dmatch_crop_b2, clouds encoded one by one: max abs diff vs the reference module:', {k: f'{v:.2e}' for k, v in worst.items()})
    assert max(worst.values()) < 1e-4, worst


# ------------------------------------------------------------------------------------------------ 5. bank operations and refusals
@pytest.fixture(scope='module')
def small():
    g = gold('3dmatch_crop_b2')
    cfg = load_cfg('3dmatch')
    model = _model(cfg)
    clouds = _dev([g['src_0'], g['src_1'], g['tgt_0'], g['tgt_1']])
    return cfg, model, clouds


def test_select_then_register_equals_register_with_remapped_indices(small):
    _, model, clouds = small
    bank = model.encode_clouds(clouds)
    keep = [3, 1, 0]                                    # drops cloud 2, reorders the rest
    sub = bank.select(keep)
    assert len(sub) == 3 and list(sub.lens) == [bank.lens[i] for i in keep] and sub.nbytes < bank.nbytes
    pairs = [(0, 3), (1, 0), (3, 3)]
    a = model.register(bank, [p[0] for p in pairs], [p[1] for p in pairs])
    b = model.register(sub, [keep.index(p[0]) for p in pairs], [keep.index(p[1]) for p in pairs])
    _assert_dicts_equal(a, b)


def test_encode_and_register_are_reproducible(small):
    _, model, clouds = small
    runs = []
    for _ in range(2):
        bank = model.encode_clouds(clouds[:3])           # an odd number of clouds
        runs.append(model.register(bank, [0, 2, 1], [1, 0, 1]))
    _assert_dicts_equal(runs[0], runs[1])


def test_refusals_launch_nothing(small, monkeypatch):
    from regtr_amd import CloudBank, ops
    from regtr_amd.optim import FusedAdamW
    cfg, model, clouds = small
    bank = model.encode_clouds(clouds)
    other = _model(cfg)
    other_bank = other.encode_clouds(clouds[:1])

    def boom(*a, **k):
        raise AssertionError('a refused call reached a launch')
    monkeypatch.setattr(ops, 'gather_segments', boom)
    monkeypatch.setattr(ops, 'gemm', boom)
    monkeypatch.setattr(model, '_backbone', boom)
    with pytest.raises(ValueError):
        model.register(bank, [], [])
    with pytest.raises(ValueError):
        model.register(bank, [0, 1], [2])
    with pytest.raises(IndexError):
        model.register(bank, [0], [4])
    with pytest.raises(IndexError):
        model.register(bank, [-1], [0])
    with pytest.raises(IndexError):
        bank.select([0, 7])
    with pytest.raises(TypeError):
        model.register({'feats': bank.feats}, [0], [1])
    with pytest.raises(RuntimeError, match='another model'):
        model.register(other_bank, [0], [0])
    with pytest.raises(RuntimeError, match='different'):
        CloudBank.cat([bank, other_bank])
    with pytest.raises(RuntimeError, match='HIP'):
        model.encode_clouds([c.cpu() for c in clouds])
    cpu_bank = CloudBank(bank.xyz.cpu(), bank.feats.cpu(), bank.pe.cpu(), bank.seg_off.cpu(), bank.lens, bank.stamp)
    with pytest.raises(RuntimeError, match='HIP'):
        model.register(cpu_bank, [0], [1])
    with pytest.raises(ValueError):
        model.encode_clouds([])
    if torch.cuda.device_count() > 1:
        moved = CloudBank(bank.xyz.to('cuda:1'), bank.feats.to('cuda:1'), bank.pe.to('cuda:1'), bank.seg_off.to('cuda:1'), bank.lens, bank.stamp)
        with pytest.raises(RuntimeError):
            model.register(moved, [0], [1])
    # stale after an optimiser step ...
    w = other.feat_proj.weight
    w.grad = torch.zeros_like(w)
    FusedAdamW([w], lr=0.0, weight_decay=0.0).step()
    monkeypatch.setattr(other, '_backbone', boom)
    with pytest.raises(RuntimeError, match='stale'):
        other.register(other_bank, [0], [0])
    # ... and after a load_state_dict
    model.load_state_dict(seeded_sd(cfg), strict=True)
    with pytest.raises(RuntimeError, match='stale'):
        model.register(bank, [0], [1])
    monkeypatch.undo()
    fresh = model.encode_clouds(clouds)                 # the same weights again: the same bits as the refused bank
    assert torch.equal(fresh.feats, bank.feats) and torch.equal(fresh.xyz, bank.xyz)
    model.register(fresh, [0], [1])


def test_register_range_trip_reruns_in_fp32x3_on_the_same_bank():
    """tests/test_gpu_range.py's overflowing FFN (an activation of ~1e5 in cross-encoder layer 2): encode_clouds does not trip (the FFN is
    not its business), register does, counts the fallback and returns the fp32x3 arithmetic's result on the SAME bank -- bit for bit what
    a compute_dtype 'fp32x3' model registers from those cached rows, and within 1e-4 of that model's forward."""
    from regtr_amd import CloudBank
    from regtr_amd.cloud_bank import model_stamp
    g = gold('modelnet_demo')
    cfg = load_cfg('modelnet')
    sd = seeded_sd(cfg)
    big = dict(sd)
    big['transformer_encoder.layers.2.linear1.weight'] = sd['transformer_encoder.layers.2.linear1.weight'] * 1.0e5
    big['transformer_encoder.layers.2.linear1.bias'] = sd['transformer_encoder.layers.2.linear1.bias'] * 1.0e5
    big['transformer_encoder.layers.2.linear2.weight'] = sd['transformer_encoder.layers.2.linear2.weight'] / 1.0e5
    m = _model(cfg, big)
    clouds = _dev([g['src'], g['tgt']])
    bank = m.encode_clouds(clouds)
    assert m.f16_range_fallbacks == 0
    out = m.register(bank, [0], [1])
    assert m.f16_range_fallbacks == 1, 'the overflow was not detected'
    assert torch.isfinite(out['pose']).all() and torch.isfinite(out['src_kp_warped'][0]).all()
    cfg3 = load_cfg('modelnet')
    cfg3.update({'compute_dtype': 'fp32x3'})
    m3 = _model(cfg3, big)
    same_rows = CloudBank(bank.xyz, bank.feats, bank.pe, bank.seg_off, bank.lens, model_stamp(m3))
    _assert_dicts_equal(out, m3.register(same_rows, [0], [1]))
    ref = m3({'src_xyz': clouds[:1], 'tgt_xyz': clouds[1:]})
    assert (out['pose'] - ref['pose']).abs().max() < 1e-4 and (out['src_kp_warped'][0] - ref['src_kp_warped'][0]).abs().max() < 1e-4


# ------------------------------------------------------------------------------------------------ 6. the harness
class _PlainPairs:
    """The pairs of a SyntheticScenePairs as a plain pair source (what run_test reads)."""

    def __init__(self, scene_pairs):
        self.sp = scene_pairs

    def __len__(self):
        return len(self.sp)

    def __getitem__(self, i):
        return self.sp[i]


@pytest.fixture(scope='module')
def harness_case():
    from regtr_amd import harness
    cfg = load_cfg('3dmatch')
    model = _model(cfg)
    sp = harness.SyntheticScenePairs(2, 4, 6, points=3000)
    dev = torch.device('cuda', torch.cuda.current_device())
    poses, ids, _ = harness.run_test(model, _PlainPairs(sp), 3, dev)
    return model, sp, dev, poses, ids


@pytest.mark.parametrize('cap', [1024, 5])
def test_run_test_shared_equals_run_test(harness_case, cap, tmp_path):
    from regtr_amd import harness
    model, sp, dev, poses, ids = harness_case
    assert len(sp) == 12
    p2, i2, timing = harness.run_test_shared(model, sp, 3, dev, max_bank_clouds=cap)
    assert i2.tolist() == ids.tolist() == list(range(12))
    assert np.abs(p2 - poses).max() < 1e-5
    assert timing['distinct_fragments'] == 8 and timing['pair_slots'] == 24
    if cap >= 8:
        assert timing['clouds_encoded'] == 8
    else:
        assert timing['clouds_encoded'] > 8
    recs = []
    for pose, i in zip(p2, i2):
        sk, tk = sp.fragment_keys(int(i))
        recs.append({'src_path': sk, 'tgt_path': tk, 'pose': pose})
    harness.write_est_log(str(tmp_path), '3DMatch', recs)
    n_blocks = 0
    for scene in os.listdir(tmp_path / '3DMatch'):
        lines = open(tmp_path / '3DMatch' / scene / 'est.log').read().strip().split('\n')
        assert len(lines) % 5 == 0
        for k in range(0, len(lines), 5):
            head = lines[k].split('\t')
            assert len(head) == 3 and int(head[2]) == -1
            T = np.array([[float(v) for v in lines[k + 1 + r].split('\t')] for r in range(4)])
            assert T.shape == (4, 4) and np.allclose(T[3], [0, 0, 0, 1])
            n_blocks += 1
    assert n_blocks == 12


def test_run_test_shared_refuses_replicas_and_losses(harness_case):
    from regtr_amd import harness
    model, sp, dev, _, _ = harness_case
    with pytest.raises(NotImplementedError):
        harness.run_test_shared([model, model], sp, 5, dev)
    with pytest.raises(NotImplementedError):
        harness.run_test_shared(model, sp, 5, dev, losses=True)
    with pytest.raises(ValueError, match='at least 5'):
        harness.run_test_shared(model, sp, 3, dev, max_bank_clouds=4)
