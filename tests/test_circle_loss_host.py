"""CircleLossFull without a GPU: the float64 closed form of tests/circle_loss_ref.py against the REAL reference module's float64
autograd (tests/golden/circle_loss_*.npz, tools/make_golden_circle_loss.py), a finite-difference check of its gradient, the NaN rule,
the model's constructor under `feature_loss_type: circle`, and the entry points' argument refusals (nothing is launched)."""
import numpy as np
import pytest
import torch

from tests import circle_loss_ref as R
from tests.util import gold, load_cfg

CASES = ['3dmatch_crop_b2', '3dmatch_kitchen', 'modelnet_630']


def golden_inputs(case):
    """(golden, per-pair [(src feat, tgt feat, anchor xyz, tgt xyz)]) with the features drawn from the stored seed."""
    g = gold(f'circle_loss_{case}')
    lg = gold(f'losses_{case}')
    gg = gold(f'loss_grads_{case}')
    B = int(g['n_pairs'])
    tgt_kp = [lg[f'tgt_kp_{b}'] for b in range(B)]
    anc = [gg[f'anc_xyz_{b}'] for b in range(B)]
    src, tgt = R.draw_features([len(x) for x in anc], [len(x) for x in tgt_kp], int(g['D']), int(g['feat_seed']), anc, tgt_kp)
    return g, [(src[b].numpy(), tgt[b].numpy(), anc[b], tgt_kp[b]) for b in range(B)]


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_reference_golden(case):
    """Both sides are float64 runs of the same formula: this pins the closed form, the exp(0) terms of the masked entries included."""
    g, pairs = golden_inputs(case)
    r_p, r_n = float(g['r_p']), float(g['r_n'])
    msk = [R.masks(p[2], p[3], r_p, r_n) for p in pairs]
    loss, per, dA, dG, cnt = R.circle([p[0] for p in pairs], [p[1] for p in pairs], msk)
    assert int(g['decision_pairs_f32']) == 0
    assert abs(loss - float(g['loss'])) <= 1e-9 * abs(float(g['loss'])), (loss, float(g['loss']))
    assert np.allclose(per, g['pair_loss'], rtol=1e-9, atol=0)
    assert [c[0] for c in cnt] == list(g['n_rows']) and [c[1] for c in cnt] == list(g['n_cols'])
    assert min(min(c) for c in cnt) >= 11 and int(g['pos_active']) > 100 and int(g['neg_active']) > 10000     # both halves carry gradient
    for b in range(len(pairs)):
        for got, ref in ((dA[b], g[f'dA_{b}']), (dG[b], g[f'dG_{b}'])):
            # 1e-9 of the tensor's maximum, plus what storing the golden as float32 did to each element (half an ulp: 2^-24 |ref|)
            ref = ref.astype(np.float64)
            assert np.all(np.abs(got - ref) <= 1e-9 * np.abs(ref).max() + 2.0 ** -24 * np.abs(ref)), b
            assert np.abs(ref).max() > 0


def _small_pair(rng, n=5, m=4, D=8):
    a = rng.normal(0, 0.35, (n, D))
    b = rng.normal(0, 0.35, (m, D))
    b[0] = a[0] + 1e-3                                        # a positive below pos_margin: zero weight
    pos = np.zeros((n, m), bool)
    neg = np.zeros((n, m), bool)
    pos[np.arange(n), np.arange(n) % m] = True
    neg[np.arange(n), (np.arange(n) + 2) % m] = True
    neg[1, 0] = True
    return a, b, pos, neg


def test_restatement_gradient_by_finite_differences():
    """The weights max(.) are constants of the differentiation: the finite difference holds them at their values."""
    rng = np.random.default_rng(3)
    a, b, pos, neg = _small_pair(rng)
    p = dict(R.DEFAULTS)
    s = p['log_scale']

    def value(a, b, wp, wn):
        d = np.sqrt(((a[:, None] - b[None]) ** 2).sum(-1) + 1e-12)
        tp, tn = s * (d - p['pos_margin']) * wp, s * (p['neg_margin'] - d) * wn
        lse = lambda t, ax: np.log(np.exp(t).sum(ax))
        row = R._softplus(lse(tp, 1) + lse(tn, 1)) / s               # (torch's: x itself above 20)
        col = R._softplus(lse(tp, 0) + lse(tn, 0)) / s
        sr, sc = pos.any(1) & neg.any(1), pos.any(0) & neg.any(0)
        return (row[sr].mean() + col[sc].mean()) / 2
    d0 = np.sqrt(((a[:, None] - b[None]) ** 2).sum(-1) + 1e-12)
    wp = np.where(pos, np.maximum(d0 - p['pos_optimal'], 0), 0.0)
    wn = np.where(neg, np.maximum(p['neg_optimal'] - d0, 0), 0.0)
    assert (wp[pos] == 0).any() and (wp > 0).any() and (wn > 0).any()
    loss, _, dA, dG, cnt = R.circle([a], [b], [(pos, neg)])
    assert abs(loss - value(a, b, wp, wn)) <= 1e-12 * abs(loss) and min(cnt[0]) > 0
    h = 1e-6
    for x, grad, which in ((a, dA[0], 0), (b, dG[0], 1)):
        num = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            args_p = (xp, b) if which == 0 else (a, xp)
            args_m = (xm, b) if which == 0 else (a, xm)
            num[idx] = (value(*args_p, wp, wn) - value(*args_m, wp, wn)) / (2 * h)
        assert np.abs(num - grad).max() <= 1e-7 * max(np.abs(grad).max(), 1e-3), which


def test_nan_pair_has_zero_gradient():
    rng = np.random.default_rng(4)
    a, b, pos, neg = _small_pair(rng)
    none = np.zeros_like(pos)
    for msk in ((none, neg), (pos, none)):                    # nothing inside r_p; nothing beyond r_n
        loss, per, dA, dG, cnt = R.circle([a, a], [b, b], [(pos, neg), msk])
        assert np.isnan(loss) and np.isfinite(per[0]) and np.isnan(per[1]) and cnt[1] == (0, 0)
        assert np.all(dA[1] == 0) and np.all(dG[1] == 0) and np.abs(dA[0]).max() > 0
    # rows selected, no column: the pos of a row and its neg lie in different columns, and no column holds both
    pos1 = np.zeros((1, 4), bool)
    neg1 = np.zeros((1, 4), bool)
    pos1[0, 0] = neg1[0, 2] = True
    loss, per, dA, dG, cnt = R.circle([a[:1]], [b], [(pos1, neg1)])
    assert np.isnan(loss) and cnt[0] == (1, 0) and np.all(dA[0] == 0) and np.all(dG[0] == 0)


def test_model_constructor_under_circle():
    from regtr_amd import RegTR
    from regtr_amd.losses import CircleLossFull
    cfg = dict(load_cfg('3dmatch'))
    cfg['feature_loss_type'] = 'circle'
    m = RegTR(cfg)
    assert isinstance(m.feature_criterion, CircleLossFull) and m.feature_criterion is m.feature_criterion_un
    assert m.feature_criterion.dist_type == 'euclidean' and (m.feature_criterion.r_p, m.feature_criterion.r_n) == (cfg['r_p'], cfg['r_n'])
    assert not [k for k in m.state_dict() if k.startswith('feature_criterion')]
    ref = RegTR(load_cfg('3dmatch'))
    assert 'feature_criterion.W' in ref.state_dict() and 'feature_criterion_un.W' in ref.state_dict()      # InfoNCE: unchanged
    assert [k for k in ref.state_dict() if not k.startswith('feature_criterion')] == list(m.state_dict())
    c = CircleLossFull()
    assert (c.dist_type, c.log_scale, c.r_p, c.r_n, c.pos_margin, c.neg_margin, c.pos_optimal, c.neg_optimal) == \
        ('cosine', 10, 0.125, 0.25, 0.1, 1.4, 0.1, 1.4)
    assert len(c.state_dict()) == 0 and not list(c.parameters())
    assert all(p is not None for p in m.trainable_parameters())        # no W to touch


def test_unknown_feature_loss_type_still_raises():
    from regtr_amd import RegTR
    cfg = dict(load_cfg('3dmatch'))
    cfg['feature_loss_type'] = 'triplet'
    with pytest.raises(NotImplementedError, match='triplet'):
        RegTR(cfg)


def test_criterion_refusals_on_the_host():
    from regtr_amd.losses import CircleLossFull
    f, x = [torch.zeros(3, 64)], [torch.zeros(3, 3)]
    with pytest.raises(NotImplementedError, match='cosine'):
        CircleLossFull()(f, f, x, x)
    c = CircleLossFull('euclidean')
    with pytest.raises(RuntimeError, match='GPU'):
        c(f, f, x, x)                                         # tensors off the GPU
    with pytest.raises(RuntimeError, match='gradient'):
        c(f, f, [torch.zeros(3, 3, requires_grad=True)], x)
    with pytest.raises(RuntimeError):
        c([], [], [], [])


FAKE = 0x10000          # never dereferenced: every call below is refused before a launch


def circle_call(bwd=False, D=256, n_pairs=1, n_anc=4, n_pos=4, max_anc=4, max_pos=4, anc=FAKE, pos=FAKE, axyz=FAKE, pxyz=FAKE, aoff=FAKE,
                poff=FAKE, out=FAKE, alse=FAKE, asel=FAKE, plse=FAKE, psel=FAKE, lda=None, ldp=None, scale=10.0, grad=FAKE, mean_div=1.0,
                danc=FAKE, dpos=FAKE, ldda=None, lddp=None):
    from regtr_amd import _lib as L
    head = (anc, lda or D, pos, ldp or D, axyz, pxyz, aoff, poff, n_pairs, n_anc, n_pos, max_anc, max_pos, D, 0.2, 0.4, scale, 0.1, 0.1,
            1.4, 1.4, None)
    if bwd:
        return L.lib().regtr_circle_bwd(*head, alse, asel, plse, psel, out, grad, mean_div, danc, ldda or D, dpos, lddp or D, None)
    return L.lib().regtr_circle_rows(*head, out, alse, asel, plse, psel, None)


BAD = [{'D': 0}, {'D': 32}, {'D': 100}, {'D': 576}, {'D': -64}, {'n_pairs': -1}, {'n_anc': -1}, {'n_pos': -3}, {'max_anc': -1},
       {'max_pos': -1}, {'anc': None}, {'pos': None}, {'axyz': None}, {'pxyz': None}, {'aoff': None}, {'poff': None}, {'out': None},
       {'alse': None}, {'asel': None}, {'plse': None}, {'psel': None}, {'lda': 255}, {'ldp': 192}, {'lda': 258}, {'anc': FAKE + 4},
       {'pos': FAKE + 8}, {'scale': 0.0}]


@pytest.mark.parametrize('bwd', [False, True])
def test_entry_points_refuse_bad_arguments(bwd):
    for kw in BAD:
        assert circle_call(bwd, **kw) == -2, kw
    if bwd:
        for kw in ({'mean_div': 0.0}, {'mean_div': -1.0}, {'grad': None}, {'danc': None}, {'dpos': None}, {'ldda': 128}, {'lddp': 258},
                   {'danc': FAKE + 4}):
            assert circle_call(True, **kw) == -2, kw
    assert circle_call(bwd, n_pairs=0, n_anc=0, n_pos=0, max_anc=0, max_pos=0, anc=None, pos=None, axyz=None, pxyz=None, aoff=None,
                       poff=None, out=None, alse=None, asel=None, plse=None, psel=None, grad=None, danc=None, dpos=None) == 0
