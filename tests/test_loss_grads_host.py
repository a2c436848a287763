"""CPU: the training-loss drop-ins (regtr_amd/losses.py) -- state_dict layout equal to the reference modules' (recorded in the
loss_grads goldens), the refusal paths, and the goldens' self-consistency: the float64 restatement of tests/loss_grads_ref.py reproduces
the REAL reference's autograd values (tools/make_golden_loss_grads.py)."""
import numpy as np
import pytest
import torch

from tests import loss_grads_ref as R
from tests.util import gold

CASES = ['3dmatch_crop_b2', '3dmatch_kitchen', 'modelnet_630']


def _inputs(g):
    lg = gold(f'losses_{g["case"]}')
    B = int(g['n_pairs'])
    src_kp = [lg[f'src_kp_{b}'] for b in range(B)]
    tgt_kp = [lg[f'tgt_kp_{b}'] for b in range(B)]
    warped = [lg[f'src_kp_warped_{b}'] for b in range(B)]
    src, tgt, W, w = R.draw_inputs([len(x) for x in src_kp], [len(x) for x in tgt_kp], int(g['D']), int(g['feat_seed']))
    return lg, src_kp, tgt_kp, warped, [x.numpy() for x in src], [x.numpy() for x in tgt], W.numpy(), [x.numpy() for x in w]


@pytest.mark.parametrize('case', CASES)
def test_state_dict_matches_reference_modules(case):
    from regtr_amd.losses import CorrCriterion, InfoNCELossFull
    g = gold(f'loss_grads_{case}')
    m = InfoNCELossFull(int(g['D']), float(g['r_p']), float(g['r_n']))
    sd = m.state_dict()
    assert list(sd.keys()) == list(g['sd_infonce_keys'])
    assert [list(v.shape) for v in sd.values()] == g['sd_infonce_shapes'].tolist()
    assert m.n_sample == 256 and m.W.requires_grad
    assert list(CorrCriterion('mae').state_dict().keys()) == list(g['sd_corr_keys'])
    # the reference's init: N(0, 0.1)
    big = InfoNCELossFull(256, 0.2, 0.4)
    assert 0.09 < float(big.W.detach().std()) < 0.11 and abs(float(big.W.detach().mean())) < 0.01


def test_refusals():
    from regtr_amd.losses import CorrCriterion, InfoNCELossFull
    with pytest.raises(NotImplementedError, match='mse'):
        CorrCriterion(metric='mse')
    c = CorrCriterion()
    kp = [torch.zeros(4, 3)]
    pose = torch.eye(4)[:3].unsqueeze(0)
    with pytest.raises(NotImplementedError, match='overlap_weights=None'):
        c(kp, kp, pose)
    with pytest.raises(RuntimeError, match='GPU'):
        c(kp, [torch.zeros(4, 3, requires_grad=True)], pose, [torch.ones(4)])
    with pytest.raises(RuntimeError, match='take no gradient'):
        c(kp, kp, pose, [torch.ones(4, requires_grad=True)])
    with pytest.raises(RuntimeError, match='take no gradient'):
        c(kp, kp, pose.clone().requires_grad_(), [torch.ones(4)])
    m = InfoNCELossFull(64, 0.2, 0.4)
    f = [torch.zeros(5, 64)]
    with pytest.raises(RuntimeError, match='GPU'):
        m(f, f, [torch.zeros(5, 3)], [torch.zeros(5, 3)])
    with pytest.raises(RuntimeError, match='take no gradient'):
        m(f, f, [torch.zeros(5, 3, requires_grad=True)], [torch.zeros(5, 3)])
    with pytest.raises(RuntimeError, match='same number'):
        m(f, f + f, [torch.zeros(5, 3)], [torch.zeros(5, 3)])


@pytest.mark.parametrize('case', CASES)
def test_golden_self_consistency(case):
    g = gold(f'loss_grads_{case}')
    B = int(g['n_pairs'])
    lg, src_kp, tgt_kp, warped, src, tgt, W, w = _inputs(g)
    r_p, r_n = float(g['r_p']), float(g['r_n'])
    # the stored anchors are the float32 GT transform of the loss golden's key points
    for b in range(B):
        assert np.array_equal(g[f'anc_xyz_{b}'], R.transform_f32(lg['pose'][b], src_kp[b]))
    dec = [R.decisions(g[f'anc_xyz_{b}'], tgt_kp[b], r_p, r_n) for b in range(B)]
    loss, dA, dG, dW = R.infonce_grads(src, tgt, W, dec)
    assert abs(loss - float(g['loss_feat'])) <= 1e-9 * abs(loss)
    for b in range(B):
        for got, ref in ((dA[b], g[f'dA_{b}']), (dG[b], g[f'dG_{b}'])):
            assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max() + 1e-12
    assert np.abs(dW - g['dW']).max() <= 1e-6 * np.abs(g['dW']).max()
    assert np.all(np.tril(g['dW'], -1) == 0)                    # triu(W) only
    lc, dwp = R.corr_grads(src_kp, warped, lg['pose'], w)
    assert abs(lc - float(g['loss_corr'])) <= 1e-6 * abs(lc)
    for b in range(B):
        assert np.abs(dwp[b] - g[f'dwarped_{b}']).max() <= 1e-6 * np.abs(dwp[b]).max()
    assert int(g['decision_rows']) == 0
    assert sum(m.sum() for _, m, _ in dec) > 0
