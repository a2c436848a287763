"""CPU: the learned positional embedding (pos_emb_type: learned) -- construction, the reference's state_dict keys, the float64
restatement of tests/posemb_mlp_ref.py against the reference module's recorded output, that its float32 bound bites, the seeded cases'
ReLU margin, and the optimiser's parameter order.  Goldens: tools/make_golden_learned_posemb.py."""
import numpy as np
import pytest
import torch

from tests import posemb_mlp_ref as PR
from tests.util import gold, load_cfg, seeded_sd

CASES = [('modelnet_demo', 'modelnet'), ('3dmatch_crop_b2', '3dmatch')]


def _learned(cfgn):
    from regtr_amd import RegTR
    cfg = load_cfg(cfgn)
    cfg.update({'pos_emb_type': 'learned'})
    return cfg, RegTR(cfg)


@pytest.mark.parametrize('case,cfgn', CASES)
def test_learned_config_constructs_with_the_reference_keys(case, cfgn):
    cfg, m = _learned(cfgn)
    g = gold(f'learned_posemb_{case}')
    assert list(m.state_dict().keys()) == [str(k) for k in g['sd_keys']]
    sd = PR.learned_state_dict(seeded_sd(cfg), cfg.d_embed, int(g['mlp_seed']))
    assert list(sd) == list(m.state_dict().keys())
    m.load_state_dict(sd, strict=True)                               # a checkpoint with the reference's keys loads strictly
    mlp = m.pos_embed.mlp
    assert [type(x).__name__ for x in mlp] == ['Linear', 'ReLU'] * 4 + ['Linear']
    for k, s in PR.shapes(cfg.d_embed).items():
        assert tuple(m.pos_embed.state_dict()[k].shape) == s, k


def test_unknown_type_and_other_dimensions_are_refused():
    from regtr_amd import RegTR
    from regtr_amd.regtr import PositionEmbeddingLearned
    cfg = load_cfg('3dmatch')
    cfg.update({'pos_emb_type': 'fourier'})
    with pytest.raises(NotImplementedError, match='fourier'):
        RegTR(cfg)
    with pytest.raises(NotImplementedError):
        PositionEmbeddingLearned(2, 256)
    with pytest.raises(RuntimeError):
        PositionEmbeddingLearned(3, 64)(torch.zeros(4, 3))           # a CPU tensor: no CPU path
    with pytest.raises(RuntimeError):
        PositionEmbeddingLearned(3, 64).forward_grad(torch.zeros(4, 3))


def test_default_initialisation_is_nn_linears():
    """The module draws what the reference's draws: nn.Linear's default initialisation, in the reference's order."""
    from regtr_amd.regtr import PositionEmbeddingLearned
    torch.manual_seed(5)
    a = PositionEmbeddingLearned(3, 128).state_dict()
    torch.manual_seed(5)
    b = torch.nn.Sequential(torch.nn.Linear(3, 32), torch.nn.ReLU(), torch.nn.Linear(32, 64), torch.nn.ReLU(), torch.nn.Linear(64, 128),
                            torch.nn.ReLU(), torch.nn.Linear(128, 256), torch.nn.ReLU(), torch.nn.Linear(256, 128)).state_dict()
    assert list(a) == ['mlp.' + k for k in b] and all(torch.equal(a['mlp.' + k], v) for k, v in b.items())


@pytest.mark.parametrize('case,cfgn', CASES)
def test_restatement_reproduces_the_reference_module(case, cfgn):
    g = gold(f'learned_posemb_{case}')
    sd = PR.draw_mlp(int(g['d_model']), int(g['mlp_seed']))
    r = PR.forward(sd, g['points_last'])
    got, want = r['pe'][::int(g['pe_step'])], g['pe_rows']
    assert got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f'{case}: restatement vs the reference module (float64): {err:.1e}; max |pe| {np.abs(want).max():.2f}')
    assert err <= 1e-12


@pytest.mark.parametrize('case,cfgn', CASES)
def test_the_bound_bites(case, cfgn):
    """On the golden's key points: a float32 numpy evaluation stays inside the bound; the same MLP on operands rounded to bf16, and to one
    f16 plane, does not (pe and the four activations, as the GPU test checks them)."""
    g = gold(f'learned_posemb_{case}')
    sd = PR.draw_mlp(int(g['d_model']), int(g['mlp_seed']))
    xyz = g['points_last']
    r = PR.forward(sd, xyz)
    ratio = lambda e, b: float((e / np.maximum(b, 1e-300)).max())
    f32 = ratio(np.abs(PR.forward_f32(sd, xyz).astype(np.float64) - r['pe']), r['b_pe'])
    print(f'{case}: float32 numpy worst err / bound {f32:.3f}')
    assert f32 <= 1.0
    for name, q in (('bf16', PR.round_bf16), ('one f16 plane', PR.round_f16)):
        rq = PR.forward(sd, xyz, quant=q)
        pe, acts = ratio(np.abs(rq['pe'] - r['pe']), r['b_pe']), ratio(np.abs(rq['acts'] - r['acts']), r['b_acts'])
        print(f'{case}: {name} operands worst err / bound: pe {pe:.2f}, activations {acts:.1f}')
        assert max(pe, acts) > 1.0


def test_relu_margins():
    """The seeded cases keep every ReLU pre-activation RELU_MARGIN away from 0 (tests/head_grads_ref.py: relu_margin), and the MLP takes
    the same ReLU sides in float32 as in float64 there."""
    g = gold(f'head_grads_learned_{PR.STACK_CASE}')
    assert int(g['seed']) == PR.STACK_SEED >= PR.STACK_NOMINAL_SEED and float(g['relu_margin']) >= PR.RELU_MARGIN
    c = PR.draw_stack_case()
    xyz = c['xyz'].numpy()
    m = PR.relu_margin(c['sd_pos'], xyz)
    print(f'stack case seed {PR.STACK_SEED}: stored margin {float(g["relu_margin"]):.2e}, the MLP alone {m:.2e}')
    assert m >= float(g['relu_margin']) >= PR.RELU_MARGIN
    for seed in range(PR.STACK_NOMINAL_SEED, PR.STACK_SEED):           # the seeds passed over did not keep the margin
        assert PR.stack_relu_margin(PR.draw_stack_case(seed)) < PR.RELU_MARGIN
    _, hs = PR.torch_fwd(c['sd_pos'], c['xyz'].float())
    r = PR.forward(c['sd_pos'], xyz)
    assert all(np.array_equal(hs[l].numpy() > 0, r['h'][l] > 0) for l in range(4))


def test_written_out_backward_is_autograds():
    sd = PR.draw_mlp(64, 3)
    gen = torch.Generator().manual_seed(1)
    xyz, dpe = torch.randn((37, 3), generator=gen).double(), torch.randn((37, 64), generator=gen).double()
    P = {k: v.double().requires_grad_() for k, v in sd.items()}
    pe, hs = PR.torch_fwd(P, xyz)
    (pe * dpe).sum().backward()
    got = PR.backward(sd, xyz.numpy(), [h.detach().numpy() for h in hs], dpe.numpy())
    alt = PR.torch_bwd(sd, xyz, [h.detach() for h in hs], dpe)
    for k in PR.KEYS:
        assert np.abs(got[k] - P[k].grad.numpy()).max() <= 1e-12 * np.abs(got[k]).max(), k
        assert np.abs(alt[k].numpy() - got[k]).max() <= 1e-12 * np.abs(got[k]).max(), k


def test_trainable_parameters_and_optimizer_order():
    cfg, m = _learned('3dmatch')
    ten = [p for _, p in m.pos_embed.named_parameters()]
    assert len(ten) == 10
    tp = m.trainable_parameters()
    assert all(any(p is q for q in tp) for p in ten)
    names = [n for n, _ in m.named_parameters()]
    i0 = names.index('pos_embed.mlp.0.weight')
    assert names[i0 - 1] == 'feat_proj.bias' and names[i0 + 10].startswith('transformer_encoder.') and \
        names[i0:i0 + 10] == ['pos_embed.' + k for k in PR.KEYS]
    g = gold('learned_posemb_3dmatch_crop_b2')
    ref_params = [str(k) for k in g['sd_keys']]                      # (the reference model has no buffers: its state_dict is its parameters)
    assert names == ref_params
    # the sine model's list is the learned one's without the ten
    sine = [n for n, _ in __import__('regtr_amd').RegTR(load_cfg('3dmatch')).named_parameters()]
    assert sine == [n for n in names if not n.startswith('pos_embed.')]
    # the optimiser is built over list(model.parameters()): the ten sit at the reference's indices (FusedAdamW needs a GPU to step, not to be built)
    opt, _ = m.configure_optimizers()
    flat = [p for grp in opt.param_groups for p in grp['params']]
    assert len(flat) == len(names) and all(flat[i0 + j] is ten[j] for j in range(10))
