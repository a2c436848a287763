"""GPU: TransformerCrossEncoderLayer / TransformerCrossEncoder.forward in EVERY configuration -- normalize_before x sa_val_has_pos_emb x
ca_val_has_pos_emb under a positional embedding, both norm orders without one, with and without the final norm and
return_intermediate -- against the float64 restatement tests/cross_encoder_fwd_ref.py, which tests/test_cross_encoder_variants_host.py
pins to the real reference module and shows to tell any two configurations apart (the closest pair differs by 0.15 of max |ref|, the
bar here is 1e-4).  No backbone: the encoder is built directly.

Bar (tests/test_gpu_cross_encoder_grads.py's): max err <= 1e-4 max |ref| per output tensor; a STACK output beyond that is held to 4x the
error of the restatement itself run in float32 torch on the same GPU.  Arithmetic: gemm_planes 3 with attn_precision 3 under the f16
pair context (compute_dtype 'fp32', the default) and with attn_precision 0 outside it ('fp32x3').  The flags only choose which float32
arrays feed which launches, so the plain-bf16 kinds add nothing here.

Per variant also: which path ran (the one C call iff pre-norm and (no pe or both value flags)), the C call bit-identical to the
op-by-op path, the pairs of a batch independent of each other; on the split-value paths a parameter update reaches the cached bias
halves and weight row blocks, and two runs are bit-identical."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import cross_encoder_fwd_ref as R

pytestmark = pytest.mark.gpu

FLAT = 1e-4
INDEP = 1e-5
# name -> (gemm_planes, attn_precision, f16 pair context)
ARITH = {'fp32': (3, 3, True), 'fp32x3': (3, 0, False)}
WIDE = ['pre-sa0-ca0-full', 'post-sa1-ca0-full', 'pre-nope-full', 'post-nope-full']
SPLIT = ['pre-sa0-ca0-full', 'pre-sa1-ca0-plain', 'post-sa0-ca1-full', 'post-sa0-ca0-plain']       # a value projection without the pe


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device='cuda', dtype=dtype)


def _flat(got, ref):
    ref = ref.double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


@functools.lru_cache(None)
def _case(name):
    return R.draw_case(name)


@functools.lru_cache(None)
def _ref(case, vname, layers=None):
    """The float64 yardstick, computed once per (case, variant) and shared by the tests; never modified."""
    return R.run_variant(_case(case), vname, layers=layers)


def _sd_of(c, vname, sd=None):
    final = R.stack_form(*R.VARIANTS[vname])[0]
    return {k: v for k, v in (c['sd'] if sd is None else sd).items() if final or not k.startswith('norm.')}


def _build(c, vname, arith, sd=None):
    from regtr_amd.transformer import TransformerCrossEncoder, TransformerCrossEncoderLayer
    (pre, sa, ca, _), mode = R.VARIANTS[vname]
    final, ri = R.stack_form(*R.VARIANTS[vname])
    layer = TransformerCrossEncoderLayer(c['D'], c['H'], c['F'], 0.0, 'relu', pre, sa, ca)
    layer.gemm_planes, layer.attn_precision = ARITH[arith][:2]
    enc = TransformerCrossEncoder(layer, c['L'], torch.nn.LayerNorm(c['D']) if final else None, return_intermediate=ri)
    enc.load_state_dict(_sd_of(c, vname, sd), strict=True)
    return enc.cuda()


def _args(c, vname):
    with_pe = R.VARIANTS[vname][0][3]
    return (_dev(c['x']), _dev(c['pe']) if with_pe else None, _dev(c['seg'], torch.int32), _dev(c['kv_self'], torch.int32),
            _dev(c['kv_cross'], torch.int32), c['max_len'])


def _eligible(vname):
    """The one C call serves pre-norm layers whose values read what the queries read: no pe at all, or both value flags."""
    pre, sa, ca, with_pe = R.VARIANTS[vname][0]
    return pre and (not with_pe or (sa and ca))


@contextlib.contextmanager
def _one_call(on, calls):
    """ops.use_one_call_cross_encoder = on, every _forward_one_call counted; both restored on the way out."""
    from regtr_amd import ops
    from regtr_amd.transformer import TransformerCrossEncoder
    saved, orig = ops.use_one_call_cross_encoder, TransformerCrossEncoder._forward_one_call
    TransformerCrossEncoder._forward_one_call = lambda self, *a: (calls.append(1), orig(self, *a))[1]
    ops.use_one_call_cross_encoder = on
    try:
        yield
    finally:
        ops.use_one_call_cross_encoder = saved
        TransformerCrossEncoder._forward_one_call = orig


def _forward(enc, c, vname, arith, one_call=True, calls=None):
    from regtr_amd import ops
    with _one_call(one_call, [] if calls is None else calls), ops.f16_pair(ARITH[arith][2]), torch.no_grad():
        return enc(*_args(c, vname))


def _held_to_the_bar(tag, got, c, vname, ref, sd=None):
    """max err <= 1e-4 max |ref|, else (a stack output) 4x the float32 torch evaluation's own error.  -> the measured error."""
    e = _flat(got, ref)
    bar, note = FLAT, ''
    if e > FLAT:
        bar = 4 * _flat(R.run_variant(c, vname, dtype=torch.float32, device='cuda', sd=sd), ref)
        note = f' (float32 torch: {bar / 4:.2e})'
    print(f'{tag}: {e:.2e}{note}')
    assert e <= bar, (tag, e, bar)
    return e


def _check_variant(case, vname, arith):
    from regtr_amd import _lib
    c = _case(case)
    ref = _ref(case, vname)
    enc = _build(c, vname, arith)
    n = len(c['x'])
    assert _lib.lib().regtr_cross_encoder_supported(n, c['D'], c['F'], c['H']), 'the shape must leave the choice of path to the flags'
    calls = []
    out = _forward(enc, c, vname, arith, calls=calls)
    assert tuple(out.shape) == tuple(ref.shape) and torch.isfinite(out).all()
    assert calls == ([1] if _eligible(vname) else []), f'{vname}: wrong path ({len(calls)} C calls)'
    _held_to_the_bar(f'{case} {vname} {arith} stack', out, c, vname, ref)
    # the op-by-op path: the same launches, so the same bits where the C call ran; and it must not be taken with the switch off
    calls = []
    by_op = _forward(enc, c, vname, arith, one_call=False, calls=calls)
    assert calls == [] and torch.equal(out, by_op), f'{vname}: the C call and the op-by-op path differ'
    # one layer alone against float64 (no fallback: that is the stack's)
    from regtr_amd import ops
    with ops.f16_pair(ARITH[arith][2]), torch.no_grad():
        one = enc.layers[0](*_args(c, vname))
    e = _flat(one, _ref(case, vname, 1))
    print(f'{case} {vname} {arith} layer: {e:.2e}')
    assert e <= FLAT, (vname, e)
    return enc, out


def _check_pairs_alone(case, vname, arith, out):
    """Every pair of the batch run alone gives the batch's rows: a wrong kv_cross or segment offset mixes clouds."""
    c = _case(case)
    scale = float(_ref(case, vname).abs().max())
    for b in range(len(c['src'])):
        p = R.pair_of(c, b)
        alone = _forward(_build(p, vname, arith), p, vname, arith)
        d = float((out[:, p['rows'].cuda()] - alone).abs().max()) / scale
        print(f'{case} {vname} {arith} pair {b} alone vs in the batch: {d:.2e}')
        assert d <= INDEP, (vname, b, d)


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize('arith', list(ARITH))
@pytest.mark.parametrize('vname', list(R.VARIANTS))
@pytest.mark.parametrize('case', ['ragged', 'ragged_empty'])
def test_every_variant_against_float64_two_pairs(case, vname, arith):
    """D 64, two pairs, a one-token cloud and one a row past a 128-row tile; 'ragged_empty': the second pair's target is empty (its
    partner's cross-attention rows are zero, the empty cloud has no rows at all)."""
    _, out = _check_variant(case, vname, arith)
    _check_pairs_alone(case, vname, arith, out)


@pytest.mark.parametrize('arith', list(ARITH))
@pytest.mark.parametrize('vname', WIDE)
def test_shipped_widths_against_float64(vname, arith):
    """D 256, F 1024, 410 + 339 tokens: where the f16 pair plan, the N = 2D / N = D split GEMMs at ldc = 3D and the strip kernels are
    the ones chosen."""
    _check_variant('wide', vname, arith)


# ------------------------------------------------------------------------------------------------ the split-value paths' caches
def _new_in_proj(c, seed):
    """The case's parameters with both attentions' in-projections of every layer redrawn."""
    gen = torch.Generator().manual_seed(seed)
    sd = dict(c['sd'])
    for k in sd:
        if 'in_proj_weight' in k:
            sd[k] = torch.randn(sd[k].shape, generator=gen) * sd[k].shape[1] ** -0.5
        elif 'in_proj_bias' in k:
            sd[k] = 0.1 * torch.randn(sd[k].shape, generator=gen)
    return sd


@pytest.mark.parametrize('arith', list(ARITH))
@pytest.mark.parametrize('case,vname', [('ragged', v) for v in SPLIT] + [('wide', SPLIT[0]), ('wide', SPLIT[2])])
def test_parameter_update_reaches_the_split_caches(case, vname, arith):
    """in_proj_weight / in_proj_bias overwritten in place, as load_state_dict and an optimiser step do: the next forward is that of the
    new parameters.  A stale bias half or weight row block leaves the first result (or a mixture) instead."""
    c = _case(case)
    enc = _build(c, vname, arith)
    first = _forward(enc, c, vname, arith)
    sd = _new_in_proj(c, 9)
    with torch.no_grad():
        for layer, pre in ((l, f'layers.{i}.') for i, l in enumerate(enc.layers)):
            for attn, name in ((layer.self_attn, 'self_attn'), (layer.multihead_attn, 'multihead_attn')):
                attn.in_proj_weight.copy_(sd[pre + name + '.in_proj_weight'])
                attn.in_proj_bias.copy_(sd[pre + name + '.in_proj_bias'])
    second = _forward(enc, c, vname, arith)
    ref = R.run_variant(c, vname, sd=sd)
    _held_to_the_bar(f'{case} {vname} {arith} after the update', second, c, vname, ref, sd=sd)
    moved = _flat(first, ref)
    assert moved >= 100 * FLAT, f'the redrawn parameters must move the result well past the bar (moved {moved:.2e})'
    assert not torch.equal(first, second)
    assert torch.equal(second, _forward(_build(c, vname, arith, sd=sd), c, vname, arith)), 'an updated encoder != one built from the new parameters'


@pytest.mark.parametrize('arith', list(ARITH))
@pytest.mark.parametrize('case,vname', [('ragged', SPLIT[0]), ('ragged', SPLIT[2]), ('wide', SPLIT[0]), ('wide', 'post-sa1-ca0-full')])
def test_split_value_variants_are_bit_reproducible(case, vname, arith):
    c = _case(case)
    enc = _build(c, vname, arith)
    a = _forward(enc, c, vname, arith)
    b = _forward(enc, c, vname, arith)
    assert torch.equal(a, b) and torch.equal(a, _forward(_build(c, vname, arith), c, vname, arith))
