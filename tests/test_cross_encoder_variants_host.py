"""CPU: the yardstick of tests/test_gpu_cross_encoder_variants.py -- the forward restatement tests/cross_encoder_fwd_ref.py of every
cross-encoder configuration -- pinned to the stored float64 outputs of the REAL reference TransformerCrossEncoder
(tools/make_golden_cross_encoder_variants.py), and the proof that the GPU tests' inputs tell any two configurations apart."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

from tests import cross_encoder_fwd_ref as R
from tests.util import ROOT

GPU_BAR = 1e-4          # tests/test_gpu_cross_encoder_variants.py: max err <= 1e-4 max |ref|
APART = 100 * GPU_BAR   # two configurations must differ by at least this much of max |ref| on the GPU tests' inputs


@functools.lru_cache(None)
def _golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'cross_encoder_variants.npz'))


def test_golden_holds_every_variant_of_the_seeded_case():
    g, c = _golden(), R.CASES['golden']
    assert int(g['seed']) == c['seed'] and list(g['src_lens']) == c['src'] and list(g['tgt_lens']) == c['tgt']
    assert (int(g['D']), int(g['H']), int(g['F']), int(g['L'])) == (c['D'], c['H'], c['F'], c['L'])
    assert list(g['variants']) == list(R.VARIANTS) and len(R.VARIANTS) == 22
    # the matrix: all 8 flag combinations under a pe and both norm orders without one, each as 'full' and as 'plain'
    bases = {b for b, m in R.VARIANTS.values()}
    assert {b[:3] for b in bases if b[3]} == set(itertools.product((True, False), repeat=3))
    assert {b[0] for b in bases if not b[3]} == {True, False}
    assert all((b, m) in R.VARIANTS.values() for b in bases for m in R.MODES)
    # the stack forms: norm None with return_intermediate, the norm with and without it, neither
    forms = {R.stack_form(b, m) for b, m in R.VARIANTS.values()}
    assert forms == {(False, True), (True, True), (True, False), (False, False)}


@pytest.mark.parametrize('vname', list(R.VARIANTS))
def test_restatement_equals_the_real_reference_module(vname):
    """Validates the yardstick, not the product: both sides float64, the reference on padded clouds under key-padding masks."""
    c = R.draw_case('golden')
    want = _golden()['out/' + vname]
    got = R.run_variant(c, vname).numpy()
    assert got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f'{vname}: restatement vs the reference module {err:.2e}')
    assert err <= 1e-12


def test_single_layer_is_the_stacks_first_intermediate():
    c = R.draw_case('golden')
    for vname, (base, mode) in R.VARIANTS.items():
        if mode == 'full' and not base[0]:                      # post-norm 'full': raw layer outputs
            assert torch.equal(R.run_variant(c, vname, layers=1), R.run_variant(c, vname)[0])


def _distance(c, a, b, outs):
    """How far apart two variants' float64 outputs are, relative to max |ref|.  Outputs of the same shape: as they are.  (L, N, D)
    against (1, N, D): the last slices -- unless those are the same computation (one base with return_intermediate and without it, the
    final norm alike: post-norm 'full' / 'plain', pre-norm 'full' / 'last'), where the shape is the difference and what must be far
    apart is the two layers' outputs, so that returning the wrong one shows."""
    (ba, ma), (bb, mb) = R.VARIANTS[a], R.VARIANTS[b]
    ya, yb = outs[a], outs[b]
    if ya.shape != yb.shape:
        if ba == bb and R.stack_form(ba, ma)[0] == R.stack_form(bb, mb)[0]:
            full = ya if ya.shape[0] > 1 else yb
            ya, yb = full[0], full[-1]
        else:
            ya, yb = ya[-1], yb[-1]
    return float((ya - yb).abs().max() / max(ya.abs().max(), yb.abs().max()))


@pytest.mark.parametrize('case', ['ragged', 'ragged_empty', 'wide'])
def test_any_two_variants_are_far_apart_on_the_gpu_tests_inputs(case):
    """A wiring mistake turns one configuration into another (a swapped flag, a value that reads the wrong array, a norm too many);
    the GPU tests catch it only if the two differ by much more than their bar on the inputs they use."""
    c = R.draw_case(case)
    names = list(R.VARIANTS) if case != 'wide' else [n for n in R.VARIANTS if R.VARIANTS[n][1] == 'full']
    outs = {n: R.run_variant(c, n) for n in names}
    worst = min((_distance(c, a, b, outs), a, b) for a, b in itertools.combinations(names, 2))
    print(f'{case}: the closest pair of variants, {worst[1]} and {worst[2]}, differs by {worst[0]:.3f} of max |ref|')
    assert worst[0] >= APART, worst


def test_a_misaligned_positional_embedding_is_refused_on_every_path():
    """TransformerCrossEncoder._one_call_ok asks pe to be contiguous, not 16-byte aligned, although every reader takes float4s: the
    launches that read pe (regtr_layernorm's `add` on the pre-norm paths and inside the one C call, regtr_add_f32 on the post-norm
    path) refuse a misaligned base on the host, before anything is launched, so neither path can read it wrongly."""
    from regtr_amd import _lib
    L = _lib.lib()
    FAKE = 0x10000                                              # never dereferenced: refused before a launch
    for off in (4, 8, 12):
        assert L.regtr_layernorm(FAKE, 8, 64, FAKE, FAKE, 1e-5, FAKE + off, FAKE, None, None) == -2
        assert L.regtr_layernorm(FAKE, 8, 64, FAKE, FAKE, 1e-5, FAKE, FAKE, FAKE + off, None) == -2
        assert L.regtr_add_f32(FAKE, FAKE + off, 8 * 64, FAKE, None) == -2
        assert L.regtr_add_f32(FAKE + off, FAKE, 8 * 64, FAKE, None) == -2


def test_pairs_are_independent_and_the_empty_cloud_gives_zero_attention_rows():
    """The restatement's own batch independence (what the GPU test asks of the product), and the convention for an empty partner: the
    cross-attention contributes its out_proj bias alone."""
    c = R.draw_case('ragged_empty')
    for vname in ('pre-sa0-ca0-plain', 'post-sa1-ca0-full'):
        both = R.run_variant(c, vname)
        for b in range(2):
            p = R.pair_of(c, b)
            assert (both[:, p['rows']] - R.run_variant(p, vname)).abs().max() <= 1e-12 * both.abs().max()
    sd = {k: v.double() for k, v in c['sd'].items()}
    x = c['x'].double()
    one = R.layer_fwd(sd, 'layers.0.', x, c['pe'].double(), c['seg'], c['kv_self'], c['kv_cross'], c['H'], True, False, False)
    rows = slice(int(c['seg'][1]), int(c['seg'][2]))             # src_1, whose partner tgt_1 is empty
    sa = R._attn(sd, 'layers.0.', 'self_attn', 'norm1', x, c['pe'].double(), c['seg'], c['kv_self'], c['H'], True, False)
    ca = sa + sd['layers.0.multihead_attn.out_proj.bias']
    n3 = R.ln_fwd(ca, sd['layers.0.norm3.weight'], sd['layers.0.norm3.bias'])[0]
    want = ca + torch.relu(n3 @ sd['layers.0.linear1.weight'].T + sd['layers.0.linear1.bias']) @ sd['layers.0.linear2.weight'].T + sd['layers.0.linear2.bias']
    assert torch.allclose(one[rows], want[rows], rtol=0, atol=1e-12)
