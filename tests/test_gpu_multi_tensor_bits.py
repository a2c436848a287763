"""GPU: the multi-tensor optimiser and bucket kernels (csrc/optim.hip, csrc/grad_bucket.hip over csrc/multi_tensor.h) write, bit for bit,
what the build that tests/golden/multi_tensor_bits.json was recorded from wrote (tools/record_multi_tensor_bits.py; the file names its
commit -- the one before the kernels were folded onto one body).  The calls and their inputs are tests/multi_tensor_bits_ref.py's:
grad_sumsq, both norm finishes, adam_step and adam_step_guarded in every variant, grad_pack assigning and accumulating with and without
a flag.  sha256 digests of the output bytes: no tolerance, no digest left out."""
import json
import os

import pytest

from tests import multi_tensor_bits_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'multi_tensor_bits.json')


def _gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def got():
    return R.digests()


def test_the_fixture_is_whole():
    gold = _gold()
    assert len(gold['commit']) == 40 and gold['seed'] == R.SEED
    names = set(gold['sha256'])
    for s, _, _ in R.SETS:
        assert {f'{s}/inputs', f'{s}/grad_sumsq', f'{s}/grad_norm_finish', f'{s}/grad_pack/nothing_to_pack'} <= names
        assert sum(k.startswith(f'{s}/grad_norm_finish_guarded/') for k in names) == 2
        assert sum(k.startswith(f'{s}/adam_step/') for k in names) == 4
        assert sum(k.startswith(f'{s}/adam_step_guarded/') for k in names) == 16
        assert sum(k.startswith(f'{s}/grad_pack/scale=') for k in names) == 10
    assert len(names) == 36 * len(R.SETS)


def test_same_calls_as_recorded(got):
    assert sorted(got) == sorted(_gold()['sha256'])


def test_inputs_are_the_recorded_ones(got):
    gold = _gold()['sha256']
    for s, _, _ in R.SETS:
        assert got[f'{s}/inputs'] == gold[f'{s}/inputs'], f'{s}: the seeded inputs differ from the recorded ones; nothing below can match'


def test_every_digest_matches(got):
    gold = _gold()['sha256']
    differ = [k for k in sorted(gold) if got.get(k) != gold[k]]
    assert not differ, f'{len(differ)} of {len(gold)} outputs differ in their bits from commit {_gold()["commit"][:12]}: {differ}'
