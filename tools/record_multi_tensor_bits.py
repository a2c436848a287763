"""Records tests/golden/multi_tensor_bits.json: sha256 digests of what the multi-tensor optimiser and bucket kernels (csrc/optim.hip,
csrc/grad_bucket.hip) write, for the calls of tests/multi_tensor_bits_ref.py -- digests only, no tensors.  Needs an MI355X.
    python tools/record_multi_tensor_bits.py [--commit HASH] [--out tests/golden/multi_tensor_bits.json]
Run it from a build of the commit whose bits are to be kept: it uses the public regtr_amd.ops functions only, so it runs unchanged on
any commit that has them.  tests/test_gpu_multi_tensor_bits.py then holds every later build to those digests, with no tolerance.
--commit: the hash of the commit the loaded library was built from, stored in the file (default: regtr_amd/_build_info.json's)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import multi_tensor_bits_ref as R                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', type=str, default=None)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'tests', 'golden', 'multi_tensor_bits.json'))
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('tools/record_multi_tensor_bits.py needs an MI355X (HIP) device')
    commit = opt.commit
    if commit is None:
        with open(os.path.join(ROOT, 'regtr_amd', '_build_info.json')) as f:
            info = json.load(f)
        if info.get('git_dirty'):
            sys.exit('the library was built from a modified tree: name the commit with --commit')
        commit = info['git_commit']
    first, second = R.digests(), R.digests()
    if first != second:
        sys.exit('two runs of the same build disagree: ' + ', '.join(k for k in first if first[k] != second[k]))
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, 'w') as f:
        json.dump({'generated_by': 'tools/record_multi_tensor_bits.py', 'commit': commit, 'seed': R.SEED, 'sha256': first}, f, indent=1)
        f.write('\n')
    print(f'{len(first)} digests of commit {commit} -> {opt.out}')


if __name__ == '__main__':
    main()
