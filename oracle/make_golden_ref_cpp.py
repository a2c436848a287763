"""TEST INFRASTRUCTURE ONLY -- records tests/golden/ref_cpp_outputs.json: the sha256 of every output of the unmodified reference C++
(oracle/_ref) that the test suite consumes, keyed by the sha256 of its inputs.  Where oracle/_ref cannot be built, oracle/native.py
answers those same calls by replay: the table recomputed by our restatement of the reference's order, accepted only when its
sha256 equals the recorded one.  Needs oracle/_ref (the reference tree); re-run after changing an input of such a test:

    python -m oracle.make_golden_ref_cpp

The CPU tests are run as they are (in-process pytest); the reference-C++ calls of the GPU tests are issued here on the same inputs
(tests/test_gpu_model.py, tests/test_gpu_stress.py)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import canonical, native, regtr_ref   # noqa: E402


def gpu_test_calls():
    from tests.test_gpu_stress import _pair
    from tests.util import gold, load_cfg
    # test_gpu_model.py: test_reference_order_meta_equals_reference_preprocessor
    for case, cfgn in (('3dmatch_crop', '3dmatch'), ('modelnet_demo', 'modelnet'), ('3dmatch_home_at', '3dmatch'), ('modelnet_630', 'modelnet')):
        g = gold(case)
        cfg = load_cfg(cfgn)
        cfg.update({'kpconv_ref_row_order': True})
        regtr_ref.preprocess([g['src'], g['tgt']], cfg, use_ref_cpp=True)
    # test_gpu_model.py: test_real_fragments_batch_reference_gpu_preprocessor_semantics_and_parity_mode (regtr_forward's preprocess)
    gs = [gold(n) for n in ('3dmatch_kitchen', '3dmatch_hotel', '3dmatch_home_at')]
    cfg = load_cfg('3dmatch')
    cfg.update({'kpconv_ref_row_order': True})
    regtr_ref.preprocess([np.asarray(g['src']) for g in gs] + [np.asarray(g['tgt']) for g in gs], cfg, use_ref_cpp=True)
    # test_gpu_stress.py: the 100k + 100k pair's canonical tables and its parity-mode level-0 / level-1 calls
    src, tgt = _pair()
    canonical.canonical_meta([src, tgt], load_cfg('3dmatch'), use_ref=True)
    pts = np.concatenate([src, tgt]); lens = np.array([len(src), len(tgt)], np.int32)
    sub, sl = native.ref_subsample_batch(pts, lens, 0.05)
    native.ref_batch_query(pts, pts, lens, lens, 0.0625)
    native.ref_batch_query(sub, pts, sl, lens, 0.0625)


def main():
    import pytest
    tests = [os.path.join(ROOT, 'tests', f) for f in ('test_oracle.py', 'test_ref_order.py')]
    with native.recording() as rec:
        rc = pytest.main(['-q', '-p', 'no:cacheprovider', '-m', 'not gpu'] + tests)
        if rc != 0:
            sys.exit(f'make_golden_ref_cpp: the CPU tests failed against the reference C++ (pytest exit {rc})')
        gpu_test_calls()
    with open(native.RECORDED, 'w') as f:         # one record per line
        f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(rec[k], sort_keys=True)}' for k in sorted(rec)) + '\n}\n')
    print(f'{len(rec)} reference-C++ outputs recorded in {os.path.relpath(native.RECORDED, ROOT)}')


if __name__ == '__main__':
    main()
