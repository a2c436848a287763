"""CPU: the host half of regtr_amd/csrc/multi_tensor.h -- the walk every multi-tensor entry point of csrc/optim.hip and
csrc/grad_bucket.hip goes through -- as a stand-alone program (tests/multi_tensor_host_main.cpp) built with the host compiler under
-fsanitize=address,undefined and run directly; nothing is loaded into Python.  Its `launch` only records and checks the chunks: at most
CAP entries and 2^31 - 1 workgroups each, wg0 the exclusive prefix, part0 the running total, the entries of a call the tensors that were
not skipped in order, and no entry without a workgroup ever found by a block -- for 0, 1, CAP - 1 .. 2 CAP + 1 tensors, empty tensors
skipped and kept, lengths around a slice, and the flush no launch on a device can reach: workgroup counts that sum past 2^31 - 1."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler (c++, g++, clang++) on the PATH'
    exe = str(tmp_path_factory.mktemp('multi_tensor') / 'multi_tensor_host_main')
    # a plain C++ compiler and no HIP header: the include path holds csrc/ alone
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', os.path.join(ROOT, 'regtr_amd', 'csrc'), os.path.join(ROOT, 'tests', 'multi_tensor_host_main.cpp'), '-o', exe],
                   check=True)
    return exe


# the three geometries in use: the norm (48 tensors, 8192 elements), the step and the pack (48, 4096), the guarded step (40, 4096)
@pytest.mark.parametrize('keep_empty', [0, 1], ids=['skipped', 'kept'])
@pytest.mark.parametrize('cap,slice_', [(48, 8192), (48, 4096), (40, 4096)])
def test_walk(program, cap, slice_, keep_empty):
    r = subprocess.run([program, str(cap), str(slice_), str(keep_empty)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, UBSAN_OPTIONS='print_stacktrace=1'))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith('chunks ok') and r.stdout.startswith('18 cases'), r.stdout + r.stderr
    assert r.stderr == ''


def test_host_half_needs_no_hip_header():
    src = open(os.path.join(ROOT, 'regtr_amd', 'csrc', 'multi_tensor.h')).read()
    assert '#include' not in src
