"""Builds regtr_amd/libregtr_hip.so and libregtr_parity.so (gfx950) in-tree with hipcc.  `python -m regtr_amd.build [--force] [--dispatch]`.
--dispatch additionally builds libregtr_hip.dispatch.so (tests only: build_dispatch)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libregtr_hip.so')
# the parity-mode neighbour search (include/regtr_hip_parity.h): nanoflann's KD-tree order + std::sort replayed on the GPU -- a checking mode's
# library of its own, so that the product library holds no nanoflann-derived code (THIRD_PARTY_NOTICES.md)
PARITY_LIB = os.path.join(HERE, 'libregtr_parity.so')
PARITY_SOURCES = ['ref_order.hip']
# development only: REGTR_VARIANT=name REGTR_VARIANT_FLAGS='-DX=1' builds libregtr_hip.name.so for A/B kernel experiments
VARIANT = os.environ.get('REGTR_VARIANT', '')
VARIANT_FLAGS = os.environ.get('REGTR_VARIANT_FLAGS', '').split()
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = 'gfx950'
SOURCES = ['preprocess.hip', 'kpconv.hip', 'kpconv_bwd.hip', 'gemm.hip', 'gemm_x3.hip', 'gemm_stream.hip', 'block_tail.hip', 'norm.hip', 'posemb_mlp.hip', 'norm_pool_bwd.hip', 'attention.hip', 'attention_bwd.hip', 'layer_bwd.hip', 'head_bwd.hip', 'cross_encoder.hip', 'encoder.hip', 'procrustes.hip', 'losses.hip', 'circle_loss.hip', 'augment.hip', 'augment_modelnet.hip', 'metrics.hip', 'optim.hip', 'cloud_bank.hip', 'grad_bucket.hip', 'icp.hip', 'icp_plane.hip']
# bit-level parity of the float32 distance / voxel arithmetic with the reference's SSE2 build needs no contraction
# kpconv.hip: SLP-packed f32 VALU (v_pk_*) beside MFMAs costs more than it saves and blocks v_add_f32_dpp fusion
EXTRA = {'preprocess.hip': ['-ffp-contract=off'], 'losses.hip': ['-ffp-contract=off'], 'circle_loss.hip': ['-ffp-contract=off'], 'augment.hip': ['-ffp-contract=off'], 'augment_modelnet.hip': ['-ffp-contract=off'], 'metrics.hip': ['-ffp-contract=off'], 'optim.hip': ['-ffp-contract=off'], 'grad_bucket.hip': ['-ffp-contract=off'], 'icp.hip': ['-ffp-contract=off'], 'icp_plane.hip': ['-ffp-contract=off'], 'ref_order.hip': ['-ffp-contract=off'], 'kpconv.hip': ['-fno-slp-vectorize']}
COMMON = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result',
          '-I' + os.path.join(os.path.dirname(HERE), 'include')]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def source_hash():
    """sha256 over the kernel sources and headers (sorted by name): the code version of libregtr_hip.so.  profiles/pmc_traffic.json is
    stamped with it and bench.py reports the counter traffic only when it matches the sources the loaded library was built from."""
    import hashlib
    h = hashlib.sha256()
    inc = os.path.join(os.path.dirname(HERE), 'include')
    files = sorted([os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.hip', '.h'))]
                   + [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith('.h')])
    for f in files:
        h.update(os.path.basename(f).encode() + b'\0')
        h.update(open(f, 'rb').read())
    return h.hexdigest()


def write_build_info():
    """regtr_amd/_build_info.json next to the library: source hash + git commit (the GPU boxes receive a snapshot without .git)."""
    import json
    info = {'source_sha256': source_hash(), 'git_commit': None, 'git_dirty': None}
    try:
        root = os.path.dirname(HERE)
        info['git_commit'] = subprocess.check_output(['git', '-C', root, 'rev-parse', 'HEAD'], stderr=subprocess.DEVNULL, text=True).strip()
        info['git_dirty'] = bool(subprocess.check_output(['git', '-C', root, 'status', '--porcelain', '--', 'regtr_amd', 'include'],
                                                         stderr=subprocess.DEVNULL, text=True).strip())
    except (OSError, subprocess.CalledProcessError):
        pass
    with open(os.path.join(HERE, '_build_info.json'), 'w') as f:
        json.dump(info, f, indent=1)
    return info


def _compile_and_link(lib, sources, objdir, flags, force, verbose):
    """Compiles the stale ones of `sources` (in parallel) into objdir and links `lib` if an object changed or the library is missing."""
    os.makedirs(objdir, exist_ok=True)
    inc = os.path.join(os.path.dirname(HERE), 'include')
    headers = ([os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
               + [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith('.h')])      # the public C-ABI header is a dependency too

    def run(cmd):
        if verbose:
            print(' '.join(cmd))
        subprocess.check_call(cmd)

    def compile_one(src):
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        if force or _stale(o, [s] + headers):
            run([HIPCC] + COMMON + EXTRA.get(src, []) + flags + ['-c', s, '-o', o])
            return o, True
        return o, False

    with ThreadPoolExecutor(max_workers=len(sources)) as ex:
        res = list(ex.map(compile_one, sources))
    if force or any(ch for _, ch in res) or not os.path.exists(lib):
        run([HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', lib] + [o for o, _ in res])
    return lib


def build(force=False, verbose=False, variant=None, variant_flags=None):
    """variant / variant_flags default to REGTR_VARIANT / REGTR_VARIANT_FLAGS (development builds next to the product library).  The product
    build (no variant) builds libregtr_parity.so as well."""
    variant = VARIANT if variant is None else variant
    flags = VARIANT_FLAGS if variant_flags is None else list(variant_flags)
    if variant:
        return _compile_and_link(os.path.join(HERE, f'libregtr_hip.{variant}.so'), SOURCES, os.path.join(HERE, 'build', variant), flags, force, verbose)
    _compile_and_link(LIB, SOURCES, os.path.join(HERE, 'build'), flags, force, verbose)
    build_parity(force, verbose)
    if os.path.isdir(os.path.join(os.path.dirname(HERE), '.git')):
        write_build_info()
    return LIB


def build_parity(force=False, verbose=False):
    """libregtr_parity.so from csrc/ref_order.hip (regtr_amd/_lib.py: parity_lib; loaded only when parity mode asks for KD-tree tables)."""
    return _compile_and_link(PARITY_LIB, PARITY_SOURCES, os.path.join(HERE, 'build', 'parity'), [], force, verbose)


def build_dispatch(force=False, verbose=False):
    """libregtr_hip.dispatch.so (tests only): the product sources with the tile planner's development switches read from the environment
    (-DREGTR_DEV_ENV=1) and eight-wave attention from the first workgroup on (-DMHA_WIDE_MIN_WG=1), so tests/test_gpu_dispatch.py can force
    every launch branch at small shapes (REGTR_DEV=1 REGTR_VARIANT=dispatch)."""
    return build(force, verbose, variant='dispatch', variant_flags=['-DREGTR_DEV_ENV=1', '-DMHA_WIDE_MIN_WG=1'])


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))      # (the parity library with it)
    if '--dispatch' in sys.argv:
        print(build_dispatch(force='--force' in sys.argv, verbose=True))
