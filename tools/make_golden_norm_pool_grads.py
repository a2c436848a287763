"""Generates tests/golden/norm_pool_grads_<case>.npz by running the REAL reference code forward + backward in float64 on the CPU:
kpconv_blocks.max_pool (models/backbone_kpconv/kpconv_blocks.py:127-143) and BatchNormBlock with nn.InstanceNorm1d followed by
nn.LeakyReLU(0.1), with the bottleneck's shortcut sum for two cases (:489,510-519,556-561,741).  Runs where the reference tree is
available, never on a GPU machine.
Re-run:  python tools/make_golden_norm_pool_grads.py

The cases and their seeded inputs are tests/norm_pool_grads_ref.py's (CASES with `golden`, draw_case): seeds and shapes are stored,
inputs are not.  The loss is sum(out * dy).

Stored (float64): every STEP-th row of `out`, `dx` (and `dres` with a shortcut), seeds and shapes.  InstanceNorm cases also store
`skip` (rows of out, C) bool: True where the (cloud, channel) column holds an element whose float64 |z| -- the LeakyReLU's argument --
is below Z_TOL(element), so small that a float32 forward may put it on the other side of 0.  That changes g for the element and,
through the two means, the gradient of its whole column, so the column is left out of a float32 comparison.  At most 0.1 % of a
case's elements may be so marked (asserted here: pick another seed otherwise).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                  # noqa: E402
from tests import norm_pool_grads_ref as R                     # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
STEP = 3                                                        # rows of out / dx / dres that are stored
MAX_SKIP = 1e-3


def z_tol(xh, mean_rstd, rh=None, rmean_rrstd=None):
    """32 float32 roundings of everything that is added up in z: far above the float32 forward's error (R.C_XH + 1 of them)."""
    t = 1 + np.abs(xh) + mean_rstd
    if rh is not None:
        t = t + np.abs(rh) + (0 if rmean_rrstd is None else rmean_rrstd)
    return 32 * R.U * t


def run_in(name):
    ref = ref_loader.load()
    c = R.draw_case(name)
    lrelu, shortcut = c['golden']
    C, lens = c['C'], c['lens']
    t = lambda a: torch.from_numpy(a).double()
    x, res = t(c['x']).requires_grad_(), t(c['res']).requires_grad_()
    stack = torch.tensor(lens, dtype=torch.long)
    z = ref.kpconv_blocks.BatchNormBlock(C, True, 0.02).double()(x, stack)
    if shortcut == 'plain':
        z = z + res
    elif shortcut == 'normed':
        z = z + ref.kpconv_blocks.BatchNormBlock(C, True, 0.02).double()(res, stack)
    out = torch.nn.LeakyReLU(0.1)(z) if lrelu else z
    (out * t(c['dy'])).sum().backward()
    # columns with an element too close to 0
    skip = np.zeros(z.shape, bool)
    zn, o = z.detach().numpy(), 0
    for n in lens:
        sl = slice(o, o + n)
        o += n

        def parts(v):
            v = v.astype(np.float64)
            m = v.mean(0)
            rs = 1.0 / np.sqrt(v.var(0) + R.EPS)
            return (v - m) * rs, np.abs(m) * rs
        xh, ms = parts(c['x'][sl])
        rh, rms = (None, None) if shortcut == 'none' else (parts(c['res'][sl]) if shortcut == 'normed' else (c['res'][sl].astype(np.float64), None))
        near = np.abs(zn[sl]) <= z_tol(xh, ms, rh, rms)
        skip[sl] = near.any(0)[None, :] & lrelu
    frac = float(skip.mean())
    assert frac <= MAX_SKIP, f'{name}: {frac:.2%} of the elements sit in a column with a LeakyReLU argument within rounding of 0; pick another seed'
    g = {'case': np.array(name), 'seed': np.int64(c['seed']), 'C': np.int64(C), 'lens': np.array(lens, dtype=np.int64),
         'lrelu': np.bool_(lrelu), 'shortcut': np.array(shortcut), 'step': np.int64(STEP), 'out': out.detach()[::STEP].numpy(),
         'dx': x.grad[::STEP].numpy(), 'skip': skip[::STEP]}
    if shortcut != 'none':
        g['dres'] = res.grad[::STEP].numpy()
    return g, f'{frac:.3%} skipped'


def run_pool(name):
    ref = ref_loader.load()
    c = R.draw_case(name)
    x = torch.from_numpy(c['x']).double().requires_grad_()
    inds = torch.from_numpy(c['nbr'][:, :c['width']].astype(np.int64))
    assert int(inds.min()) >= 0 and int(inds.max()) <= c['Ns']      # the reference's gather takes no other shadow than Ns
    out = ref.kpconv_blocks.max_pool(x, inds)
    (out * torch.from_numpy(c['dy']).double()).sum().backward()
    g = {'case': np.array(name), 'seed': np.int64(c['seed']), 'C': np.int64(c['C']), 'Ns': np.int64(c['Ns']), 'Nq': np.int64(c['Nq']),
         'ld': np.int64(c['ld']), 'width': np.int64(c['width']), 'step': np.int64(STEP), 'out': out.detach()[::STEP].numpy(),
         'dx': x.grad[::STEP].numpy()}
    return g, ''


def main():
    for name in R.GOLDEN_CASES:
        g, note = (run_in if R.CASES[name]['kind'] == 'in' else run_pool)(name)
        path = os.path.join(GOLD, f'norm_pool_grads_{name}.npz')
        np.savez_compressed(path, **g)
        print(name, g['out'].shape, f'{os.path.getsize(path) / 1024:.0f} KB', note)


if __name__ == '__main__':
    main()
