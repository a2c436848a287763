"""Generates tests/golden/kpconv_grads_<case>.npz by running the REAL reference KPConv (models/backbone_kpconv/kpconv_blocks.py:175-414,
rigid / linear / sum) forward + backward in float64 on the CPU.  Runs where the reference tree is available, never on a GPU machine.
Re-run:  python tools/make_golden_kpconv_grads.py

The cases, their seeded clouds, neighbour tables, weights, kernel points, features and upstream gradient are
tests/kpconv_grads_ref.py's (CASES / draw_case): seeds and shapes are stored, inputs are not (the kernel points are: 15 x 3).  The
module's `weights` and `kernel_points` are overwritten with the case's; the loss is sum(out * d_out).

Stored (float64): `out` (every `q_step`-th query row), `dx` (every `s_step`-th support row), `dw` for the input channels `w_chan`
(15, len(w_chan), Cout), the kernel points, the extent, seeds and shapes.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_loader                                  # noqa: E402
from tests import kpconv_grads_ref as R                        # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
STEP = 3                                                        # rows of out / dx that are stored


def w_chan(Cin):
    return sorted({0, 1 % Cin, Cin // 2, Cin - 1})


def run(name):
    ref = ref_loader.load()
    c = R.draw_case(name)
    with ref_loader.chdir(ref_loader.REF_SRC):                  # load_kernels opens the cwd-relative 'kernels/dispositions'
        conv = ref.kpconv_blocks.KPConv(R.KP, 3, c['Cin'], c['Cout'], c['extent'], c['radius'], fixed_kernel_points='center',
                                        KP_influence='linear', aggregation_mode='sum', deformable=False).double()
    with torch.no_grad():
        conv.weights.copy_(torch.from_numpy(c['weights']).double())
        conv.kernel_points.copy_(torch.from_numpy(c['kernel_points']).double())
    x = torch.from_numpy(c['x']).double().requires_grad_()
    out = conv(torch.from_numpy(c['q_pts']).double(), torch.from_numpy(c['s_pts']).double(), torch.from_numpy(c['nbr']).long(), x)
    (out * torch.from_numpy(c['d_out']).double()).sum().backward()
    ch = w_chan(c['Cin'])
    g = {'case': np.array(name), 'seed': np.int64(c['seed']), 'Cin': np.int64(c['Cin']), 'Cout': np.int64(c['Cout']),
         'Ns': np.int64(c['Ns']), 'Nq': np.int64(c['Nq']), 'H': np.int64(c['H']), 'extent': np.float64(c['extent']),
         'kernel_points': c['kernel_points'], 'q_step': np.int64(STEP), 's_step': np.int64(STEP), 'w_chan': np.array(ch, dtype=np.int64),
         'out': out.detach()[::STEP].numpy(), 'dx': x.grad[::STEP].numpy(), 'dw': conv.weights.grad[:, ch].numpy()}
    path = os.path.join(GOLD, f'kpconv_grads_{name}.npz')
    np.savez_compressed(path, **g)
    print(name, tuple(out.shape), f'{os.path.getsize(path) / 1024:.0f} KB')


def main():
    for name in R.CASES:
        run(name)


if __name__ == '__main__':
    main()
