"""CPU: the checkers of tests/test_gpu_norm.py are sharp enough to catch a kernel that drops rows.

Statistics that omit one 128-row chunk of a cloud, or its last partial chunk, fail the InstanceNorm statistics bound; block-tail product
statistics that omit one 2048-row chunk fail the out_stats bound.  Exact float64 statistics rounded to float32 pass both."""
import numpy as np
import torch

from tests import test_gpu_norm as gn


def _x(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, C), generator=g) * (torch.rand(C, generator=g) * 3 + 0.1) + torch.rand(C, generator=g) * 4
    x[:, 0] = 2.5
    x[:, 1] = 1e3 + 1e-3 * torch.randn(n, generator=g)
    return x


def _f32(mean, var, lens):
    """float32 (mean, rstd) as the kernels report them: (0, 0) for an empty cloud."""
    st = torch.stack((mean, 1 / torch.sqrt(var + gn.EPS)), -1).float()
    st[torch.tensor(lens) == 0] = 0
    return st


def _f32_stats(x, lens):
    _, mean, var, _, _ = gn.moments64(x, lens)
    return _f32(mean, var, lens)


def test_instnorm_stats_bound_catches_a_missing_chunk():
    lens = [1000, 0, 300]
    x = _x(sum(lens), 16, 0)
    ref = gn.moments64(x, lens)
    assert gn.stats_ratio(_f32_stats(x, lens), *ref) <= 1
    for lo, hi in ((128, 256), (896, 1000)):              # one 128-row chunk; the last partial chunk (1000 = 7 x 128 + 104)
        keep = torch.ones(sum(lens), dtype=torch.bool)
        keep[lo:hi] = False
        got = _f32_stats(x[keep], [1000 - (hi - lo), 0, 300])
        r = gn.stats_ratio(got, *ref)
        assert r > 1, (lo, hi, r)


def test_out_stats_bound_catches_a_missing_chunk():
    lens = [6000, 0, 2100]
    M = sum(lens)
    g = torch.Generator().manual_seed(1)
    x = (torch.randn((M, 16), generator=g) * (torch.rand(16, generator=g) * 2 + 0.3) + 1.0).double()
    x[:, 3] = 50 + 1e-3 * x[:, 3]
    W = torch.randn((16, 64), generator=g) / 4
    m, mu, var = gn.prod_stats64(x, lens, W)
    bm, br = gn.moment_stats_bound(x, lens, W, gn.pivot_of(x, lens), m, mu, var, 2 * gn.U)
    exact = _f32(mu, var, lens)
    assert gn.out_stats_ratio(exact, lens, mu, var, bm, br) <= 1
    keep = torch.ones(M, dtype=torch.bool)
    keep[2048:4096] = False
    _, mu_d, var_d = gn.prod_stats64(x[keep], [6000 - 2048, 0, 2100], W)
    fake = _f32(mu_d, var_d, lens)
    assert gn.out_stats_ratio(fake, lens, mu, var, bm, br) > 1
    assert np.isfinite(bm.numpy()).all() and np.isfinite(br.numpy()).all()
