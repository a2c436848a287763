"""The calls whose output BITS tests/golden/multi_tensor_bits.json pins (tools/record_multi_tensor_bits.py records them from one build,
tests/test_gpu_multi_tensor_bits.py compares another's): every multi-tensor kernel of csrc/optim.hip and csrc/grad_bucket.hip through the
public regtr_amd.ops functions only, so that the same code runs against any commit that has them.

TENSOR SETS.  MIXED: tests/test_gpu_nonfinite_guard.py's -- lengths 1, 3, 4, 5, 4095, 4096, 4097, an empty tensor, a 6-element view that
starts one float off a 16-byte boundary, 8193.  MANY(n): n tensors of 1 .. 5 elements, n = 41 and 97 (they straddle 40 and 48 tensors
per launch, once and twice).  Every tensor is a view inside ONE sentinel-filled buffer per role, and what is digested is the whole buffer:
a write outside a tensor changes the digest too.  Inputs come from numpy's default_rng(SEED); the host scalars are formed with float64
multiplies, adds and square roots only (no pow), so they are the same numbers everywhere."""
import hashlib

import numpy as np
import torch

SEED = 20240917
SENT = 12345.0
MIXED = [1, 3, 4, 5, 4095, 4096, 4097, 0, 6, 8193]
MISALIGNED = 8
CLIP = 0.37
SCALES = (None, 0.5)


def many(n):
    return [1 + i % 5 for i in range(n)]


SETS = (('mixed', MIXED, MISALIGNED), ('many41', many(41), None), ('many97', many(97), None))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


class Flat:
    """One sentinel-filled float32 device buffer holding every tensor of a role: tensor i starts on a 16-byte boundary (one float past
    it for the misaligned one), four sentinels or more between neighbours."""

    def __init__(self, lens, mis):
        self.lens, self.starts = lens, []
        off = 4
        for i, n in enumerate(lens):
            self.starts.append(off + int(i == mis))
            off = (self.starts[-1] + n + 3) // 4 * 4 + 4
        self.total = off

    def fill(self, arrays):
        host = np.full(self.total, SENT, np.float32)
        for s, a in zip(self.starts, arrays):
            host[s:s + a.size] = a
        return torch.from_numpy(host).cuda()

    def views(self, buf, none_at=None):
        return [None if i == none_at else buf[s:s + n] for i, (s, n) in enumerate(zip(self.starts, self.lens))]


def _ipow(b, t):
    r = 1.0
    for _ in range(t):
        r *= b
    return r


def _one(x, dtype=torch.float32):
    return torch.tensor([x], dtype=dtype, device='cuda')


def digests():
    """{name: sha256 hex digest of the output bytes} over every recorded call."""
    from regtr_amd import ops
    out = {}
    for set_name, lens, mis in SETS:
        rng = np.random.default_rng(SEED)
        n = len(lens)
        lay = Flat(lens, mis)
        draw = lambda scale=1.0: [(rng.standard_normal(k) * scale).astype(np.float32) for k in lens]
        g_h, g2_h, p_h, m_h = draw(), draw(), draw(), draw(0.01)
        v_h = [(a.astype(np.float64) ** 2 * 1e-4).astype(np.float32) for a in draw()]
        g_buf, g2_buf = lay.fill(g_h), lay.fill(g2_h)
        grads = lay.views(g_buf)
        out[f'{set_name}/inputs'] = sha(g_buf, g2_buf, lay.fill(p_h), lay.fill(m_h), lay.fill(v_h))

        # ---- the norm
        partials = ops.grad_sumsq(grads)
        out[f'{set_name}/grad_sumsq'] = sha(partials)
        out[f'{set_name}/grad_norm_finish'] = sha(ops.grad_norm_finish(partials, CLIP), ops.grad_norm_finish(partials, 0.0))
        for gs in SCALES:
            guard = torch.tensor([0, 5, 7, 0], dtype=torch.int32, device='cuda')
            res = ops.grad_norm_finish_guarded(partials, CLIP, guard, None if gs is None else _one(gs))
            out[f'{set_name}/grad_norm_finish_guarded/scale={gs}'] = sha(res, guard)

        # ---- the steps
        hypers = [(1e-3 * (1 + i % 3), 1e-2, 0.9, 0.999, 1e-8) for i in range(n)]
        scalars = [h + (1.0 - _ipow(h[2], 3 + i % 2), float(np.sqrt(1.0 - _ipow(h[3], 3 + i % 2)))) for i, h in enumerate(hypers)]
        step_index = [(7 * i) % (n + 2) for i in range(n)]
        for dec in (True, False):
            for clip in (None, CLIP):
                coef = None if clip is None else _one(clip)
                bufs = [lay.fill(p_h), lay.fill(m_h), lay.fill(v_h)]
                ops.adam_step(lay.views(bufs[0]), grads, lay.views(bufs[1]), lay.views(bufs[2]), scalars, clip_coef=coef, decoupled=dec)
                out[f'{set_name}/adam_step/decoupled={dec}/clip={clip}'] = sha(*bufs)
                for gs in SCALES:
                    for ok in (1, 0):
                        bufs = [lay.fill(p_h), lay.fill(m_h), lay.fill(v_h)]
                        steps = torch.tensor([float(3 + j % 4 * 5) for j in range(n + 2)], dtype=torch.float32, device='cuda')
                        step_scalars = torch.full((2 * (n + 2),), SENT, dtype=torch.float32, device='cuda')
                        guard = torch.tensor([ok, 5, 7, 0], dtype=torch.int32, device='cuda')
                        ops.adam_step_guarded(lay.views(bufs[0]), grads, lay.views(bufs[1]), lay.views(bufs[2]), hypers, step_index, steps,
                                              guard, clip_coef=coef, grad_scale=None if gs is None else _one(gs), decoupled=dec,
                                              step_scalars=step_scalars)
                        out[f'{set_name}/adam_step_guarded/decoupled={dec}/clip={clip}/scale={gs}/guard={ok}'] = sha(*bufs, steps, step_scalars,
                                                                                                                   guard)

        # ---- the bucket: assign, then accumulate, one None gradient in each call; the segments in list order, 4-element aligned
        offsets, end = [], 0
        for k in lens:
            offsets.append(end)
            end = (end + k + 3) // 4 * 4
        first, second = lay.views(g_buf, none_at=1), lay.views(g2_buf, none_at=n - 2)
        for scale in (0.5, 1.0 / 3.0):
            for flags in (None, (1, 1), (0, 0), (1, 0), (0, 1)):
                bucket = torch.full((end + 8,), SENT, dtype=torch.float32, device='cuda')      # the tail: sentinels and n_good's slot
                bucket[:end] = 0.0
                kw = [{}, {}]
                if flags is not None:
                    kw = [dict(flag=torch.tensor([f, 5, 7, 0], dtype=torch.int32, device='cuda'), n_good=bucket[end + 4:end + 5]) for f in flags]
                ops.grad_pack(first, offsets, bucket, scale, False, sizes=lens, **kw[0])
                after_assign = sha(bucket)
                ops.grad_pack(second, offsets, bucket, scale, True, sizes=lens, **kw[1])
                out[f'{set_name}/grad_pack/scale={scale:.3f}/flags={flags}'] = hashlib.sha256((after_assign + sha(bucket)).encode()).hexdigest()
        # a guarded accumulate call with nothing to pack still counts its flag
        bucket = torch.full((end + 8,), SENT, dtype=torch.float32, device='cuda')
        ops.grad_pack([None] * n, offsets, bucket, 0.5, True, sizes=lens, flag=torch.tensor([1, 5, 7, 0], dtype=torch.int32, device='cuda'),
                      n_good=bucket[end + 4:end + 5])
        out[f'{set_name}/grad_pack/nothing_to_pack'] = sha(bucket)
    torch.cuda.synchronize()
    return out
