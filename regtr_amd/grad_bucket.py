"""GradBucket: the gradients of one optimiser step in ONE flat float32 device tensor -- the accumulator of gradient accumulation and the
payload of data-parallel training's single all-reduce (csrc/grad_bucket.hip packs; regtr_amd.distributed.all_reduce_sum reduces).

    bucket = GradBucket(list(model.named_parameters()), n_extra=len(loss_keys))
    for every micro-batch of the step:   backward();  bucket.add(1 / (k * world), stacked_losses);  gradients back to None
    bucket.all_reduce();  bucket.attach();  optimizer.step()

A run with (k, W) and a run with (k W, 1) average the same micro-batches.  Bit for bit the two agree only where the additions are the
same: accumulation computes fmaf(s, g1, fl(s g0)), the rank sum fl(s g0) + fl(s g1), which are one number where s g is exact (k W a
power of two, no underflow) and may differ in the last bit otherwise.  The mean is over micro-batches of each micro-batch's own loss (torch
DDP's rule), not a re-weighting by pair count.

Without skip_nonfinite a non-finite gradient on one rank reaches every rank.  With GradBucket(..., skip_nonfinite=True) every add() first
forms a device flag from the micro-batch's GRADIENTS alone (one more read of them: grad_sumsq and a guarded finish; a NaN loss with finite
gradients does not count) and packs under it: a micro-batch whose gradient norm is not finite contributes nothing -- neither to the
segments nor to the `extra` tail -- and the flag is counted into one private tail slot, n_good, which rides the same all-reduce
unscaled, so every rank sees the same count.  attach(n_expected, optimizer) hands the optimiser grad_scale = n_expected / n_good on the
device: exactly 1.0 when nothing was excluded (the unguarded path's bits), the mean over the good micro-batches otherwise, and
non-finite when there is none, which makes FusedAdamW(skip_nonfinite=True) skip the step.  No host read anywhere."""
import torch

from . import ops
from .distributed import all_reduce_sum


class GradBucket:
    """GradBucket(params, n_extra=0).  params: the parameters in the optimiser's order, tensors or (name, tensor) pairs (the names only
    serve error messages).  The LAYOUT is fixed at the first add() from the parameters that then hold a gradient, in `params` order: every
    segment starts on a multiple of 4 floats (its length rounded up to 4), and a tail of n_extra floats follows the last segment -- the
    stacked loss scalars ride the same collective as one more row of the same table.  Parameters without a gradient (a frozen backbone,
    kernel_points) are simply not in the layout, as FusedAdamW skips them.  The flat tensor is zeroed once, when it is allocated, and
    its padding is never written afterwards.  skip_nonfinite=True (the module docstring): one more tail float after the n_extra ones
    holds n_good; `skipped_micro_batches` is then a float32 device scalar, the cumulative n_expected - n_good over the attach() calls
    (over all ranks: it is formed after the all-reduce)."""

    def __init__(self, params, n_extra=0, skip_nonfinite=False):
        params = list(params)
        self.names = [p[0] if isinstance(p, (tuple, list)) else None for p in params]
        self.params = [p[1] if isinstance(p, (tuple, list)) else p for p in params]
        self.n_extra = int(n_extra)
        if self.n_extra < 0:
            raise ValueError('GradBucket: n_extra must not be negative')
        self.flat = None              # (n_total,) float32, on the parameters' device
        self.index = None             # positions in `params` of the parameters in the layout
        self.offsets = None           # their first elements in `flat`; one more entry: the tail's
        self.sizes = None
        self._filled = False          # the current optimiser step has had its first add()
        self.skip_nonfinite = bool(skip_nonfinite)
        self._flag = None             # skip_nonfinite: the scratch guard word of the per-micro-batch flag, (4,) int32
        self._scale = None            # ... the (1,) float32 grad_scale attach() computes
        self.skipped_micro_batches = None
        self._n_expected = None       # ... (value, its (1,) device tensor)

    def _name(self, i):
        return self.names[i] if self.names[i] is not None else f'params[{i}] {tuple(self.params[i].shape)}'

    @staticmethod
    def layout(sizes, n_extra=0):
        """(offsets of the segments and of the tail, total length) for segment lengths `sizes`: plain host arithmetic."""
        offsets, o = [], 0
        for n in sizes:
            offsets.append(o)
            o += (int(n) + 3) // 4 * 4
        offsets.append(o)
        return offsets, o + int(n_extra)

    def _fix_layout(self, held):
        if not held:
            raise RuntimeError('GradBucket.add: no parameter holds a gradient (call it after backward())')
        self.index = held
        self.sizes = [self.params[i].numel() for i in held]
        self.offsets, total = self.layout(self.sizes, self.n_extra + (1 if self.skip_nonfinite else 0))
        dev = self.params[held[0]].device
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        if self.skip_nonfinite:
            self._flag = ops.new_guard(dev)
            self._scale = torch.ones(1, dtype=torch.float32, device=dev)
            self.skipped_micro_batches = torch.zeros((), dtype=torch.float32, device=dev)

    def add(self, scale, extra=None):
        """One grad_pack over the current p.grad's (and `extra`, n_extra float32 values on the device, into the tail): the first call of
        an optimiser step assigns scale * g, later ones accumulate fmaf(scale, g, bucket).  extra None: zeros on the first call, nothing
        afterwards.  Raises RuntimeError when the set of gradient-holding parameters differs from the layout's, naming the first one."""
        held = [i for i, p in enumerate(self.params) if p.grad is not None]
        if self.index is None:
            self._fix_layout(held)
        elif held != self.index:
            a, b = set(self.index), set(held)
            i = min(a ^ b)
            raise RuntimeError(f'GradBucket.add: the set of parameters with a gradient changed: {self._name(i)} '
                               f'{"lost its" if i in a else "now has a"} gradient (the layout is fixed at the first add)')
        grads = [self.params[i].grad for i in held]
        sizes = self.sizes
        if self.n_extra:
            if extra is not None and (extra.numel() != self.n_extra or extra.dtype is not torch.float32):
                raise RuntimeError(f'GradBucket.add: extra must hold {self.n_extra} float32 values, got {tuple(extra.shape)} {extra.dtype}')
            grads = grads + [None if extra is None else extra.detach().reshape(-1)]
            sizes = sizes + [self.n_extra]
        elif extra is not None:
            raise RuntimeError('GradBucket.add: extra given but n_extra = 0')
        if self.skip_nonfinite:
            with ops._lib.on_device(self.flat.device):
                ops.grad_finite_flag(grads[:len(held)], self._flag)           # the gradients only: not `extra`
            ops.grad_pack(grads, self.offsets[:len(grads)], self.flat, scale, self._filled, sizes=sizes, flag=self._flag, n_good=self.n_good())
        else:
            ops.grad_pack(grads, self.offsets[:len(grads)], self.flat, scale, self._filled, sizes=sizes)
        self._filled = True

    def all_reduce(self):
        """ONE all_reduce(SUM) of the whole flat tensor when a process group is initialised (at world size 1 too); else nothing."""
        all_reduce_sum(self.flat)

    def views(self):
        """The parameters' views of the bucket, in layout order, each of its parameter's shape."""
        return [self.flat[o:o + n].view(self.params[i].shape) for i, o, n in zip(self.index, self.offsets, self.sizes)]

    def attach(self, n_expected=None, optimizer=None):
        """p.grad = the parameter's view of the bucket, and the step is over: the next add() assigns.  FusedAdamW.step() then runs
        unchanged on the averaged gradient (its last_grad_norm is the averaged gradient's norm; clipping acts after averaging, as
        clip_grad_norm_ after DDP).  The views stay valid until that next add().
        skip_nonfinite: n_expected = the micro-batches of the step over all ranks (k W, what the scales of add() divided by); -> the
        (1,) float32 device tensor grad_scale = n_expected / n_good, also set as optimizer.grad_scale when an optimiser is given."""
        for i, v in zip(self.index, self.views()):
            self.params[i].grad = v
        self._filled = False
        if not self.skip_nonfinite:
            return None
        if n_expected is None:
            raise RuntimeError('GradBucket.attach: a skip_nonfinite bucket needs n_expected (the micro-batches of the step over all ranks)')
        n_good = self.n_good()
        if self._n_expected is None or float(n_expected) != self._n_expected[0]:
            self._n_expected = (float(n_expected), torch.full((1,), float(n_expected), dtype=torch.float32, device=self.flat.device))
        torch.div(self._n_expected[1], n_good, out=self._scale)               # n_good == 0: inf, and the optimiser skips the step
        self.skipped_micro_batches += self._n_expected[1][0] - n_good[0]
        if optimizer is not None:
            optimizer.grad_scale = self._scale
        return self._scale

    def n_good(self):
        """skip_nonfinite: the (1,) view of the tail slot that counts the micro-batches the bucket holds (after all_reduce: of all ranks)."""
        o = self.offsets[-1] + self.n_extra
        return self.flat[o:o + 1]

    def reset(self):
        """Abandons the current optimiser step: what was added so far is dropped, the next add() assigns."""
        self._filled = False

    def extra(self):
        """The tail (n_extra floats) as a view."""
        o = self.offsets[-1]
        return self.flat[o:o + self.n_extra]
