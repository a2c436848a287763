"""GradBucket: the gradients of one optimiser step in ONE flat float32 device tensor -- the accumulator of gradient accumulation and the
payload of data-parallel training's single all-reduce (csrc/grad_bucket.hip packs; regtr_amd.distributed.all_reduce_sum reduces).

    bucket = GradBucket(list(model.named_parameters()), n_extra=len(loss_keys))
    for every micro-batch of the step:   backward();  bucket.add(1 / (k * world), stacked_losses);  gradients back to None
    bucket.all_reduce();  bucket.attach();  optimizer.step()

A run with (k, W) and a run with (k W, 1) average the same micro-batches.  Bit for bit the two agree only where the additions are the
same: accumulation computes fmaf(s, g1, fl(s g0)), the rank sum fl(s g0) + fl(s g1), which are one number where s g is exact (k W a
power of two, no underflow) and may differ in the last bit otherwise.  The mean is over micro-batches of each micro-batch's own loss (torch
DDP's rule), not a re-weighting by pair count.  There is no skip logic: a non-finite gradient on one rank reaches every rank."""
import torch

from . import ops
from .distributed import all_reduce_sum


class GradBucket:
    """GradBucket(params, n_extra=0).  params: the parameters in the optimiser's order, tensors or (name, tensor) pairs (the names only
    serve error messages).  The LAYOUT is fixed at the first add() from the parameters that then hold a gradient, in `params` order: every
    segment starts on a multiple of 4 floats (its length rounded up to 4), and a tail of n_extra floats follows the last segment -- the
    stacked loss scalars ride the same collective as one more row of the same table.  Parameters without a gradient (a frozen backbone,
    kernel_points) are simply not in the layout, as FusedAdamW skips them.  The flat tensor is zeroed once, when it is allocated, and
    its padding is never written afterwards."""

    def __init__(self, params, n_extra=0):
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
        self.offsets, total = self.layout(self.sizes, self.n_extra)
        self.flat = torch.zeros(total, dtype=torch.float32, device=self.params[held[0]].device)

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
        ops.grad_pack(grads, self.offsets[:len(grads)], self.flat, scale, self._filled, sizes=sizes)
        self._filled = True

    def all_reduce(self):
        """ONE all_reduce(SUM) of the whole flat tensor when a process group is initialised (at world size 1 too); else nothing."""
        all_reduce_sum(self.flat)

    def views(self):
        """The parameters' views of the bucket, in layout order, each of its parameter's shape."""
        return [self.flat[o:o + n].view(self.params[i].shape) for i, o, n in zip(self.index, self.offsets, self.sizes)]

    def attach(self):
        """p.grad = the parameter's view of the bucket, and the step is over: the next add() assigns.  FusedAdamW.step() then runs
        unchanged on the averaged gradient (its last_grad_norm is the averaged gradient's norm; clipping acts after averaging, as
        clip_grad_norm_ after DDP).  The views stay valid until that next add()."""
        for i, v in zip(self.index, self.views()):
            self.params[i].grad = v
        self._filled = False

    def reset(self):
        """Abandons the current optimiser step: what was added so far is dropped, the next add() assigns."""
        self._filled = False

    def extra(self):
        """The tail (n_extra floats) as a view."""
        o = self.offsets[-1]
        return self.flat[o:o + self.n_extra]
