"""FusedAdamW: the reference's optimiser step (trainer.py:116-120: clip_grad_norm_(model.parameters(), cfg.grad_clip), then
torch.optim.AdamW / Adam .step()) as three HIP kernels over all parameters at once (csrc/optim.hip): the global gradient norm in float64
partials, the clip coefficient on the device, and torch's single-tensor update with the coefficient folded in.  No host wait and no
read-back: the norm stays on the device (`last_grad_norm`).

A torch.optim.Optimizer: lr_scheduler.StepLR, zero_grad, param_groups, state_dict and load_state_dict work unchanged, and the state per
parameter is torch's own ('step', 'exp_avg', 'exp_avg_sq'), so a state_dict loads into torch.optim.AdamW over the same parameter list and
the reverse -- a reference checkpoint's 'optimizer' entry included.

Differences from the torch calls, both deliberate:
  - the clipped gradient is NOT written back to p.grad (clip_grad_norm_ scales .grad in place; nothing in the reference reads it after
    the step);
  - m = beta1 m + (1 - beta1) g where torch writes m.lerp_(g, 1 - beta1): the same number up to float32 rounding (tests/optim_ref.py
    bounds both against the float64 restatement)."""
import math
import operator

import torch

from . import ops

_is_sparse = operator.attrgetter('is_sparse')


class FusedAdamW(torch.optim.Optimizer):
    """FusedAdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, decoupled=True).
    max_grad_norm > 0: every step first clips the global gradient norm -- over all parameters with a gradient in ALL groups, the one
    clip_grad_norm_ call of the reference -- to it; <= 0: no clipping (the norm is still computed, for `last_grad_norm`).
    decoupled=False: torch.optim.Adam (the weight decay joins the gradient)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, decoupled=True):
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f'Invalid beta parameters: {betas}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if max_grad_norm != max_grad_norm:
            raise ValueError('Invalid max_grad_norm: NaN')
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = float(max_grad_norm)
        self.decoupled = bool(decoupled)
        self.last_grad_norm = None        # 0-dim float32 device tensor: the total norm BEFORE clipping of the last step (for logging)
        self.last_clip_coef = None        # ... and the coefficient the step multiplied the gradients by

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # (p, p.grad) afresh on every call: zero_grad(set_to_none=True) makes every backward allocate new gradients
        params, grads, ms, vs, steps, states, hyper = [], [], [], [], [], [], []
        state = self.state
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:             # torch's rule: no decay, no state, no step count
                    continue
                st = state[p]
                if not st:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)      # torch's layout: a CPU float32 scalar (not capturable)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                params.append(p); grads.append(g); ms.append(st['exp_avg']); vs.append(st['exp_avg_sq']); steps.append(st['step'])
                states.append(st); hyper.append(gi)
        if not params:
            return loss
        if any(map(_is_sparse, grads)):
            raise RuntimeError('FusedAdamW does not support sparse gradients')
        # the step counts: one gather, one add, one split -- every 'step' stays a 0-dim CPU tensor of its own value (a view into this
        # step's small buffer), which is what torch.optim.AdamW, state_dict() and torch.save expect; ~150 separate `step += 1` on CPU
        # scalars cost more host time than the three kernels take
        try:
            new = torch.stack(steps).to(device='cpu', dtype=torch.float32) + 1.0
        except (TypeError, RuntimeError):      # a loaded state: an old checkpoint's int counts, counts on different devices
            new = torch.tensor([float(s) for s in steps], dtype=torch.float32) + 1.0
        ts = new.tolist()
        for st, s in zip(states, new.unbind(0)):
            st['step'] = s
        groups = [(float(gr['lr']), float(gr['weight_decay']), float(gr['betas'][0]), float(gr['betas'][1]), float(gr['eps']))
                  for gr in self.param_groups]
        memo = {}
        scalars = []
        for gi, t in zip(hyper, ts):
            sc = memo.get((gi, t))
            if sc is None:
                lr, wd, b1, b2, eps = groups[gi]
                sc = memo[(gi, t)] = (lr, wd, b1, b2, eps, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t))
            scalars.append(sc)
        with ops._lib.on_device(params[0].device):
            norm_coef = ops.clip_adam_step(params, grads, ms, vs, scalars, self.max_grad_norm, decoupled=self.decoupled)
        # the kernel wrote through raw pointers: tell autograd and every cache keyed on a parameter's version (kpconv._prepared, RegTR._w_sym)
        torch.autograd.graph.increment_version(params + ms + vs)
        self.last_grad_norm, self.last_clip_coef = norm_coef[0], norm_coef[1]
        return loss
