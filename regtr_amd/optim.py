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
    bounds both against the float64 restatement).

skip_nonfinite=True (opt-in; off: the launches and the bits above): torch's GradScaler / fused-optimiser found_inf behaviour ON THE
DEVICE.  The norm kernel leaves a guard word {ok, applied_steps, skipped_steps}; with ok == 0 -- a NaN, an infinity, or finite elements
whose float32 norm overflows -- the update kernel returns without writing one byte: weights, moments and the Adam step counts stand
still, and nothing waits for the host.  The step counts then live in ONE device float32 vector (state[p]['step'] is a 0-dim view into
it, torch's capturable / fused layout) and the bias corrections are formed from them in the kernel."""
import math
import operator

import torch

from . import ops

_is_sparse = operator.attrgetter('is_sparse')


class FusedAdamW(torch.optim.Optimizer):
    """FusedAdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, decoupled=True).
    max_grad_norm > 0: every step first clips the global gradient norm -- over all parameters with a gradient in ALL groups, the one
    clip_grad_norm_ call of the reference -- to it; <= 0: no clipping (the norm is still computed, for `last_grad_norm`).
    decoupled=False: torch.optim.Adam (the weight decay joins the gradient).
    skip_nonfinite=True: a step whose (scaled) gradient norm is not finite is left out on the device (the module docstring).  Then
    `skipped_steps` (cumulative) and `last_step_applied` are int32 device scalars, views of the guard word that every step rewrites;
    `grad_scale` (None = 1, or a 1-element float32 device tensor: GradBucket.attach sets it) multiplies every gradient, and the norm,
    before the clip; the version counters advance whether or not the step was applied.  The LR scheduler is the caller's and steps
    on (GradScaler's semantics)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, decoupled=True,
                 skip_nonfinite=False):
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
        self.skip_nonfinite = bool(skip_nonfinite)
        self.grad_scale = None            # skip_nonfinite: an optional 1-element float32 device tensor (None = 1)
        self.skipped_steps = None         # skip_nonfinite: int32 device scalars (views of the guard word) after the first step
        self.last_step_applied = None
        self._guard = None                # (4,) int32 {ok, applied_steps, skipped_steps, reserved}
        self._steps = None                # (number of parameters,) float32 on the device: every state[p]['step'] is a view into it
        self._step_scalars = None         # (2 x number of parameters,) float32: the per-tensor step scalars the kernels exchange
        self._steps_bound = False         # every existing state's 'step' IS such a view (false after load_state_dict)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps_bound = False         # loaded counts (CPU, integer, another optimiser's) move to the device at the next step

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._steps_bound = False         # the device vector has one entry per parameter

    def _bind_steps(self, device):
        """The step counts of every existing state into the device vector, once after construction / load_state_dict (the only host
        reads of the guarded optimiser: the loaded counts may be CPU scalars or ints)."""
        plist = [p for group in self.param_groups for p in group['params']]
        self._index = {p: i for i, p in enumerate(plist)}
        host = [float(self.state[p]['step']) if p in self.state and 'step' in self.state[p] else 0.0 for p in plist]
        self._steps = torch.tensor(host, dtype=torch.float32).to(device)
        self._step_scalars = torch.empty(2 * len(host), dtype=torch.float32, device=device)      # the kernels' workspace
        for p, view in zip(plist, self._steps.unbind(0)):
            if p in self.state and 'step' in self.state[p]:
                self.state[p]['step'] = view
        if self._guard is None or self._guard.device != self._steps.device:
            self._guard = ops.new_guard(device)
            self.skipped_steps, self.last_step_applied = self._guard[2], self._guard[0]
        self._steps_bound = True

    def _step_guarded(self):
        params, grads, ms, vs, index, hyper = [], [], [], [], [], []
        state = self.state
        first = next((p for group in self.param_groups for p in group['params'] if p.grad is not None), None)
        if first is None:
            return
        if not first.is_cuda:
            raise RuntimeError(f'FusedAdamW: the parameters must be GPU tensors (got {first.device}); there is no CPU fallback')
        if not self._steps_bound:
            self._bind_steps(first.device)
        for gi, group in enumerate(self.param_groups):
            for p in group['params']:
                g = p.grad
                if g is None:
                    continue
                st = state[p]
                i = self._index[p]
                if not st:
                    st['step'] = self._steps[i]                               # (zero: the vector starts so)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                params.append(p); grads.append(g); ms.append(st['exp_avg']); vs.append(st['exp_avg_sq']); index.append(i); hyper.append(gi)
        if any(map(_is_sparse, grads)):
            raise RuntimeError('FusedAdamW does not support sparse gradients')
        groups = [(float(gr['lr']), float(gr['weight_decay']), float(gr['betas'][0]), float(gr['betas'][1]), float(gr['eps']))
                  for gr in self.param_groups]
        with ops._lib.on_device(params[0].device):
            norm_coef = ops.clip_adam_step_guarded(params, grads, ms, vs, [groups[gi] for gi in hyper], index, self._steps, self._guard,
                                                   self.max_grad_norm, grad_scale=self.grad_scale, decoupled=self.decoupled,
                                                   step_scalars=self._step_scalars)
        # applied or not -- the host does not know, and must not ask: every cache keyed on a version rebuilds either way
        torch.autograd.graph.increment_version(params + ms + vs)
        self.last_grad_norm, self.last_clip_coef = norm_coef[0], norm_coef[1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.skip_nonfinite:
            self._step_guarded()
            return loss
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
