"""numpy restatement of the guarded optimiser step (FusedAdamW(skip_nonfinite=True); csrc/optim.hip's k_grad_norm_finish under a guard,
k_adam_steps_advance, k_adam_step_guarded) and of the guarded bucket's flag, on top of tests/optim_ref.py, whose float64 update and
one-step float32 bound it imports unchanged.

    norm32 = fl32(sqrt(sum g^2)) * grad_scale        (float32 product; grad_scale None = 1)
    ok     = isfinite(norm32) and isfinite(grad_scale)
    ok == 0: the identity -- p, m, v and every step count keep their bits; skipped_steps += 1
    ok == 1: t_i += 1 for every tensor with a gradient, then tests/optim_ref.adam_update with g' = g grad_scale coef and
             bc1 = 1 - ipow(b1, t), bc2 = 1 - ipow(b2, t)

ipow: binary exponentiation over the integer t in double-double products, the kernel's loop operation for operation, so that
bias_scalars() reproduces the device's two float32 scalars BIT FOR BIT (float64 multiply, add, divide and sqrt are correctly rounded on
both sides, and neither side contracts or reorders).  Against b ** t it differs by at most 1 float64 ulp
(tests/test_nonfinite_guard_host.py asserts 4 for t <= 2^20), 2^-29 of the float32 unit roundoff the bound of tests/optim_ref.py is made
of: the bound is used as it stands."""
import numpy as np

from tests.optim_ref import AdamRef, U, adam_update, clip_coef, step_bound, total_norm      # noqa: F401  (re-exported for the tests)


_SPLIT = np.float64(134217729.0)          # 2^27 + 1


def _dd_mul(ah, al, bh, bl):
    """(ah + al)(bh + bl) as hi + lo: Dekker's product over Veltkamp's split, the kernel's opt_dd_mul operation for operation."""
    p = ah * bh
    c = _SPLIT * ah
    a1 = c - (c - ah)
    a2 = ah - a1
    c = _SPLIT * bh
    b1 = c - (c - bh)
    b2 = bh - b1
    e = ((a1 * b1 - p) + a1 * b2 + a2 * b1) + a2 * b2
    e = e + (ah * bl + al * bh)
    hi = p + e
    return hi, e - (hi - p)


def ipow(b, t):
    """b^t, t a non-negative integer: r = 1; while t: if t odd: r = r b; b = b b; t >>= 1 -- in double-double products (plain float64
    squarings double the relative error at every step: 0.999^t came out up to 5e4 ulp off for t <= 2^20; this form stays within 1)."""
    t = int(t)
    rh, rl, bh, bl = np.float64(1.0), np.float64(0.0), np.float64(b), np.float64(0.0)
    with np.errstate(under='ignore'):
        while t > 0:
            if t & 1:
                rh, rl = _dd_mul(rh, rl, bh, bl)
            bh, bl = _dd_mul(bh, bl, bh, bl)
            t >>= 1
    return float(rh)


def bias_scalars(lr, b1, b2, t):
    """(float32(lr / (1 - b1^t)), float32(sqrt(1 - b2^t))), float64 rounded once -- the kernel's two per-step scalars."""
    with np.errstate(divide='ignore'):
        return np.float32(np.float64(lr) / np.float64(1.0 - ipow(b1, t))), np.float32(np.sqrt(np.float64(1.0 - ipow(b2, t))))


def finish(sumsq, max_norm, grad_scale=None):
    """The guarded finish from the float64 sum of squares -> (norm32, coef32, ok): float32 arithmetic as the kernel's."""
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        gs = np.float32(1.0 if grad_scale is None else grad_scale)
        norm = np.float32(np.sqrt(np.float64(sumsq))) * gs
        coef = np.float32(1.0)
        if max_norm > 0:
            c = np.float32(max_norm) / (norm + np.float32(1e-6))
            coef = np.float32(1.0) if c > 1.0 else c                          # (a NaN stays a NaN)
        ok = bool(np.isfinite(norm) and np.isfinite(gs))
    return norm, coef, ok


def gradients_ok(grads, grad_scale=None):
    """The guard's decision for a list of gradients (None entries skipped)."""
    with np.errstate(over='ignore', invalid='ignore'):
        s = sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads if g is not None)
    return finish(s, 0.0, grad_scale)[2]


class GuardedAdamRef(AdamRef):
    """AdamRef under the guard: step(grads, lr=None, grad_scale=None) -> True when the step was applied.  A skipped step is the
    identity on p, m, v, t."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.skipped_steps = 0
        self.applied_steps = 0

    def step(self, grads, lr=None, grad_scale=None):
        if not gradients_ok(grads, grad_scale):
            self.skipped_steps += 1
            return False
        gs = 1.0 if grad_scale is None else float(np.float32(grad_scale))
        scaled = [None if g is None else np.asarray(g, np.float64) * gs for g in grads]
        super().step(scaled, lr=lr)
        self.applied_steps += 1
        return True
