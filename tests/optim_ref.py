"""numpy float64 restatement of the reference's optimiser step (trainer.py:116-121, generic_reg_model.py:38-58):
torch.nn.utils.clip_grad_norm_ over all parameters, torch.optim.AdamW / Adam with a step count PER TENSOR (a parameter whose gradient
is None on a step is skipped: no decay, no state change, no count), and StepLR.  tests/test_optim_host.py pins it to the real torch calls
on CPU float64 tensors; the GPU tests (tests/test_gpu_optim.py) compare regtr_amd's kernels and FusedAdamW with it.

    total_norm = sqrt(sum_t sum_i g_ti^2);  coef = min(1, max_norm / (total_norm + 1e-6))        (max_norm <= 0: no clipping, coef = 1)
    g' = g coef
    AdamW: p = p (1 - lr wd)            Adam: g' = g' + wd p
    m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
    p = p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),   bc1 = 1 - b1^t, bc2 = 1 - b2^t

ONE-STEP FLOAT32 ERROR BOUND (step_bound).  u = 2^-24 is float32's unit roundoff: fl(x op y) = (x op y)(1 + d), |d| <= u, for + - * /
and sqrt (the kernel is compiled without contraction, with correctly rounded divide and sqrt), plus at most TINY = 2^-149 absolute per
operation where a result is subnormal.  p, g, m, v are float32 numbers, hence exact in float64.  Every host scalar (1 - lr wd, wd, b1,
1 - b1, b2, 1 - b2, lr / bc1, sqrt(bc2), eps) is computed in float64 and rounded to float32 once: relative error u each.  The clip
coefficient the kernel multiplies by may differ from the float64 one by a relative c (coef_rel; 0 when the test hands both the same
float32 number).  To first order in u, with E(x) the bound on |computed x - exact x|:

    g' = fl(g coef):                           E(g') = (u + c) |g'|
    Adam only, g' = fl(g' + fl(wd p)):         E(g') += 2u |wd p| + u (|g'| + |wd p|)              (wd rounded, product, sum)
    m  = fl(fl(b1 m) + fl((1-b1) g')):         E(m)  = 4u (b1 |m| + (1-b1) |g'|) + (1-b1) E(g')
         (2u per product: scalar rounded + product; u (b1|m| + (1-b1)|g'|) for the sum -- 3u in all; 4u so that torch's own form
          m + (1-b1)(g' - m), three roundings on (1-b1)(|g'| + |m|) and one on the sum, stays inside the same bound for b1 >= 0.75)
    v  = fl(fl(b2 v) + fl(fl((1-b2) g') g')):  E(v)  = 3u b2 v + (1-b2) (4u g'^2 + 2 |g'| E(g'))
         (every term is >= 0: no cancellation, the relative error of v is about 4u + 2c however small v is)
    s  = fl(sqrt(v~)), v~ the kernel's v:      |sqrt(v~) - sqrt(v)| <= min(E(v) / sqrt(v), sqrt(E(v))) =: E0
         (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b) <= |a - b| / sqrt b, and <= sqrt|a - b|: the second form is the one that
          stays finite at the v -> 0 end, where the first divides by zero)
                                               E(s) = E0 + u (sqrt(v) + E0)
    q  = fl(s / sqrt(bc2)):                    E(q) = (E(s) + 3u sqrt(v)) / sqrt(bc2)
         (scalar rounded, quotient: 2u; 3u so that s fl(1 / sqrt(bc2)), the way torch's kernels divide by a host scalar, is covered)
    D  = fl(q + eps):                          E(D) = E(q) + u eps + u (sqrt(v) / sqrt(bc2) + eps) (eps rounded, sum)
         (at v -> 0 the denominator is eps itself, known to relative 2u: nothing blows up as long as eps > 0)
    r  = fl(m~ / D~):                          E(r) = E(m) / D_lo + |m| E(D) / (D D_lo) + u |m| / D_lo,   D_lo = D - E(D) > 0
    t  = fl(fl(lr / bc1) r):                   E(t) = (lr / bc1) E(r) + 2u (lr / bc1) |m| / D
    AdamW, p' = fl(p fl(1 - lr wd)):           E(p') = 2u |p (1 - lr wd)|;    Adam: p' = p, E(p') = 0
    p  = fl(p' - t):                           E(p) = E(p') + E(t) + u (|p'| + |t|)

Each E gains TINY per rounding and the whole is multiplied by 1 + 2^-10 for the second-order terms (they are of relative size u)."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
SLACK = 1.0 + 2.0 ** -10


def total_norm(grads):
    """sqrt of the sum of squares over every gradient that is not None, float64."""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, np.float64) ** 2)) for g in grads if g is not None)))


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient; max_norm <= 0: no clipping.  A NaN norm gives NaN (torch.clamp keeps it)."""
    if max_norm <= 0:
        return 1.0
    c = float(max_norm) / (float(norm) + 1e-6)          # (an infinite norm gives 0.0, as torch's division does)
    return c if c != c else min(1.0, c)


def adam_update(p, g, m, v, coef, lr, wd, b1, b2, eps, t, decoupled=True):
    """One tensor, float64, step count t (after the increment) -> (p, m, v)."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    g = g * coef
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p, m, v


def step_bound(p, g, m, v, coef, lr, wd, b1, b2, eps, t, decoupled=True, coef_rel=0.0):
    """The module docstring's bound for one float32 step from float32-representable p, g, m, v -> (E(p), E(m), E(v)) arrays."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    u = U
    bc1, sb = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
    ss = lr / bc1
    gp = np.abs(g * coef)
    eg = (u + coef_rel) * gp + TINY
    if not decoupled:
        wp = np.abs(wd * p)
        eg = eg + 2 * u * wp + u * (gp + wp) + 2 * TINY
        gx = g * coef + wd * p
        gp = np.abs(gx)
    else:
        gx = g * coef
    em = 4 * u * (b1 * np.abs(m) + (1 - b1) * gp) + (1 - b1) * eg + 3 * TINY
    ev = 3 * u * b2 * v + (1 - b2) * (4 * u * gp * gp + 2 * gp * eg) + 4 * TINY
    m1 = b1 * m + (1 - b1) * gx
    v1 = b2 * v + (1 - b2) * gx * gx
    rv = np.sqrt(v1)
    with np.errstate(divide='ignore', invalid='ignore'):
        e0 = np.where(rv > 0, np.minimum(ev / np.where(rv > 0, rv, 1.0), np.sqrt(ev)), np.sqrt(ev))
    es = e0 + u * (rv + e0) + TINY
    eq = (es + 3 * u * rv) / sb + TINY
    D = rv / sb + eps
    eD = eq + u * eps + u * D + TINY
    D_lo = D - eD
    assert np.all(D_lo > 0), 'the bound needs a denominator known to better than itself (eps > 0)'
    er = em / D_lo + np.abs(m1) * eD / (D * D_lo) + u * np.abs(m1) / D_lo + TINY
    et = ss * er + 2 * u * ss * np.abs(m1) / D + TINY
    if decoupled:
        p1 = p * (1.0 - lr * wd)
        ep1 = 2 * u * np.abs(p1) + TINY
    else:
        p1, ep1 = p, 0.0
    ep = ep1 + et + u * (np.abs(p1) + ss * np.abs(m1) / D) + TINY
    return ep * SLACK, em * SLACK, ev * SLACK


def step_lr(base_lr, step_size, gamma, epoch):
    """torch.optim.lr_scheduler.StepLR's lr after `epoch` scheduler steps."""
    return base_lr * gamma ** (epoch // step_size)


class AdamRef:
    """Clip + AdamW / Adam over a list of float64 arrays with torch's per-tensor state.  step(grads, lr): grads[i] None skips tensor i."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, decoupled=True):
        self.p = [np.array(x, dtype=np.float64) for x in params]
        self.m = [None] * len(self.p)
        self.v = [None] * len(self.p)
        self.t = [0] * len(self.p)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.max_grad_norm, self.decoupled = max_grad_norm, decoupled
        self.last_norm = self.last_coef = None

    def step(self, grads, lr=None, coef=None):
        """coef: use this coefficient instead of the float64 one (a test that hands the kernel a float32 coefficient)."""
        lr = self.lr if lr is None else lr
        self.last_norm = total_norm(grads)
        c = clip_coef(self.last_norm, self.max_grad_norm) if coef is None else coef
        self.last_coef = c
        for i, g in enumerate(grads):
            if g is None:
                continue
            if self.m[i] is None:
                self.m[i], self.v[i] = np.zeros_like(self.p[i]), np.zeros_like(self.p[i])
            self.t[i] += 1
            self.p[i], self.m[i], self.v[i] = adam_update(self.p[i], g, self.m[i], self.v[i], c, lr, self.wd, self.betas[0], self.betas[1],
                                                          self.eps, self.t[i], self.decoupled)
        return self.last_norm, c
