"""A plain fp64 Adam to check FusedAdam against: torch.optim.Adam as the reference configures it (no weight decay, no
amsgrad), per element and for step count t

    m' = m + (1 - b1)(g - m)
    v' = b2 v + (1 - b2) g^2
    p' = p - (lr / (1 - b1^t)) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

Nothing here imports the product.  Two uses:

* `step_from_fp32` / `check_step`: ONE step from fp32 state, in fp64, with a decomposed bar - the moments against the fp64
  moments, the parameter change against the fp64 update formed from the moments the implementation actually stored - so the
  cancellation in m' (g close to m) does not leak into the bar on p.
* `Trajectory`: the same recurrence with its state HELD in fp64 over many steps, for drift.

The three budgets, in units of ulp32 (numpy.spacing in float32: denormal-aware), from the operation count of `adam_update`
in csrc/adam.hip.  Each correctly rounded fp32 operation costs at most 1/2 ulp of its result; a constant rounded once from
double costs 1/2 ulp relative:

  A = 2   m' = fmaf(omb1, g - m, m): the subtraction (1/2 ulp of |g - m| <= 2 max(|m|, |g|), i.e. <= 1 ulp of the larger,
          scaled by omb1 = 0.1), the rounded constant 1 - b1 (1/2 ulp of a term <= 0.2 max), the fma's one rounding (1/2):
          <= 1.5 ulp32(max(|m|, |g|)).
  B = 4   v' = fmaf(b2, v, (omb2 * g) * g): rounded b2 (1/2), rounded 1 - b2 (1/2), two multiplies (1/2 + 1/2), the fma
          (1/2), all terms non-negative and no larger than v': <= 2.5 ulp, 3 where a term sits just under a binade edge.
  C = 6   d = step_size * (m' / fmaf(sqrtf(v'), inv_sqrt_bc2, eps)): rounded lr / bc1 (1/2), rounded 1 / sqrt(bc2) (1/2),
          sqrt (1/2), fma (1/2), divide (1/2 if correctly rounded, up to 2 if not), multiply (1/2): 3 ... 4.5, and one more
          where the relative errors of the denominator meet a binade edge of d: <= 4 ... 5.5 ulp32(d),
          plus 1/2 ulp32(max(|p|, |p'|)) for the final subtraction.

torch.optim.Adam(foreach=False) in fp32 on the CPU stays at 0.55 / 2.2 / 2.75 of these units over the input family of
`family()` (tests/test_adam_oracle_cpu.py asserts that it stays inside A, B, C).
"""
import math

import numpy as np

A_M, B_V, C_D = 2.0, 4.0, 6.0

T_STEPS = (1, 2, 7, 1000, 30000)
LRS = (1.6e-6, 1.6e-4, 0.05)
# decade bands of the per-element scale; together they are the family's 1e-30 ... 1e2
BANDS = ((-30.0, -20.0), (-20.0, -10.0), (-10.0, -3.0), (-3.0, 2.0))


def _f64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def ulp32(x):
    """Spacing of float32 at |x| (as float64; denormal-aware: ulp32(0) = 2^-149)."""
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(_f64(x)).astype(np.float32)).astype(np.float64)


def step_from_fp32(p, g, m, v, lr, b1, b2, eps, t):
    """One step in fp64 from fp32 state taken as it is.  Returns (m64', v64', update_from); update_from(m_stored, v_stored)
    is the fp64 update d (p' = p - d) formed from the fp32 moments an implementation stored."""
    g, m, v = _f64(g), _f64(m), _f64(v)
    m2 = m + (1.0 - b1) * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** t)
    sqrt_bc2 = math.sqrt(1.0 - b2 ** t)

    def update_from(m_stored, v_stored):
        return step_size * _f64(m_stored) / (np.sqrt(_f64(v_stored)) / sqrt_bc2 + eps)
    return m2, v2, update_from


def step_errors(p, g, m, v, p_got, m_got, v_got, lr, b1, b2, eps, t, where=None):
    """Worst error of one step over the elements of `where` (default: all), in the units of A, B, C: a dict m / v / d.
    A non-finite result where the fp64 step is finite counts as infinitely wrong."""
    p, g, m, v = _f64(p).ravel(), _f64(g).ravel(), _f64(m).ravel(), _f64(v).ravel()
    p_got, m_got, v_got = _f64(p_got).ravel(), _f64(m_got).ravel(), _f64(v_got).ravel()
    assert p.shape == g.shape == m.shape == v.shape == p_got.shape == m_got.shape == v_got.shape
    sel = np.ones(p.shape, bool) if where is None else np.asarray(_f64(where) != 0).ravel()
    if not sel.any():
        return {"m": 0.0, "v": 0.0, "d": 0.0}
    p, g, m, v, p_got, m_got, v_got = (a[sel] for a in (p, g, m, v, p_got, m_got, v_got))
    assert np.isfinite(p).all() and np.isfinite(g).all() and np.isfinite(m).all() and np.isfinite(v).all()
    m2, v2, update_from = step_from_fp32(p, g, m, v, lr, b1, b2, eps, t)
    bad = ~(np.isfinite(p_got) & np.isfinite(m_got) & np.isfinite(v_got))
    with np.errstate(invalid="ignore", divide="ignore"):
        d = update_from(np.where(bad, 0.0, m_got), np.where(bad, 0.0, np.abs(v_got)))
        em = np.abs(m_got - m2) / ulp32(np.maximum(np.abs(m), np.abs(g)))
        ev = np.abs(v_got - v2) / ulp32(v2)
        ed = (np.abs((p - p_got) - d) - 0.5 * ulp32(np.maximum(np.abs(p), np.abs(p_got)))) / ulp32(d)
    out = {}
    for k, e in (("m", em), ("v", ev), ("d", ed)):
        e = np.where(bad | ~np.isfinite(e), np.inf, e)
        out[k] = float(e.max())
    out["v"] = float("inf") if (v_got < 0).any() else out["v"]
    return out


def step_ok(err):
    return err["m"] <= A_M and err["v"] <= B_V and err["d"] <= C_D


def check_step(*args, what="", **kw):
    err = step_errors(*args, **kw)
    assert step_ok(err), f"{what}: worst errors {err} in ulp32 units against A, B, C = {A_M}, {B_V}, {C_D}"
    return err


def family(n, band, seed):
    """fp32 (p, g, m, v) of n elements whose scale s is log-uniform over 10^band: g = s N, m = 0.3 s N, v = 0.1 (s N)^2, a
    fifth of the gradients exactly 0, a seventh of the elements with m = v = 0 (Gaussians that were never stepped); p = s_p N with s_p log-uniform over
    1e-8 ... 1e1, so that the half ulp of p in the bar does not hide the small updates of the eps regime."""
    r = np.random.default_rng(seed)
    s = 10.0 ** r.uniform(band[0], band[1], n)
    g = s * r.standard_normal(n)
    g[r.random(n) < 0.2] = 0.0
    m = 0.3 * s * r.standard_normal(n)
    v = 0.1 * (s * r.standard_normal(n)) ** 2
    fresh = r.random(n) < 1.0 / 7.0
    m[fresh] = 0.0
    v[fresh] = 0.0
    p = 10.0 ** r.uniform(-8.0, 1.0, n) * r.standard_normal(n)
    with np.errstate(under="ignore"):
        return tuple(a.astype(np.float32) for a in (p, g, m, v))


class Trajectory:
    """Adam on one tensor with p, m, v held in fp64 (torch tensors on any device); `step(g, lr)` takes the fp32 gradient
    the implementations under test were given."""

    def __init__(self, p, b1=0.9, b2=0.999, eps=1e-8):
        self.p = p.detach().double().clone()
        self.m = self.p.new_zeros(self.p.shape)
        self.v = self.p.new_zeros(self.p.shape)
        self.b1, self.b2, self.eps, self.t = b1, b2, eps, 0

    def step(self, g, lr):
        g = g.detach().double()
        self.t += 1
        self.m += (1.0 - self.b1) * (g - self.m)
        self.v.mul_(self.b2).addcmul_(g, g, value=1.0 - self.b2)
        step_size = lr / (1.0 - self.b1 ** self.t)
        self.p -= step_size * self.m / (self.v.sqrt() / math.sqrt(1.0 - self.b2 ** self.t) + self.eps)

    def prune_and_append(self, keep, extra):
        """The densification edit: rows `keep` (bool) stay with their moments, rows `extra` join with zero moments.  The
        step count stays (torch keeps one `step` per parameter across the reference's state edits)."""
        import torch
        extra = extra.to(self.p)
        self.p = torch.cat([self.p[keep], extra], 0)
        self.m = torch.cat([self.m[keep], torch.zeros_like(extra)], 0)
        self.v = torch.cat([self.v[keep], torch.zeros_like(extra)], 0)
