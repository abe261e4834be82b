"""fp64 restatements for the capturable optimizer step.  Nothing here imports the product.

* `schedule(i, ...)`: the learning-rate schedule a scheduled group follows, at iteration i.
* `constants(lr, b1, b2, t)`: the two fp32 constants of an Adam step, formed in fp64 and rounded once.
* `reset_opacity(raw, cap)`: the in-place opacity reset, in fp64 from the fp32 input.
"""
import math

import numpy as np

# the grid the CPU test and the GPU test share
DELAY, MAX_STEPS = 100, 30000
ITERATIONS = (0, 1, DELAY // 2, DELAY, MAX_STEPS // 2, MAX_STEPS, MAX_STEPS + 5)
DELAY_MULTS = (1.0, 0.01)
DELAY_STEPS = (0, DELAY)
RATES = ((1.6e-4, 1.6e-6), (0.0, 0.0))
STEP_WORDS = (0, 1, 6, 999, 29999)


def schedule(i, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """Log-linear from lr_init at i = 0 to lr_final from max_steps on; both zero: the group is frozen.  During the first
    lr_delay_steps iterations the rate is scaled by a factor that goes from lr_delay_mult to 1 along a quarter sine."""
    if lr_init == 0.0 and lr_final == 0.0:
        return 0.0
    factor = 1.0
    if lr_delay_steps > 0:
        w = min(max(i / lr_delay_steps, 0.0), 1.0)
        factor = lr_delay_mult + (1.0 - lr_delay_mult) * math.sin(0.5 * math.pi * w)
    u = min(max(i / max_steps, 0.0), 1.0)
    return factor * math.exp(math.log(lr_init) * (1.0 - u) + math.log(lr_final) * u)


def constants(lr, b1, b2, t):
    """(float32(lr / (1 - b1^t)), float32(1 / sqrt(1 - b2^t))) as numpy float32 scalars."""
    t = float(t)
    return np.float32(lr / (1.0 - b1 ** t)), np.float32(1.0 / math.sqrt(1.0 - b2 ** t))


def reset_opacity(raw, cap=0.01):
    """logit(min(sigmoid(raw), cap)) per element in fp64; NaN stays NaN, -inf stays -inf (sigmoid 0, log 0)."""
    x = np.asarray(raw, dtype=np.float64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
        c = np.where(np.isnan(s), s, np.minimum(s, float(cap)))
        return np.log(c / (1.0 - c))
