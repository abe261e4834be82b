"""Float64 restatement of the reference's PCA colour image (render.py:38-53, feature_visualize_saving) and the seeded inputs
of its tests.  numpy only.

The seven steps, for a (C, H, W) map and a sample stride (the reference: 3):
  1. x^_p = x_p / max(||x_p||, 1e-12) for every pixel p (F.normalize: a zero pixel stays zero)
  2. the samples are pixels 0, stride, 2 stride, ... of the row-major flattened H * W index: n = ceil(HW / stride)
  3. mu = their mean, cov = sum (x^_s - mu)(x^_s - mu)^T / (n - 1)
  4. components = the eigenvectors of cov for its three largest eigenvalues, largest first, each signed so that its entry of
     largest magnitude is positive (scikit-learn >= 1.5: svd_flip(u_based_decision=False))
  5. t = (x^ - mu) . components^T
  6. lo, hi = numpy.percentile(t of the samples, all 3 n values together, [1, 99])
  7. image = clamp((t - lo) / (hi - lo), 0, 1), (H, W, 3)
"""
from typing import NamedTuple

import numpy as np


class Result(NamedTuple):
    image: np.ndarray         # (H, W, 3) float64
    mean: np.ndarray          # (C,)
    cov: np.ndarray           # (C, C)
    components: np.ndarray    # (3, C)
    lo: float
    hi: float
    eigenvalues: np.ndarray   # (C,) descending


def normalized_pixels(f):
    """(HW, C) float64: step 1 on the map as it is stored (float32 values, float64 arithmetic)."""
    f = np.asarray(f, np.float64)
    x = f.reshape(f.shape[0], -1).T
    return x / np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-12)[:, None]


def project(f, mean, components, lo, hi):
    """Steps 5 and 7 with a given fit: the (H, W, 3) float64 image of the map `f`."""
    t = (normalized_pixels(f) - np.asarray(mean, np.float64)) @ np.asarray(components, np.float64).T
    return np.clip((t - float(lo)) / (float(hi) - float(lo)), 0.0, 1.0).reshape(f.shape[1], f.shape[2], 3)


def oracle(f, stride=3):
    xh = normalized_pixels(f)
    s = xh[::stride]
    n = s.shape[0]
    mean = s.mean(axis=0)
    z = s - mean
    cov = z.T @ z / (n - 1)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1], v[:, ::-1]
    comp = v[:, :3].T.copy()
    for k in range(3):
        if comp[k, np.argmax(np.abs(comp[k]))] < 0:
            comp[k] = -comp[k]
    t = (xh - mean) @ comp.T
    lo, hi = np.percentile(t[::stride], [1, 99])
    image = np.clip((t - lo) / (hi - lo), 0.0, 1.0).reshape(f.shape[1], f.shape[2], 3)
    return Result(image, mean, cov, comp, float(lo), float(hi), w)


def determined_components(C, n):
    """How many of the three components the samples determine: cov has rank <= n - 1, and the eigenvectors of its zero
    eigenvalues are any basis of the null space (all of it when only one direction is left: C == 3 or the rank allows)."""
    rank = min(C, n - 1)
    return 3 if (rank >= 3 or C == 3 and rank >= 2) else rank


# name: (C, H, W, zero pixels, seed, seed of the offset and the directions: shared by the views of one family)
CASES = {
    "c3_20x31": (3, 20, 31, False, 101, 2033),
    "c4_20x31": (4, 20, 31, False, 102, 2043),
    "c4_1x7": (4, 1, 7, False, 103, 2043),
    "c16_37x53_zeros": (16, 37, 53, True, 504, 2160),
    "c20_45x60": (20, 45, 60, False, 105, 2200),
    "c32_45x61": (32, 45, 61, False, 106, 2320),
    "c33_37x53": (33, 37, 53, False, 107, 2330),
    "c128_12x16": (128, 12, 16, False, 108, 3280),
    "c512_12x16": (512, 12, 16, False, 2109, 7120),
    "c128_90x121": (128, 90, 121, False, 110, 3280),
    "c512_36x48": (512, 36, 48, False, 111, 7120),
    "c128_180x240": (128, 180, 240, False, 112, 3280),
    "c20_45x60_second_view": (20, 45, 60, False, 113, 2200),
}
FIXTURE_CASES = ("c3_20x31", "c4_20x31", "c16_37x53_zeros", "c20_45x60", "c128_12x16", "c512_12x16")
MIN_GAP = 0.02
ZERO_PIXELS = (0, 3, 4, 7, 30, 31)          # flattened indices set to exactly zero: sampled (0, 3, 30) and not


def _generate(C, H, W, zeros, seed, basis_seed):
    """offset + five smooth fields along random channel directions + noise, times a per-pixel magnitude.  `basis_seed` fixes
    the offset and the directions (two views of one family share them), `seed` the fields, the noise and the magnitudes."""
    b = np.random.default_rng(basis_seed)
    offset = b.standard_normal(C)
    offset *= 3.0 / np.linalg.norm(offset)
    dirs = b.standard_normal((5, C))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    r = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H) / max(H, 2), np.arange(W) / max(W, 2), indexing="ij")
    f = np.broadcast_to(offset[:, None, None], (C, H, W)).copy()
    for k, amp in enumerate((1.0, 0.6, 0.35, 0.1, 0.05)):
        fy, fx = r.uniform(0.5, 2.0, 2)
        field = np.sin(2 * np.pi * (fy * yy + fx * xx) + r.uniform(0, 2 * np.pi))
        f += amp * dirs[k][:, None, None] * field[None]
    f += 0.05 * r.standard_normal((C, H, W))
    f *= r.uniform(0.5, 2.5, (H, W))[None]
    if zeros:
        f.reshape(C, -1)[:, [i for i in ZERO_PIXELS if i < H * W]] = 0.0
    return f.astype(np.float32)


def gaps_of(f, stride=3):
    """(lambda_i - lambda_{i+1}) / lambda_1 below each component the samples determine (none below the third when C == 3)"""
    C, n = f.shape[0], -(-f.shape[1] * f.shape[2] // stride)
    w = oracle(f, stride).eigenvalues
    k = min(determined_components(C, n), C - 1)
    return [(w[i] - w[i + 1]) / w[0] for i in range(k)]


def make_inputs(name, stride=3):
    """The (C, H, W) float32 map of a case.  Asserts that the components are well separated for `stride`; a case that fails is
    re-seeded in CASES, not tolerated."""
    C, H, W, zeros, seed, basis_seed = CASES[name]
    f = _generate(C, H, W, zeros, seed, basis_seed)
    g = gaps_of(f, stride)
    assert min(g) >= MIN_GAP, f"{name} (stride {stride}): eigenvalue gaps {g}: re-seed the case"
    return f
