"""The LPIPS test cases: weights, images and pairs are pure functions of a seed, so the golden file records none of them.

Conv weights are normal with std sqrt(2 / (9 Cin)) (activations stay O(1) through the 13 layers), biases normal with std 0.05,
heads uniform in [0, 1 / C_l] (the published ones are non-negative).  An image is a smooth field plus noise in [0, 1]; the
partner of x is x itself (`same`), x with +-1/255 on a tenth of the pixels (`near`) or an unrelated image (`other`).
"""
from collections import namedtuple

import numpy as np

SEED = 4100
CONV_LAYERS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_WIDTHS = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512), (512, 512),
               (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)
GAP_SEEDS = 8                 # seeds over which the golden file measures the scalar float32-to-float64 gap

# samples: tap elements recorded per layer (of all 2N images' tensor, flattened); the whole tensor where it is smaller
Case = namedtuple("Case", "name H W kinds dead samples")
CASES = [
    Case("min16", 16, 16, ("near",), False, 1024),                 # block 5 is 1 x 1
    Case("odd", 37, 53, ("near", "other"), False, 1024),           # every pool drops a row or a column: 18x26, 9x13, 4x6, 2x3
    Case("tile_edges", 33, 65, ("other",), False, 1024),           # one past a 32- and a 64-pixel tile
    Case("wide", 24, 200, ("near",), False, 1024),                 # many pixel tiles across the conv tile edges
    Case("tall", 130, 20, ("other",), False, 1024),                # many row tiles, narrow rows
    Case("batch3", 40, 48, ("same", "near", "other"), False, 1024),
    Case("dead", 37, 53, ("near", "other"), True, 1024),           # conv5_3's bias is -1e3: the fifth taps are exactly 0
    Case("mid", 135, 240, ("near",), False, 4096),
]
BY_NAME = {c.name: c for c in CASES}


def tap_shapes(case):
    n = 2 * len(case.kinds)
    return [(n, c, case.H >> l, case.W >> l) for l, c in enumerate(TAP_CHANNELS)]


def make_weights(seed, dead=False):
    """{name: float32 array} under parameter_table()'s names."""
    rng = np.random.default_rng([seed, 1])
    out = {}
    for n, (co, ci) in zip(CONV_LAYERS, CONV_WIDTHS):
        out[f"features.{n}.weight"] = (rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32)
        out[f"features.{n}.bias"] = (rng.standard_normal(co) * 0.05).astype(np.float32)
    for i, c in enumerate(TAP_CHANNELS):
        out[f"lin.{i}.weight"] = (rng.random((1, c, 1, 1)) / c).astype(np.float32)
    if dead:
        out["features.28.bias"] = np.full(512, -1e3, np.float32)
    return out


def make_image(H, W, rng):
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    img = np.empty((3, H, W))
    for c in range(3):
        f = rng.uniform(0.02, 0.3, (3, 2))
        ph = rng.uniform(0, 2 * np.pi, 3)
        field = sum(np.sin(f[k, 0] * xx + f[k, 1] * yy + ph[k]) for k in range(3)) / 3
        img[c] = 0.5 + 0.3 * field + 0.15 * (rng.random((H, W)) - 0.5)
    return np.clip(img, 0, 1).astype(np.float32)


def make_pairs(case, seed):
    """x, y: (N, 3, H, W) float32 in [0, 1]"""
    rng = np.random.default_rng([seed, 2, case.H, case.W])
    xs, ys = [], []
    for kind in case.kinds:
        x = make_image(case.H, case.W, rng)
        if kind == "same":
            y = x.copy()
        elif kind == "near":
            step = np.where(rng.random(x.shape) < 0.5, -1.0, 1.0) * (rng.random(x.shape) < 0.1)
            y = np.clip(x + (step / 255).astype(np.float32), 0, 1).astype(np.float32)
        else:
            y = make_image(case.H, case.W, rng)
        xs.append(x)
        ys.append(y)
    return np.stack(xs), np.stack(ys)


def sample_index(size, count, layer):
    """sorted indices into a flattened tap tensor: all of it where size <= count, else the first and last 64 and a fixed draw"""
    if size <= count:
        return np.arange(size, dtype=np.int64)
    rng = np.random.default_rng([SEED, 3, layer, size])
    idx = np.concatenate([np.arange(64), np.arange(size - 64, size), rng.choice(size, count - 128, replace=False)])
    return np.unique(idx).astype(np.int64)
