"""Label maps and the numpy painter shared by the label-vote and instance-map tests (tests/test_label_votes_cpu.py,
tests/test_gpu_label_votes.py, tests/test_gpu_instance_map.py)."""
import numpy as np


def ladder(W, H, L):
    """Every 8 x 8 quadrant q (row-major over ceil(W / 8) columns) holds d = 1 + q % 12 distinct labels, all valid: 1 .. 12 per
    quadrant, across the 7 / 8 / 9 boundary between the rounds of the vote's reduction.  Needs L >= 20."""
    assert L >= 20
    y, x = np.mgrid[0:H, 0:W]
    q = (y // 8) * ((W + 7) // 8) + x // 8
    d = 1 + q % 12
    return ((5 * q) % (L - 12) + ((x % 8) + 8 * (y % 8)) % d).astype(np.int64)


def noise(W, H, L, seed=0):
    """Uniform integers in [-1, L]: up to 57 distinct valid labels in a quadrant, and both kinds of invalid label."""
    return np.random.default_rng(seed).integers(-1, L + 1, size=(H, W)).astype(np.int64)


def constant(W, H, L):
    return np.full((H, W), L - 1, np.int64)


KINDS = {"ladder": ladder, "noise": noise, "constant": constant}


def distinct_per_quadrant(labels, L):
    """The number of distinct labels in [0, L) of every 8 x 8 quadrant, flat."""
    H, W = labels.shape
    out = []
    for y0 in range(0, H, 8):
        for x0 in range(0, W, 8):
            blk = labels[y0:y0 + 8, x0:x0 + 8].reshape(-1)
            out.append(len(np.unique(blk[(blk >= 0) & (blk < L)])))
    return np.array(out)


def one_hot(labels, L):
    """(L, H, W) float32: the rule of MaskLifter.from_label_map - a label outside [0, L) belongs to no mask."""
    return (labels[None] == np.arange(L)[:, None, None]).astype(np.float32)


def as_dtype(labels, dtype):
    """The map in a narrower type; in uint8 a negative label becomes 255 (the caller keeps L <= 255 there, so it stays invalid)."""
    if dtype == np.uint8:
        assert labels.max() <= 255
        return np.where(labels < 0, 255, labels).astype(np.uint8)
    return labels.astype(dtype)


def painter(masks, order=None):
    """show_anns' loop: for j in order: img[mask_j] = position of j in the order.  masks (K, FH, FW) bool; int32 (FH, FW), -1
    where nothing was painted."""
    K, FH, FW = masks.shape
    img = np.full((FH, FW), -1, np.int32)
    for pos, j in enumerate(range(K) if order is None else order):
        img[masks[j]] = pos
    return img
