"""numpy statement of the small-region removal of feature-3dgs_amd/sam_masks.py (remove_small_regions, postprocess_small_regions),
for the tests.  The reference's results are recorded in tests/golden/reference_small_regions.npz (made by the reference's own
utils/amg.py:remove_small_regions over scipy.ndimage.label); test_sam_regions_cpu.py holds this file against them.

The labelling here is independent of both: HORIZONTAL runs of every row (the kernels use vertical runs of every column), joined
by a two-pass union-find whose root is the smallest run, 8-connected: run [a, b] of row y and run [c, d] of row y + 1 touch iff
c <= b + 1 and d >= a - 1.  Runs are numbered in row-major order, so a component's root is the run that holds its first pixel
in row-major order, and components sorted by root come in scipy.ndimage.label's order - the order that decides a tie for the
largest component (this project's rule; OpenCV's was not consulted).  No scipy."""
import numpy as np


def components(img):
    """(runs (n,3) int: row, first column, last column; root (n,) int: the smallest run of each run's component)"""
    img = np.asarray(img, bool)
    H, W = img.shape
    edge = np.diff(np.concatenate([np.zeros((H, 1), np.int8), img.astype(np.int8), np.zeros((H, 1), np.int8)], 1), axis=1)
    ys, x0 = np.nonzero(edge == 1)
    _, x1 = np.nonzero(edge == -1)
    runs = np.stack([ys, x0, x1 - 1], 1)
    n = len(runs)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = np.searchsorted(ys, np.arange(H + 1))                 # the first run of every row
    for y in range(H - 1):
        i, i_end, j, j_end = first[y], first[y + 1], first[y + 1], first[y + 2]
        while i < i_end and j < j_end:
            a, b, c, d = runs[i, 1], runs[i, 2], runs[j, 1], runs[j, 2]
            if c <= b + 1 and d >= a - 1:
                ri, rj = find(i), find(j)
                if ri != rj:
                    parent[max(ri, rj)] = min(ri, rj)
            if b <= d:
                i += 1
            else:
                j += 1
    return runs, np.array([find(i) for i in range(n)], np.int64)


def remove_small_regions(mask, area_thresh, mode):
    """utils/amg.py:remove_small_regions of one (H,W) bool mask: (mask, changed)"""
    assert mode in ("holes", "islands")
    mask = np.asarray(mask, bool)
    holes = mode == "holes"
    runs, root = components(~mask if holes else mask)
    if len(runs) == 0:
        return mask, False
    length = runs[:, 2] - runs[:, 1] + 1
    roots, inverse = np.unique(root, return_inverse=True)         # ascending: the order of the components' first pixels
    sizes = np.bincount(inverse, weights=length).astype(np.int64)
    small = sizes < area_thresh
    if not small.any():
        return mask, False
    if holes:
        paint = small                                             # filled
    else:
        paint = ~small                                            # kept
        if not paint.any():
            paint[int(np.argmax(sizes))] = True                   # every one small: the largest, the first of equals
    out = mask.copy() if holes else np.zeros_like(mask)
    for (y, a, b), c in zip(runs, inverse):
        if paint[c]:
            out[y, a:b + 1] = True
    return out, True


def postprocess(masks, min_area):
    """holes, then islands, of (K,H,W) bool masks: (after holes, after islands, changed by holes, changed by islands, area, box)"""
    filled, final, ch_h, ch_i = [], [], [], []
    for m in masks:
        f, c = remove_small_regions(m, min_area, "holes")
        filled.append(f)
        ch_h.append(c)
        f, c = remove_small_regions(f, min_area, "islands")
        final.append(f)
        ch_i.append(c)
    final = np.array(final).reshape(masks.shape)
    box = np.zeros((len(final), 4), np.int32)
    for k, m in enumerate(final):
        ys, xs = np.nonzero(m)
        if len(ys):
            box[k] = (xs.min(), ys.min(), xs.max(), ys.max())
    return (np.array(filled).reshape(masks.shape), final, np.array(ch_h, bool), np.array(ch_i, bool),
            final.sum((1, 2)).astype(np.int32), box)
