"""numpy statement of what feature-3dgs_amd/sam_masks.py computes, for the tests.

The resize chain, the statistics, the edge filter and the run lengths restate rules whose reference results are recorded in
tests/golden/reference_sam_masks.npz (test_sam_masks_cpu.py holds this file against them).  `nms` has NO recorded reference:
torchvision is not installed beside this project's torch, so it states torchvision.ops.nms' documented greedy rule - visit the
boxes by descending score, keep a box unless its IoU with an already kept box is > the threshold - in fp32 numpy.
"""
import numpy as np


def expand_logits(grid, h):
    """(M,g+1,g+1) float32 -> (M,h,h) float32 logits: the grid's bilinear interpolant sampled at i g / h.  h / g is a power of two,
    so the weights are dyadic and every step is one IEEE float64 operation (no library function): the same array on every machine."""
    grid = np.asarray(grid, np.float64)
    g = grid.shape[1] - 1
    f = h // g
    assert g * f == h and f & (f - 1) == 0
    i = np.arange(h)
    i0, fr = i // f, (i % f) / f
    rows = grid[:, i0] * (1 - fr)[None, :, None] + grid[:, i0 + 1] * fr[None, :, None]
    out = rows[:, :, i0] * (1 - fr)[None, None, :] + rows[:, :, i0 + 1] * fr[None, None, :]
    return out.astype(np.float32)


def taps(n_in, n_out, dtype):
    """upsample_bilinear2d, align_corners=False: (i0, i1, l0, l1) of every destination index, in `dtype` arithmetic"""
    one_half = dtype(0.5)
    scale = dtype(n_in) / dtype(n_out)
    src = scale * (np.arange(n_out).astype(dtype) + one_half) - one_half
    src = np.maximum(src, dtype(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(dtype)
    return i0, i1, dtype(1) - l1, l1


def resize(x, out_h, out_w, dtype=np.float32):
    x = np.asarray(x, dtype)
    y0, y1, ly0, ly1 = taps(x.shape[-2], out_h, dtype)
    x0, x1, lx0, lx1 = taps(x.shape[-1], out_w, dtype)
    top = lx0 * x[..., y0, :][..., x0] + lx1 * x[..., y0, :][..., x1]
    bot = lx0 * x[..., y1, :][..., x0] + lx1 * x[..., y1, :][..., x1]
    return ly0[:, None] * top + ly1[:, None] * bot


def chain(low_res, img_size, input_size, original_size, dtype=np.float32):
    """Sam.postprocess_masks: (M,h,w) -> (M,H,W)"""
    s1 = resize(low_res, img_size, img_size, dtype)[..., :input_size[0], :input_size[1]]
    return resize(s1, original_size[0], original_size[1], dtype)


def thresholds(t, offset):
    return np.float32(t), np.float32(float(t) + float(offset)), np.float32(float(t) - float(offset))


def boxes_of(masks):
    """batched_mask_to_box: int XYXY, [0,0,0,0] for an empty mask"""
    out = np.zeros((masks.shape[0], 4), np.int32)
    for m, mask in enumerate(masks):
        ys, xs = np.nonzero(mask)
        if len(ys):
            out[m] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def stats(v, t, offset):
    """(n_hi, n_lo, area, box, stability) of float32 maps v (M,H,W)"""
    t, t_hi, t_lo = thresholds(t, offset)
    n_hi = (v > t_hi).sum((1, 2)).astype(np.int32)
    n_lo = (v > t_lo).sum((1, 2)).astype(np.int32)
    area = (v > t).sum((1, 2)).astype(np.int32)
    with np.errstate(all="ignore"):
        stability = n_hi.astype(np.float32) / n_lo.astype(np.float32)
    return n_hi, n_lo, area, boxes_of(v > t), stability


def near_crop_edge(box_frame, crop_box, frame_size, atol=20.0):
    b = np.asarray(box_frame, np.float32)
    crop = np.asarray(crop_box, np.float32)[None]
    orig = np.asarray([0, 0, frame_size[1], frame_size[0]], np.float32)[None]
    return ((np.abs(b - crop) <= atol) & ~(np.abs(b - orig) <= atol)).any(1)


def uncrop(masks, crop_box, frame_size):
    out = np.zeros((masks.shape[0],) + tuple(frame_size), bool)
    x0, y0, x1, y1 = crop_box
    out[:, y0:y1, x0:x1] = masks
    return out


def rle(mask):
    """mask_to_rle_pytorch of one (FH,FW) bool mask: the counts"""
    flat = np.asarray(mask, bool).T.reshape(-1)
    change = np.nonzero(flat[1:] != flat[:-1])[0] + 1
    edges = np.concatenate([[0], change, [flat.size]])
    return ([0] if flat[0] else []) + np.diff(edges).tolist()


def rle_to_mask(counts, size):
    flat = np.zeros(size[0] * size[1], bool)
    at, value = 0, False
    for c in counts:
        flat[at:at + c] = value
        at += c
        value = not value
    return flat.reshape(size[1], size[0]).T


def pack(masks):
    """bool (M,FH,FW) -> int32 (M,FW,ceil(FH/32)) words, bit = row % 32"""
    M, FH, FW = masks.shape
    NW = (FH + 31) // 32
    rows = np.zeros((M, NW * 32, FW), np.uint64)
    rows[:, :FH] = masks
    words = (rows.reshape(M, NW, 32, FW) << np.arange(32, dtype=np.uint64)[None, None, :, None]).sum(2)
    return words.astype(np.uint32).view(np.int32).transpose(0, 2, 1).copy()


def unpack(words, FH):
    w = np.asarray(words).view(np.uint32).transpose(0, 2, 1)               # (M,NW,FW)
    bits = (w[:, :, None, :] >> np.arange(32, dtype=np.uint32)[None, None, :, None]) & 1
    return bits.reshape(w.shape[0], -1, w.shape[2])[:, :FH].astype(bool)


def iou_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    w = np.maximum(np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]), np.float32(0))
    h = np.maximum(np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]), np.float32(0))
    inter = w * h
    with np.errstate(all="ignore"):
        return inter / (area_a + area_b - inter)


def nms(boxes, scores, threshold, idxs=None):
    """torchvision's greedy rule (see the module text): the kept rows by descending score, equal scores the lower row first"""
    boxes = np.asarray(boxes, np.float32)
    order = np.argsort(-np.asarray(scores, np.float64), kind="stable")
    kept = []
    for i in order:
        if not any((idxs is None or idxs[i] == idxs[k]) and iou_f32(boxes[k], boxes[i]) > np.float32(threshold) for k in kept):
            kept.append(int(i))
    return kept
