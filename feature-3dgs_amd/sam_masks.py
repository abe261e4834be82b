"""SAM mask post-processing on the device: from the mask decoder's low-resolution logits to the list of mask records, without
the full-size float masks ever existing.

Replaces what the reference runs after the decoder (encoders/sam_encoder/segment_anything) -

    masks = sam.postprocess_masks(low_res_masks, input_size, original_size)      # modeling/sam.py:133-162: two bilinear resizes
    data["stability_score"] = calculate_stability_score(masks, mask_threshold, offset)   # automatic_mask_generator.py:295-320
    data["masks"] = masks > mask_threshold;  data["boxes"] = batched_mask_to_box(data["masks"])
    keep_mask = ~is_box_near_crop_edge(...);  uncrop_masks(...);  data["rles"] = mask_to_rle_pytorch(data["masks"])
    keep_by_nms = batched_nms(boxes, scores, idxs, iou_threshold)                # torchvision, not installed beside this project

- with

    st = mask_pass(low_res, img_size=1024, input_size=(576, 1024), original_size=(1080, 1920), iou_preds=iou, pred_iou_thresh=0.88,
                   stability_score_thresh=0.95)          # MaskStats of device tensors, no host read
    masks = upscale_masks(low_res, 1024, (576, 1024), (1080, 1920))              # the drop-in for postprocess_masks
    keep, count = box_nms(boxes, scores, 0.7);  keep = batched_nms(boxes, scores, idxs, 0.7)
    rles = masks_to_rle(st.packed, st.kept_index[:k]);  dense = unpack_masks(st.packed, index)
    ids = instance_map(st.packed, paint_order(st.area))                          # segment.py:57-70 show_anns: int32 (FH, FW), -1 = none
    new, changed = remove_small_regions(st.packed, 100, "holes", index)          # utils/amg.py:remove_small_regions, K masks at once
    sr = postprocess_small_regions(st.packed, 100, index)                        # holes, then islands: packed, changed, area, box
    pp = MaskPostprocessor((1080, 1920), min_mask_region_area=100);  pp.add_batch(...);  records = pp.finish()      # generate's records

csrc/sam_masks.hip and csrc/mask_regions.hip behind include/f3dgs.h (f3dgs_sam_masks, f3dgs_sam_upscale, f3dgs_box_nms,
f3dgs_mask_rle_*, f3dgs_mask_unpack, f3dgs_mask_instance_map, f3dgs_mask_regions).  The small-region removal labels the bit-packed masks where they lie:
its nodes are the vertical runs of a column, joined by a union-find of integer atomics; no dense label image, no OpenCV.
Both resizes are PyTorch's upsample_bilinear2d (align_corners=False) in fp32, one rounding per operation, kept as two stages;
counts, boxes and bits are integers, the stability score one IEEE division: two calls give the same bits.  The networks (image
encoder, prompt encoder, mask decoder) are not part of this project.

HIP only; no CPU fallback; argument errors are raised as ValueError before any device work.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

MAX_MASKS = 65535               # masks per mask_pass / upscale_masks call
MAX_SIZE = 32768                # any edge length
NMS_MAX = 16384                 # F3DGS_BOX_NMS_MAX
OUTPUT_MODES = ("uncompressed_rle", "binary_mask")

PackedMasks = namedtuple("PackedMasks", ["words", "frame_size"])
PackedMasks.__doc__ = """words: int32 (M, FW, ceil(FH / 32)) - word (x, y // 32) holds rows 32 (y // 32) .. + 31 of column x, bit = row % 32;
frame_size: (FH, FW)."""
SmallRegions = namedtuple("SmallRegions", ["packed", "changed", "area", "box"])
REGION_MODES = ("holes", "islands")
MaskStats = namedtuple("MaskStats", ["n_hi", "n_lo", "area", "box", "box_frame", "stability", "packed", "keep", "kept_index", "kept_count"])


def _C():
    from diff_gaussian_rasterization import _C as ext
    return ext


def _int(v, name, lo=1, hi=MAX_SIZE):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} {v!r}: an integer from {lo} to {hi} expected")
    return int(v)


def _pair(v, name, lo=1):
    if not isinstance(v, (tuple, list)) and not (torch.is_tensor(v) or isinstance(v, np.ndarray)) or len(v) != 2:
        raise ValueError(f"{name} {v!r}: two integers (height, width) expected")
    return _int(v[0], f"{name}[0]", lo), _int(v[1], f"{name}[1]", lo)


def _number(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or np.isnan(float(v)):
        raise ValueError(f"{name} {v!r}: a number expected")
    return float(v)


def _logits(low_res):
    if not torch.is_tensor(low_res):
        raise ValueError(f"low_res: a tensor expected, got {type(low_res).__name__}")
    if low_res.dtype != torch.float32:
        raise ValueError(f"low_res: float32 logits expected, got {low_res.dtype}")
    if low_res.dim() != 3 or low_res.shape[1] < 1 or low_res.shape[2] < 1:
        raise ValueError(f"low_res: (M,h,w) expected, got {tuple(low_res.shape)}")
    if low_res.shape[0] > MAX_MASKS or max(low_res.shape[1:]) > MAX_SIZE:
        raise ValueError(f"low_res {tuple(low_res.shape)}: up to {MAX_MASKS} masks of up to {MAX_SIZE} a side are supported")
    return low_res.detach()


def _sizes(low_res, img_size, input_size, original_size):
    lr = _logits(low_res)
    S = _int(img_size, "img_size")
    ih, iw = _pair(input_size, "input_size")
    if ih > S or iw > S:
        raise ValueError(f"input_size {(ih, iw)} beyond img_size {S}")
    H, W = _pair(original_size, "original_size")
    return lr, S, ih, iw, H, W


def _on_device(t, name, what):
    if t.device.type != "cuda":
        raise ValueError(f"{name} lives on {t.device}: {what} on a HIP device only (no CPU path)")


def _prepare(low_res, img_size, input_size, original_size, mask_threshold, stability_offset, iou_preds, pred_iou_thresh, crop_box,
             frame_size, stability_score_thresh):
    lr, S, ih, iw, H, W = _sizes(low_res, img_size, input_size, original_size)
    t, off = _number(mask_threshold, "mask_threshold"), _number(stability_offset, "stability_offset")
    pit, sst = _number(pred_iou_thresh, "pred_iou_thresh"), _number(stability_score_thresh, "stability_score_thresh")
    if crop_box is None:
        crop = (0, 0, W, H)
    else:
        if not isinstance(crop_box, (tuple, list, np.ndarray)) or len(crop_box) != 4:
            raise ValueError(f"crop_box {crop_box!r}: (x0, y0, x1, y1) expected")
        crop = tuple(_int(v, "crop_box", 0) for v in crop_box)
        if (crop[3] - crop[1], crop[2] - crop[0]) != (H, W):
            raise ValueError(f"crop_box {crop} is not of original_size {(H, W)}")
    FH, FW = (crop[3], crop[2]) if frame_size is None else _pair(frame_size, "frame_size")
    if frame_size is None and crop_box is not None and (crop[0] or crop[1]):
        raise ValueError("crop_box: a crop that does not start at (0, 0) needs frame_size")
    if crop[2] > FW or crop[3] > FH:
        raise ValueError(f"crop_box {crop} does not lie in the frame {(FH, FW)}")
    if FH * FW > 1 << 30:
        raise ValueError(f"frame_size {(FH, FW)}: up to 2^30 pixels are supported")
    iou = None
    if iou_preds is not None:
        if not torch.is_tensor(iou_preds) or iou_preds.dtype != torch.float32 or tuple(iou_preds.shape) != (lr.shape[0],):
            raise ValueError(f"iou_preds: a float32 tensor ({lr.shape[0]},) expected")
        iou = iou_preds.detach()
    _on_device(lr, "low_res", "the mask pass runs")        # last, so that every other error can be met without a device
    if iou is not None and iou.device != lr.device:
        raise ValueError(f"low_res is on {lr.device}, iou_preds on {iou.device}")
    # the reference compares float32 masks with Python floats: the sums are formed in double and rounded once
    th = (float(np.float32(t)), float(np.float32(t + off)), float(np.float32(t - off)))
    return lr, S, ih, iw, H, W, crop, FH, FW, iou, pit, sst, th


@torch.no_grad()
def mask_pass(low_res, img_size, input_size, original_size, *, mask_threshold=0.0, stability_offset=1.0, iou_preds=None,
              pred_iou_thresh=0.0, crop_box=None, frame_size=None, stability_score_thresh=0.0, edge_filter=True) -> MaskStats:
    """The fused pass and the filter: MaskStats of device tensors, one row per mask, no host read.
    low_res (M,h,w) float32 logits; per pixel of the (H,W) = original_size crop the reference's v (resize to img_size squared, keep
    [:input_size[0], :input_size[1]], resize to original_size).  n_hi, n_lo, area (M,) int32: the pixels with v > t + offset,
    v > t - offset, v > t.  box (M,4) int32 XYXY in the crop's frame by batched_mask_to_box's rule ([0,0,0,0] when empty),
    box_frame the same shifted by the crop's origin.  stability (M,) float32 = n_hi / n_lo (0 / 0 = NaN).  packed: PackedMasks of
    the masks v > t in the full frame_size frame, zero outside the crop.  crop_box (x0,y0,x1,y1) of original_size in the frame;
    by default the crop is the whole frame.  A mask whose iou_preds is not > pred_iou_thresh (NaN included; a threshold <= 0
    switches the test off) is skipped: zero bits, zero counts.  keep (M,) bool = iou ok and stability >= stability_score_thresh
    (off when <= 0) and, with edge_filter, not is_box_near_crop_edge (atol 20); kept_index (M,) int32 the kept rows ascending
    then -1, kept_count (1,) int32."""
    lr, S, ih, iw, H, W, crop, FH, FW, iou, pit, sst, th = _prepare(low_res, img_size, input_size, original_size, mask_threshold,
                                                                   stability_offset, iou_preds, pred_iou_thresh, crop_box, frame_size,
                                                                   stability_score_thresh)
    packed, counts, box, box_frame, stab, keep, kept_index, kept_count = _C().sam_masks(
        lr, iou, pit, S, ih, iw, H, W, FH, FW, crop[0], crop[1], th[0], th[1], th[2], sst, bool(edge_filter))
    return MaskStats(n_hi=counts[:, 0], n_lo=counts[:, 1], area=counts[:, 2], box=box, box_frame=box_frame, stability=stab,
                     packed=PackedMasks(packed, (FH, FW)), keep=keep, kept_index=kept_index, kept_count=kept_count)


@torch.no_grad()
def upscale_masks(low_res, img_size, input_size, original_size, out=torch.float32, mask_threshold=0.0) -> torch.Tensor:
    """Drop-in for Sam.postprocess_masks: (M,H,W) float32 of low_res (M,h,w) - or, with out=torch.bool, the masks
    v > mask_threshold.  (B,C,h,w) logits give (B,C,H,W), as the reference's."""
    lead = None
    if torch.is_tensor(low_res) and low_res.dim() == 4:
        lead, low_res = tuple(low_res.shape[:2]), low_res.reshape(-1, *low_res.shape[2:])
    lr, S, ih, iw, H, W = _sizes(low_res, img_size, input_size, original_size)
    if out not in (torch.float32, torch.bool):
        raise ValueError(f"out {out!r}: torch.float32 or torch.bool expected")
    t = _number(mask_threshold, "mask_threshold")
    _on_device(lr, "low_res", "the masks are made")
    res = _C().sam_upscale(lr, S, ih, iw, H, W, float(np.float32(t)), out == torch.bool)
    return res if lead is None else res.reshape(*lead, H, W)


# ---- NMS --------------------------------------------------------------------------------------------------------------------
def _nms_args(boxes, scores, iou_threshold, idxs):
    if not torch.is_tensor(boxes) or boxes.dtype not in (torch.int32, torch.int64, torch.float32) or boxes.dim() != 2 or boxes.shape[1] != 4:
        raise ValueError("boxes: an int32 or float32 tensor (M,4) XYXY expected")
    M = boxes.shape[0]
    if not torch.is_tensor(scores) or not scores.dtype.is_floating_point or tuple(scores.shape) != (M,):
        raise ValueError(f"scores: a floating-point tensor ({M},) expected")
    if idxs is not None and (not torch.is_tensor(idxs) or idxs.dtype.is_floating_point or tuple(idxs.shape) != (M,)):
        raise ValueError(f"idxs: an integer tensor ({M},) expected")
    thr = _number(iou_threshold, "iou_threshold")
    if M > NMS_MAX:
        raise ValueError(f"{M} boxes: up to {NMS_MAX} are supported")
    _on_device(boxes, "boxes", "the suppression runs")
    if scores.device != boxes.device or (idxs is not None and idxs.device != boxes.device):
        raise ValueError("boxes, scores and idxs live on different devices")
    return M, thr


@torch.no_grad()
def box_nms(boxes, scores, iou_threshold, idxs=None):
    """Greedy box NMS on the device: (keep (M,) int32, count (1,) int32) - the kept rows by descending score (equal scores: the
    lower row first), then -1.  A box is suppressed when its IoU with an earlier KEPT box (of the same idxs category, if given)
    is > iou_threshold; IoU = inter / (area_a + area_b - inter) in fp32, no +1; two empty boxes (NaN) never suppress.  boxes
    (M,4) int32 or float32, M <= 16384.  No host read."""
    M, thr = _nms_args(boxes, scores, iou_threshold, idxs)
    order = torch.sort(scores.detach(), descending=True, stable=True)[1]
    b = boxes.detach().to(torch.float32)[order]
    cats = None if idxs is None else idxs.detach()[order].to(torch.int32)
    return _C().box_nms(b, cats, thr, order.to(torch.int32))


def batched_nms(boxes, scores, idxs, iou_threshold) -> torch.Tensor:
    """torchvision.ops.batched_nms: the int64 rows kept, by descending score (one host read, for the count, as torchvision's)."""
    keep, count = box_nms(boxes, scores, iou_threshold, idxs)
    return keep[:int(count)].to(torch.int64)


# ---- RLE and dense masks ----------------------------------------------------------------------------------------------------
def _packed_args(packed, index, what):
    if not isinstance(packed, PackedMasks) or not torch.is_tensor(packed.words):
        raise ValueError("packed: the PackedMasks of mask_pass or pack_masks expected")
    FH, FW = _pair(packed.frame_size, "packed.frame_size")
    w = packed.words
    if w.dtype != torch.int32 or w.dim() != 3 or tuple(w.shape[1:]) != (FW, (FH + 31) // 32):
        raise ValueError(f"packed.words: int32 (M,{FW},{(FH + 31) // 32}) expected for a {(FH, FW)} frame, got {w.dtype} {tuple(w.shape)}")
    if index is not None:
        if not torch.is_tensor(index) or index.dtype not in (torch.int32, torch.int64) or index.dim() != 1:
            raise ValueError("index: an int32 or int64 tensor (K,) of mask rows expected")
    _on_device(w, "packed", what)
    if index is not None:
        if index.device != w.device:
            raise ValueError(f"packed is on {w.device}, index on {index.device}")
        index = index.detach().to(torch.int32).contiguous()
    return w.contiguous(), index, FH, FW


@torch.no_grad()
def pack_masks(masks) -> PackedMasks:
    """PackedMasks of bool masks (M,FH,FW) on the device (torch plumbing: the fused pass writes this form itself)."""
    if not torch.is_tensor(masks) or masks.dtype != torch.bool or masks.dim() != 3 or masks.shape[1] < 1 or masks.shape[2] < 1:
        raise ValueError("masks: a bool tensor (M,FH,FW) expected")
    M, FH, FW = masks.shape
    NW = (FH + 31) // 32
    rows = torch.zeros((M, NW * 32, FW), dtype=torch.int64, device=masks.device)
    rows[:, :FH] = masks
    weights = (1 << torch.arange(32, dtype=torch.int64, device=masks.device))[None, None, :, None]
    words = (rows.view(M, NW, 32, FW) * weights).sum(2)                    # (M,NW,FW) in [0, 2^32)
    words = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
    return PackedMasks(words.permute(0, 2, 1).contiguous(), (FH, FW))


@torch.no_grad()
def masks_to_rle(packed, index=None) -> list:
    """mask_to_rle_pytorch of the masks packed[index] (all, without index): [{"size": [FH, FW], "counts": [...]}], runs down the
    columns and across column ends, a leading 0 where pixel (0, 0) is set.  Two kernels (the lengths; the counts) around a
    prefix sum, then ONE host read of the lengths and counts together.  The read-back buffer is sized before the lengths are
    known, at 4 FW + 64 counts per mask (a blob has about 2 FW); only a list that outgrows it costs a second emit and read."""
    w, index, FH, FW = _packed_args(packed, index, "the run lengths are made")
    K = w.shape[0] if index is None else index.shape[0]
    if K == 0:
        return []
    C = _C()
    lens = C.mask_rle_count(w, index, FH)
    ends = torch.cumsum(lens, 0, dtype=torch.int64)

    def emit(capacity):
        out = torch.empty(K + capacity, dtype=torch.int32, device=w.device)
        out[:K] = lens
        C.mask_rle_emit(w, index, FH, lens, ends, out, K)
        return out.cpu().numpy()                                           # the host read

    capacity = K * (4 * FW + 64)
    host = emit(capacity)
    n = host[:K].astype(np.int64)
    if int(n.sum()) > capacity:
        host = emit(int(n.sum()))
    stops = np.cumsum(n)
    return [{"size": [FH, FW], "counts": host[K + stops[k] - n[k]:K + stops[k]].tolist()} for k in range(K)]


@torch.no_grad()
def unpack_masks(packed, index=None) -> torch.Tensor:
    """bool (K,FH,FW) of the masks packed[index] (all, without index)."""
    w, index, FH, FW = _packed_args(packed, index, "the masks are unpacked")
    return _C().mask_unpack(w, index, FH)


@torch.no_grad()
def instance_map(packed, index=None) -> torch.Tensor:
    """The painter's picture of the masks packed[index] (all, without index), what the reference's show_anns
    (encoders/sam_encoder/segment.py:57-70) paints: int32 (FH,FW), per pixel the LARGEST j whose mask index[j] covers it - later
    masks paint over earlier ones -, -1 where none does.  Rows may repeat in index.  With index = paint_order(areas) the small
    masks lie on top, as in show_anns; the values are positions in `index`.  One launch, no host read; the map is a label map
    contrib.label_votes takes as it is."""
    w, index, FH, FW = _packed_args(packed, index, "the instance map is painted")
    return _C().mask_instance_map(w, index, FH)


def paint_order(areas) -> torch.Tensor:
    """The order show_anns paints in: sorted(range(K), key=area, reverse=True) - descending areas, equal areas in their
    former order (Python's sort is stable, with reverse too).  int64 (K,), on the device of `areas` if it is a tensor."""
    a = torch.as_tensor(areas)
    if a.dim() != 1 or a.dtype == torch.bool:
        raise ValueError(f"areas: K numbers expected, got {a.dtype} {tuple(a.shape)}")
    return torch.sort(a.detach(), descending=True, stable=True)[1]


# ---- small regions ----------------------------------------------------------------------------------------------------------
def _area(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)) or float(v) < 0:
        raise ValueError(f"{name} {v!r}: a finite number >= 0 expected")
    return float(v)


def _label(w, index, FH, FW, thresh, holes):
    """One labelling: (words, changed, area, box).  The run buffers are sized before the runs are known, at 4 FW + 64 per mask (a
    blob has about 2 per column, its background about 2 FW); the call's one host read brings the number back, and only masks
    that outgrow the provision cost a second call."""
    K = w.shape[0] if index is None else index.shape[0]
    capacity = K * (4 * FW + 64)
    *out, runs = _C().mask_regions(w, index, FH, thresh, holes, capacity)
    if runs > capacity:
        *out, runs = _C().mask_regions(w, index, FH, thresh, holes, runs)
    return out


@torch.no_grad()
def remove_small_regions(packed, area_thresh, mode, index=None):
    """utils/amg.py:remove_small_regions of the K masks packed[index] (all, without index) at once: (PackedMasks, changed (K,) bool).
    mode "holes": the 8-connected components of the BACKGROUND with area < area_thresh (strict; the outer background counts) are
    filled.  mode "islands": the foreground components with area < area_thresh are dropped - but where every one is small the
    largest stays, and changed is True all the same (one island below the threshold: the same bits, changed).  changed is False,
    and the bits are the input's, where no component is small.  Ties for the largest go to the component whose first pixel comes
    first in row-major order: this project's rule (scipy.ndimage.label's label order), not measured against OpenCV.  packed is
    only read.  One host read (the number of runs, with the kernels' error word), a second call and read only where the masks
    have more than 4 FW + 64 runs each."""
    thresh = _area(area_thresh, "area_thresh")
    if mode not in REGION_MODES:
        raise ValueError(f"mode {mode!r}: one of {', '.join(REGION_MODES)} expected")
    w, index, FH, FW = _packed_args(packed, index, "the regions are labelled")
    words, changed, _, _ = _label(w, index, FH, FW, thresh, mode == "holes")
    return PackedMasks(words, (FH, FW)), changed


@torch.no_grad()
def postprocess_small_regions(packed, min_area, index=None) -> SmallRegions:
    """What automatic_mask_generator.py:postprocess_small_regions does to every mask: holes, then islands on the result.
    SmallRegions(packed, changed (K,) bool = either pass changed, area (K,) int32 and box (K,4) int32 XYXY of the new masks in
    the full frame, [0,0,0,0] when empty - both from the launch that writes the words).  One host read per labelling: two."""
    thresh = _area(min_area, "min_area")
    w, index, FH, FW = _packed_args(packed, index, "the regions are labelled")
    filled, changed_h, _, _ = _label(w, index, FH, FW, thresh, True)
    words, changed_i, area, box = _label(filled, None, FH, FW, thresh, False)
    return SmallRegions(PackedMasks(words, (FH, FW)), changed_h | changed_i, area, box)


# ---- the assembled pipeline -------------------------------------------------------------------------------------------------
class MaskPostprocessor:
    """The records of SamAutomaticMaskGenerator.generate from the decoder's outputs:

        pp = MaskPostprocessor((orig_h, orig_w), pred_iou_thresh=0.88, stability_score_thresh=0.95)
        for points in batches:                                   # automatic_mask_generator.py:_process_batch
            _, iou_preds, low_res = predictor.predict_torch(..., return_logits=True)
            pp.add_batch(low_res, iou_preds, points, crop_box, predictor.input_size, predictor.original_size, 1024)
        records = pp.finish()

    add_batch runs the fused pass and the filter and keeps their device tensors: no host read.  finish() reads the kept lists
    once, runs the box NMS of every crop (scores iou_preds, box_nms_thresh; one read of the count per crop, as torchvision's has)
    and, with more than one crop, the NMS across crops (scores 1 / crop area, crop_nms_thresh), then reads the survivors' scalars
    once and their run lengths once.  With min_mask_region_area > 0 the survivors first go through postprocess_small_regions
    (two labellings, one host read each) and a second NMS at max(box_nms_thresh, crop_nms_thresh) on the new masks' boxes with
    score 1 for an unchanged mask and 0 for a changed one (this project's box_nms: stable, the lower row first among equal
    scores); a kept changed mask takes its new bits, box and area, and the records come out unchanged masks first, then the
    changed ones, each group in its former order.  Not built: coco_rle."""

    def __init__(self, frame_size, *, pred_iou_thresh=0.88, stability_score_thresh=0.95, stability_score_offset=1.0, box_nms_thresh=0.7,
                 crop_nms_thresh=0.7, mask_threshold=0.0, output_mode="uncompressed_rle", min_mask_region_area=0):
        self.frame_size = _pair(frame_size, "frame_size")
        if output_mode not in OUTPUT_MODES:
            raise ValueError(f"output_mode {output_mode!r}: one of {', '.join(OUTPUT_MODES)} expected (coco_rle needs pycocotools and is not built)")
        self.pred_iou_thresh = _number(pred_iou_thresh, "pred_iou_thresh")
        self.stability_score_thresh = _number(stability_score_thresh, "stability_score_thresh")
        self.stability_score_offset = _number(stability_score_offset, "stability_score_offset")
        self.box_nms_thresh = _number(box_nms_thresh, "box_nms_thresh")
        self.crop_nms_thresh = _number(crop_nms_thresh, "crop_nms_thresh")
        self.mask_threshold = _number(mask_threshold, "mask_threshold")
        self.output_mode = output_mode
        self.min_mask_region_area = _area(min_mask_region_area, "min_mask_region_area")
        self._batches = []

    def add_batch(self, low_res, iou_preds, points, crop_box, input_size, original_size, img_size):
        """low_res (B,C,h,w) or (M,h,w) logits and iou_preds (B,C) or (M,) as predict_torch returns them; points (B,2) - each
        stands for its C masks - or (M,2), in the crop's coordinates, a numpy array or tensor.  crop_box (x0,y0,x1,y1) or None."""
        if torch.is_tensor(low_res) and low_res.dim() == 4:
            per_point = low_res.shape[1]
            low_res = low_res.reshape(-1, *low_res.shape[2:])
        else:
            per_point = 1
        if torch.is_tensor(iou_preds) and iou_preds.dim() == 2:
            iou_preds = iou_preds.reshape(-1)
        pts = np.asarray(points.detach().cpu() if torch.is_tensor(points) else points, dtype=np.float64)
        M = _logits(low_res).shape[0]
        if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] * per_point != M:
            raise ValueError(f"points {pts.shape}: one (x, y) per prompt expected")
        if iou_preds is None:
            raise ValueError("iou_preds: needed (they are the NMS scores)")
        FH, FW = self.frame_size
        crop = (0, 0, FW, FH) if crop_box is None else tuple(int(v) for v in crop_box)
        st = mask_pass(low_res, img_size, input_size, original_size, mask_threshold=self.mask_threshold,
                       stability_offset=self.stability_score_offset, iou_preds=iou_preds, pred_iou_thresh=self.pred_iou_thresh,
                       crop_box=crop, frame_size=self.frame_size, stability_score_thresh=self.stability_score_thresh)
        self._batches.append((st, iou_preds.detach(), pts.repeat(per_point, axis=0), crop))

    def finish(self) -> list:
        batches, self._batches = self._batches, []
        if not batches:
            return []
        dev = batches[0][0].keep.device
        lists = torch.cat([torch.cat([st.kept_count, st.kept_index]) for st, _, _, _ in batches]).cpu().numpy()      # host read 1
        per_crop, at = {}, 0
        for b, (st, _, _, crop) in enumerate(batches):
            M = st.keep.shape[0]
            rows = lists[at + 1:at + 1 + lists[at]]
            at += 1 + M
            per_crop.setdefault(crop, []).extend((b, int(m)) for m in rows)
        offsets = np.cumsum([0] + [b[0].keep.shape[0] for b in batches])
        cat = lambda f: torch.cat([f(b) for b in batches])
        box, box_frame, iou = cat(lambda b: b[0].box), cat(lambda b: b[0].box_frame), cat(lambda b: b[1])
        survivors = []                                          # global rows, in the reference's order
        crop_of = []
        for crop, rows in per_crop.items():
            g = torch.as_tensor([offsets[b] + m for b, m in rows], dtype=torch.int64, device=dev)
            if len(rows):
                g = g[batched_nms(box[g], iou[g], torch.zeros(len(rows), dtype=torch.int32, device=dev), self.box_nms_thresh)]
            survivors.append(g)
            crop_of += [crop] * g.shape[0]
        g = torch.cat(survivors)
        if len(per_crop) > 1 and g.shape[0]:
            crops = torch.as_tensor(crop_of, dtype=torch.float32, device=dev)
            scores = 1 / ((crops[:, 2] - crops[:, 0]) * (crops[:, 3] - crops[:, 1]))
            keep = batched_nms(box_frame[g], scores, torch.zeros(g.shape[0], dtype=torch.int32, device=dev), self.crop_nms_thresh)
            g = g[keep]
            crop_of = [crop_of[i] for i in keep.tolist()]
        K = g.shape[0]
        if K == 0:
            return []
        stats = cat(lambda b: torch.cat([b[0].area[:, None].double(), b[0].stability[:, None].double()], 1))

        def gather(rows):
            which = np.searchsorted(offsets, rows, side="right") - 1
            words = torch.empty((len(rows),) + tuple(batches[0][0].packed.words.shape[1:]), dtype=torch.int32, device=dev)
            for b in np.unique(which):
                sel = np.nonzero(which == b)[0]
                words[torch.as_tensor(sel, device=dev)] = batches[b][0].packed.words[torch.as_tensor(rows[sel] - offsets[b], device=dev)]
            return words

        if self.min_mask_region_area > 0:
            # automatic_mask_generator.py:postprocess_small_regions, before any scalar or run length is read
            sr = postprocess_small_regions(PackedMasks(gather(g.cpu().numpy()), self.frame_size), self.min_mask_region_area)
            keep = batched_nms(sr.box, (~sr.changed).to(torch.float32), torch.zeros(K, dtype=torch.int32, device=dev),
                               max(self.box_nms_thresh, self.crop_nms_thresh))
            g, ch = g[keep], sr.changed[keep]
            crop_of = [crop_of[i] for i in keep.tolist()]
            K = g.shape[0]
            words = torch.where(ch[:, None, None], sr.packed.words[keep], gather(g.cpu().numpy()))
            new_box = torch.where(ch[:, None], sr.box[keep], box_frame[g]).double()
            new_stats = torch.cat([torch.where(ch, sr.area[keep], stats[g][:, 0].to(torch.int32))[:, None].double(), stats[g][:, 1:]], 1)
            table = torch.cat([new_box, iou[g][:, None].double(), new_stats], 1).cpu().numpy()                # host read of the scalars
            rows = g.cpu().numpy()
        else:
            table = torch.cat([box_frame[g].double(), iou[g][:, None].double(), stats[g]], 1).cpu().numpy()  # host read of the scalars
            rows = g.cpu().numpy()
            words = gather(rows)
        packed = PackedMasks(words, self.frame_size)
        if self.output_mode == "binary_mask":
            seg = list(unpack_masks(packed).cpu().numpy())
        else:
            seg = masks_to_rle(packed)                                                  # host read of the run lengths
        points = np.concatenate([b[2] for b in batches])
        records = []
        for k in range(K):
            x0, y0, x1, y1 = (int(v) for v in table[k, :4])
            c = crop_of[k]
            records.append({"segmentation": seg[k], "area": int(table[k, 5]), "bbox": [x0, y0, x1 - x0, y1 - y0],
                            "predicted_iou": float(np.float32(table[k, 4])),
                            "point_coords": [[float(points[rows[k], 0] + c[0]), float(points[rows[k], 1] + c[1])]],
                            "stability_score": float(np.float32(table[k, 6])), "crop_box": [c[0], c[1], c[2] - c[0], c[3] - c[1]]})
        return records
