"""Open-vocabulary segmentation of a rendered feature map: which of K text embeddings every pixel of a view matches.

The reference spreads the chain over two scripts.  render.py:168-180 resizes the rendered (C, H, W) map to the teacher's
size (bilinear, align_corners=True), runs the 1x1 `CNN_decoder` (C -> Cout) and stores the result as fp16;
encoders/lseg_encoder/segmentation.py:526-540 reloads it, L2-normalises every pixel's Cout-vector and every text embedding,
forms the (Hs Ws, Cout) @ (Cout, K) logits and takes `torch.max(..., 1)[1]`.  Here that is ONE call (csrc/segment.hip behind
include/f3dgs.h: f3dgs_segment): neither the decoded (Cout, Hs, Ws) map - 354 MB at 360 x 480 x 512 - nor the logits ever
exist in memory, and the fp16 store, which decides labels, is reproduced (`half=True`), not improved on.

    labels = segment(render_pkg["feature_map"], text_features, size=gt_feature_map.shape[1:],
                     weight=cnn_decoder.conv.weight, bias=cnn_decoder.conv.bias)

HIP only; no CPU fallback.  The call reads nothing back to the host: it may be captured in a graph.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _C
from feature_loss import fused_feature_decode

MAX_TEXTS = 256                 # F3DGS_SEGMENT_MAX_TEXTS
DECODER_WIDTHS = (32, 64, 128)  # the fused decoder's input widths (fused_feature_decode's own limit)


def _check(feature_map, text_features, size, weight, bias):
    """Argument errors, raised before any device work.  Returns (Hs, Ws, weight as (Cout, C) or None)."""
    if feature_map.dim() != 3 or text_features.dim() != 2:
        raise ValueError(f"feature_map (C, H, W) and text_features (K, Cout) expected, got {tuple(feature_map.shape)} and "
                         f"{tuple(text_features.shape)}")
    if feature_map.dtype != torch.float32 or text_features.dtype != torch.float32:
        raise ValueError(f"feature_map and text_features must be float32, got {feature_map.dtype} and {text_features.dtype}")
    C, H, W = feature_map.shape
    if C < 1 or H < 1 or W < 1:
        raise ValueError(f"empty feature_map {tuple(feature_map.shape)}")
    K, Ct = text_features.shape
    if K < 1 or K > MAX_TEXTS:
        raise ValueError(f"{K} text embeddings: 1 to {MAX_TEXTS} are supported")
    if size is None:
        Hs, Ws = H, W
    else:
        if len(size) != 2:
            raise ValueError(f"size {tuple(size)}: (Hs, Ws) expected")
        Hs, Ws = int(size[0]), int(size[1])
        if Hs < 0 or Ws < 0:
            raise ValueError(f"size {(Hs, Ws)}: negative")
    w2 = None
    Cout = C
    if weight is None:
        if bias is not None:
            raise ValueError("bias without weight")
    else:
        if not (weight.dim() == 2 or (weight.dim() == 4 and weight.shape[2:] == (1, 1))) or weight.shape[1] != C:
            raise ValueError(f"weight (Cout, {C}) or (Cout, {C}, 1, 1) expected, got {tuple(weight.shape)}")
        Cout = weight.shape[0]
        if bias is not None and tuple(bias.shape) != (Cout,):
            raise ValueError(f"bias ({Cout},) expected, got {tuple(bias.shape)}")
        if weight.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
            raise ValueError("weight and bias must be float32")
        if C not in DECODER_WIDTHS or Cout % 32 != 0:
            raise ValueError(f"decoder {C} -> {Cout}: supported are input widths {DECODER_WIDTHS} and outputs that are multiples "
                             f"of 32")
        w2 = weight.reshape(Cout, C)
    if Ct != Cout:
        raise ValueError(f"text_features has {Ct} channels, the scored map has {Cout}")
    return Hs, Ws, w2


@torch.no_grad()
def segment(feature_map: torch.Tensor, text_features: torch.Tensor, size=None, weight: Optional[torch.Tensor] = None,
            bias: Optional[torch.Tensor] = None, half: bool = True, text_normalized: bool = False, return_score: bool = False):
    """labels (Hs, Ws) int64: argmax_k of the cosine between pixel (y, x) of decode(resize(feature_map)) and text_features[k].

    feature_map (C, H, W) float32 on the GPU; text_features (K, Cout) float32, 1 <= K <= 256, never modified; size (Hs, Ws)
    or None for the map's own size (which also serves an already decoded map: no resize, no decoder); weight (Cout, C) or
    (Cout, C, 1, 1) and bias (Cout) of the 1x1 decoder (C in 32, 64, 128; Cout a multiple of 32), or None for no decoder
    (then Cout == C, any C).  half=True rounds the decoded values to fp16 first, as render.py stores the map.
    text_normalized=True: the rows of text_features are already t / ||t||.  return_score=True: also the winning cosine,
    (Hs, Ws) float32.  As torch.max: NaN counts as the maximum and the lowest index wins a tie, so a pixel of zero norm or
    with a non-finite value gets label 0 and score NaN."""
    Hs, Ws, w2 = _check(feature_map, text_features, size, weight, bias)
    flags = (_C.SEGMENT_ROUND_HALF if half else 0) | (_C.SEGMENT_TEXT_NORMALIZED if text_normalized else 0)
    e = torch.Tensor([])
    if w2 is None:
        labels, score = _C.segment(feature_map, text_features, Hs, Ws, e, e, flags, bool(return_score))
    else:
        b = bias if bias is not None else torch.zeros(w2.shape[0], device=w2.device, dtype=w2.dtype)
        labels, score = _C.segment(feature_map, text_features, Hs, Ws, w2, b, flags, bool(return_score))
    return (labels, score) if return_score else labels


@torch.no_grad()
def segment_reference_chain(feature_map: torch.Tensor, text_features: torch.Tensor, gt_size, weight: Optional[torch.Tensor] = None,
                            bias: Optional[torch.Tensor] = None, seg_size=(360, 480)) -> torch.Tensor:
    """The reference's two scripts end to end: render.py:168-180 stores the map at the teacher's size `gt_size` as fp16, and
    segmentation.py:501-521 resizes the stored map a second time, to `seg_size`, when it is wider than seg_size[1].  That
    case is composed here (fused_feature_decode(half=True), F.interpolate, segment() without a decoder: the second resize is
    not fused); otherwise it is one segment() call.  Returns the labels, (gt_size) or (seg_size) int64."""
    gt_size = (int(gt_size[0]), int(gt_size[1]))
    if gt_size[1] > int(seg_size[1]):
        _check(feature_map, text_features, gt_size, weight, bias)
        stored = fused_feature_decode(feature_map, gt_size, weight, bias, half=True)
        again = F.interpolate(stored.to(torch.float32)[None], size=(int(seg_size[0]), int(seg_size[1])), mode="bilinear",
                              align_corners=True)[0]
        return segment(again, text_features, half=False)
    return segment(feature_map, text_features, size=gt_size, weight=weight, bias=bias, half=True)


def label_agreement(teacher: torch.Tensor, student: torch.Tensor, num_classes: int):
    """(accuracy, mean IoU) of two label maps as encoders/lseg_encoder/segmentation_metric.py:58-61, 76-90 compute them:
    the share of equal pixels, and the NaN-mean of intersection / union over the `num_classes` most frequent labels of the
    concatenation of both maps.  Plain torch on the labels' device; returns two Python floats.
    (seg_metrics.py scores whole test sets with HIP kernels and one host read, by the same rule for equal counts.)"""
    if teacher.shape != student.shape:
        raise ValueError(f"label maps of shapes {tuple(teacher.shape)} and {tuple(student.shape)}")
    if teacher.numel() == 0:
        raise ValueError("empty label maps")
    t, s = teacher.reshape(-1).to(torch.int64), student.reshape(-1).to(torch.int64)
    if int(torch.minimum(t.min(), s.min())) < 0:
        raise ValueError("negative label")
    accuracy = float((t == s).to(torch.float64).mean())
    counts = torch.bincount(torch.cat((t, s)))
    order = torch.sort(counts, descending=True, stable=True).indices          # equal counts: the lower label first
    order = order[counts[order] > 0][:int(num_classes)]
    ious = []
    for i in order.tolist():
        a, b = t == i, s == i
        ious.append(float((a & b).sum()) / float((a | b).sum()))
    iou = torch.tensor(ious, dtype=torch.float64)
    return accuracy, float(torch.nanmean(iou)) if iou.numel() else float("nan")
