"""Instances across views: from per-view SAM masks to 3D instance labels of the Gaussians.

SAM numbers its masks afresh in every view: mask 3 of one view and mask 17 of the next may be the same chair.  The label vote
(contrib.label_votes) lifts ONE view's instance map to the Gaussians; this module carries the ids over from view to view
(csrc/instances.hip behind include/f3dgs.h: f3dgs_instance_associate, f3dgs_instance_merge):

    overlap   how much of each view mask's weight lies on each 3D instance built so far, from the view's vote (P, M + 1) and the
              global accumulator (P, L + 1): a small (M + 1, L + 1) table, one float atomic per non-zero of the vote
    match     IoU of mask and instance on that table; a mask claims its best instance at IoU >= iou_thresh, an instance takes
              its best claimant; every other mask of weight > min_weight opens a new instance while slots remain
    merge     the view's columns are added into the global accumulator under that mapping

    lifter = InstanceLifter(P, max_instances=512, max_masks=255, device=device)
    for cam in cameras:
        packed = post(low_res_of(cam), ...)["packed"]                     # sam_masks.MaskPostprocessor
        out = lifter.add_view(cam, gaussians, pipe, bg, sam_masks.instance_map(packed))
        picture = seg_metrics.colorize(out["global_map"], palette)        # the view's masks in global ids
    edit.apply_edit(opacity, shs, lifter.select(instance), {"deletion": True})

HIP only; no CPU fallback.  Nothing is read back to the host but by num_instances().
"""
from __future__ import annotations

import math

import torch

import contrib
from contrib import LabelLifter, render_label_votes
from diff_gaussian_rasterization import _C

MAX_MASKS = 1024         # F3DGS_INSTANCE_MAX_MASKS: masks of one view
MAX_INSTANCES = 4096     # F3DGS_INSTANCE_MAX_INSTANCES: 3D instance slots


def _describe(t):
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__


def _check_pair(acc_view, acc):
    """acc_view (P, M + 1) and acc (P, L + 1) under the rules of contrib._check_votes; returns (P, M, L, device)."""
    for t, name, n in ((acc_view, "acc_view", "M"), (acc, "acc", "L")):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] < 2:
            raise ValueError(f"{name}: a contiguous float32 (P, {n} + 1) tensor with {n} >= 1 expected, got {_describe(t)}")
    P, M, L = acc_view.shape[0], acc_view.shape[1] - 1, acc.shape[1] - 1
    if M > MAX_MASKS:
        raise ValueError(f"acc_view {tuple(acc_view.shape)}: M = {M} masks, 1 .. {MAX_MASKS} are taken")
    if L > MAX_INSTANCES:
        raise ValueError(f"acc {tuple(acc.shape)}: L = {L} instances, 1 .. {MAX_INSTANCES} are taken")
    dev = acc_view.device
    try:
        contrib._check_votes(acc_view, P, M, dev)
    except ValueError as e:
        raise ValueError(f"acc_view: {e}") from None
    contrib._check_votes(acc, P, L, dev)
    return P, M, L, dev


def _check_counter(t, name, dev):
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != 1 or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{name} must be one int32 on {dev} (it is updated on the device), got {_describe(t)}")


def _check_thresholds(iou_thresh, min_weight):
    for v, name in ((iou_thresh, "iou_thresh"), (min_weight, "min_weight")):
        if not isinstance(v, (int, float)) or math.isnan(v) or v < 0:
            raise ValueError(f"{name} = {v!r}: a number >= 0 expected")


def associate_votes(acc_view, acc, count, *, iou_thresh=0.5, min_weight=0.0, dropped=None) -> dict:
    """Matches the M masks of one view's vote with the 3D instances of the accumulator (include/f3dgs.h:
    f3dgs_instance_associate).

    acc_view: (P, M + 1) float32, what label_votes wrote for this view with num_classes = M.  acc: (P, L + 1) float32, the global
    accumulator (LabelLifter's layout).  count: one int32 on the device, the instances in use; UPDATED.  dropped: one int32 on
    the device, INCREASED by the masks that found no free slot (a fresh zero when not given).  Neither acc_view nor acc is
    changed.  Returns mapping (M) int32 - the global id of every mask, -1: none -, best_label (M) int32, best_iou (M) float64,
    table (M + 1, L + 1) float32 and dropped."""
    _check_thresholds(iou_thresh, min_weight)
    _, _, _, dev = _check_pair(acc_view, acc)
    _check_counter(count, "count", dev)
    if dropped is None:
        dropped = torch.zeros(1, device=dev, dtype=torch.int32)
    _check_counter(dropped, "dropped", dev)
    with torch.no_grad():
        mapping, best_label, best_iou, table = _C.instance_associate(acc_view.detach(), acc.detach(), count, dropped, float(iou_thresh),
                                                                     float(min_weight))
    return {"mapping": mapping, "best_label": best_label, "best_iou": best_iou, "table": table, "dropped": dropped}


def merge_votes(acc_view, mapping, acc, *, clear_view=False):
    """acc[g][mapping[m]] += acc_view[g][m] and acc[g][L] += acc_view[g][M] for the Gaussians seen in the view (include/f3dgs.h:
    f3dgs_instance_merge).  mapping: (M) int32 on the device, entries outside [0, L) are ignored, repeated targets add up.
    clear_view: acc_view is written back as zeros where it was read as non-zero.  Returns acc."""
    _, M, _, dev = _check_pair(acc_view, acc)
    if not torch.is_tensor(mapping) or mapping.dtype != torch.int32 or tuple(mapping.shape) != (M,) or not mapping.is_contiguous() \
            or mapping.device != dev:
        raise ValueError(f"mapping must be a contiguous int32 ({M},) tensor on {dev}, got {_describe(mapping)}")
    with torch.no_grad():
        _C.instance_merge(acc_view, mapping, acc, bool(clear_view))
    return acc


class InstanceLifter(LabelLifter):
    """Labels the P Gaussians with 3D instance ids from per-view instance maps (sam_masks.instance_map) whose ids are NOT
    consistent between views: per view one label vote into a reusable (P, max_masks + 1) buffer, the association of its masks
    with the instances so far, and the merge into LabelLifter's accumulator (acc, (P, max_instances + 1)).  labels, confidence,
    ratios, select, label_image and seen are LabelLifter's, over the global ids."""

    def __init__(self, P: int, max_instances: int, max_masks: int, device, iou_thresh: float = 0.5, min_weight: float = 0.0):
        if not 1 <= int(max_instances) <= MAX_INSTANCES or not 1 <= int(max_masks) <= MAX_MASKS:
            raise ValueError(f"InstanceLifter(max_instances={max_instances}, max_masks={max_masks}): 1 <= max_instances <= "
                             f"{MAX_INSTANCES} and 1 <= max_masks <= {MAX_MASKS} expected")
        _check_thresholds(iou_thresh, min_weight)
        super().__init__(P, int(max_instances), device)
        dev = self.acc.device
        self.max_masks = int(max_masks)
        self.iou_thresh, self.min_weight = float(iou_thresh), float(min_weight)
        self.view = torch.zeros(self.P, self.max_masks + 1, device=dev, dtype=torch.float32)      # all zero between the views
        self.count = torch.zeros(1, device=dev, dtype=torch.int32)
        self.dropped = torch.zeros(1, device=dev, dtype=torch.int32)

    def add_view(self, viewpoint_camera, pc, pipe, bg_color, instance_map, scaling_modifier=1.0, override_color=None) -> dict:
        """Accumulates one view's (H, W) instance map (uint8 / int32 / int64; an id outside [0, max_masks) belongs to no mask,
        as for the label vote).  Returns the view's render dictionary (acc: the global accumulator) plus mapping, best_label,
        best_iou, table and global_map: mapping[instance_map] as int64, -1 where the pixel has no mask or its mask no instance."""
        M = self.max_masks
        out = render_label_votes(viewpoint_camera, pc, pipe, bg_color, instance_map, M, acc=self.view,
                                 scaling_modifier=scaling_modifier, override_color=override_color)
        res = associate_votes(self.view, self.acc, self.count, iou_thresh=self.iou_thresh, min_weight=self.min_weight,
                              dropped=self.dropped)
        merge_votes(self.view, res["mapping"], self.acc, clear_view=True)
        ids = instance_map.long()
        valid = (ids >= 0) & (ids < M)
        global_map = torch.where(valid, res["mapping"].long()[ids.clamp(0, M - 1)], torch.full((), -1, dtype=torch.int64, device=ids.device))
        self.views += 1
        out.update(acc=self.acc, mapping=res["mapping"], best_label=res["best_label"], best_iou=res["best_iou"], table=res["table"],
                   global_map=global_map)
        return out

    def num_instances(self) -> int:
        """The instances in use (the one host read of this class)."""
        return int(self.count.item())

    def num_dropped(self) -> int:
        """The masks, over all views, that found no free instance slot (a host read)."""
        return int(self.dropped.item())


__all__ = ["MAX_MASKS", "MAX_INSTANCES", "associate_votes", "merge_votes", "InstanceLifter"]
