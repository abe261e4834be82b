"""Per-group statistics of the Gaussians, and what follows from them: one decision per instance, and the merge of instances.

LabelLifter, InstanceLifter, neighbors.mode_filter and neighbors.components / split_labels end in one integer per Gaussian.  This
module says something about a group as a whole (csrc/group_stats.hip behind include/f3dgs.h: f3dgs_group_stats, f3dgs_group_merge):

    group_stats      per id: the number of members, their mass, centroid, covariance and box, and their mean semantic feature -
                     every sum in fp64 on the device, no (P, C) temporary, nothing copied to the host
    lifter_stats     the same over a LabelLifter's / InstanceLifter's labels()
    select_groups    edit.selection_mask on the (G, C) table of mean features: one decision per group instead of one per
                     Gaussian, under the reference's calculate_selection_score[_delete] contract; the mask apply_edit takes
    merge_similar    unites groups that touch in the neighbour lists and whose mean features agree (over-segmentation after the
                     association of instances across views)

    idx, dist2 = neighbors.knn(xyz, 8)
    st = groups.lifter_stats(instance_lifter, xyz, features=gaussians.get_semantic_feature)
    merged = groups.merge_similar(instance_lifter.labels(), idx, st.feature_mean, min_cos=0.95)
    st = groups.group_stats(merged.groups, xyz, instance_lifter.L, features=gaussians.get_semantic_feature)
    group_mask, mask = groups.select_groups(merged.groups, st.feature_mean, text_features)

HIP only; no CPU fallback.  Nothing is read back to the host.
"""
from __future__ import annotations

import collections
import math

import torch

from simple_knn import _C
from neighbors import _check_lists, _describe, _max_dist2, _need_device

MAX_GROUPS = 65536           # F3DGS_GROUP_MAX_GROUPS
MAX_CHANNELS = 4096          # F3DGS_GROUP_MAX_CHANNELS
MERGE_MAX_GROUPS = 4096      # F3DGS_GROUP_MERGE_MAX_GROUPS

GroupStats = collections.namedtuple("GroupStats", ["count", "mass", "centroid", "cov", "aabb_min", "aabb_max", "feature_mean"])
MergedGroups = collections.namedtuple("MergedGroups", ["groups", "group_root", "status"])


def _group_ids(groups, num_groups, limit, name="groups"):
    """(ids as the kernels take them - int32, contiguous, anything outside int32 as -1 -, number of groups)"""
    _need_device(groups, name)
    if groups.dim() != 1 or groups.dtype not in (torch.int32, torch.int64, torch.bool):
        raise ValueError(f"{name}: an int32, int64 or bool (P,) tensor expected, got {_describe(groups)}")
    if groups.dtype == torch.bool:
        if num_groups not in (None, 1):
            raise ValueError(f"num_groups = {num_groups!r}: a bool mask is one group (selected = group 0)")
        return groups.to(torch.int32) - 1, 1
    if not isinstance(num_groups, int) or isinstance(num_groups, bool) or not 1 <= num_groups <= limit:
        raise ValueError(f"num_groups = {num_groups!r}: an integer in 1 .. {limit} expected")
    g = groups.detach()
    if g.dtype == torch.int64:
        g = torch.where((g >= 0) & (g < num_groups), g, torch.full((), -1, dtype=torch.int64, device=g.device)).to(torch.int32)
    return g.contiguous(), num_groups


def group_stats(groups, xyz, num_groups=None, weight=None, features=None, cov=True):
    """Statistics of the Gaussians per group.  groups: (P,) int32 or int64 on the device - any integers, an id outside
    [0, num_groups) belongs to no group - or a bool `mask` of edit.apply_edit (selected = group 0, num_groups = 1).  xyz: (P, 3)
    float32.  weight: (P,) float32 or None (1 each).  features: (P, C) or the model's (P, 1, C) float32, or None; a strided view
    is read in place.

    Gaussian i is a member of groups[i] iff the id is in range, its coordinates are finite and 0 < weight[i] < inf.  Returns
    GroupStats(count (G,) int64, mass (G,), centroid (G, 3), cov (G, 3, 3) symmetric or None with cov=False (no second pass),
    aabb_min (G, 3), aabb_max (G, 3), feature_mean (G, C) or None without features), float32: sum w, sum w x / mass, the
    population covariance sum w (x - c)(x - c)^T / mass about the fp64 centroid, the exact box of the members, sum w f / mass.
    Every sum is accumulated in fp64 and rounded once.  An empty group: zeros, and the box (+inf, -inf).  count and the box are
    exact; the float sums meet in a varying order and may differ in the last bit between two calls."""
    g32, G = _group_ids(groups, num_groups, MAX_GROUPS)
    P, dev = g32.shape[0], g32.device
    if not torch.is_tensor(xyz) or xyz.dtype != torch.float32 or tuple(xyz.shape) != (P, 3) or xyz.device != dev:
        raise ValueError(f"xyz: a float32 ({P}, 3) tensor on {dev} expected, got {_describe(xyz)}")
    if weight is not None and (not torch.is_tensor(weight) or weight.dtype != torch.float32 or tuple(weight.shape) != (P,)
                               or weight.device != dev):
        raise ValueError(f"weight: a float32 ({P},) tensor on {dev} or None expected, got {_describe(weight)}")
    f2 = None
    if features is not None:
        f2 = features
        if torch.is_tensor(f2) and f2.dim() == 3 and f2.shape[1] == 1:
            f2 = f2[:, 0, :]
        if not torch.is_tensor(f2) or f2.dtype != torch.float32 or f2.dim() != 2 or f2.shape[0] != P or f2.device != dev \
                or not 1 <= f2.shape[1] <= MAX_CHANNELS:
            raise ValueError(f"features: a float32 ({P}, C) or ({P}, 1, C) tensor on {dev} with 1 <= C <= {MAX_CHANNELS} expected, got "
                             f"{_describe(features)}")
        f2 = f2.detach()
        if (f2.shape[1] > 1 and f2.stride(1) != 1) or (P > 1 and f2.stride(0) < f2.shape[1]):
            f2 = f2.contiguous()                      # (a transposed or expanded view: the kernel reads rows)
    want = _C.GROUP_COUNT | _C.GROUP_MASS | _C.GROUP_CENTROID | _C.GROUP_AABB | (_C.GROUP_COV if cov else 0) | \
        (_C.GROUP_FEATURE_MEAN if f2 is not None else 0)
    with torch.no_grad():
        count, mass, centroid, cov6, aabb, fm = _C.group_stats(g32, xyz.detach().contiguous(), G,
                                                               None if weight is None else weight.detach().contiguous(), f2, want)
        cov33 = None if cov6 is None else torch.stack([cov6[:, k] for k in (0, 1, 2, 1, 3, 4, 2, 4, 5)], dim=1).reshape(G, 3, 3)
    return GroupStats(count.long(), mass, centroid, cov33, aabb[:, :3], aabb[:, 3:], fm)


def _check_lifter(lifter):
    for name in ("labels", "confidence", "seen"):
        if not callable(getattr(lifter, name, None)):
            raise ValueError(f"lifter: an object with labels(), confidence() and seen() expected (LabelLifter, InstanceLifter), "
                             f"got {type(lifter).__name__}")
    if not isinstance(getattr(lifter, "L", None), int):
        raise ValueError(f"lifter: no class count L (LabelLifter, InstanceLifter expected), got {type(lifter).__name__}")


def lifter_labels(lifter, min_weight=0.0):
    """lifter.labels() with the Gaussians that are not lifter.seen(min_weight) as -1 (as neighbors.smooth_labels takes them)"""
    _check_lifter(lifter)
    labels = lifter.labels()
    return torch.where(lifter.seen(min_weight), labels, torch.full((), -1, dtype=labels.dtype, device=labels.device))


def lifter_stats(lifter, xyz, features=None, weight=None, min_weight=0.0, cov=True):
    """group_stats over a contrib.LabelLifter's or an instances.InstanceLifter's labels(): one group per class, or per global
    instance id (num_groups = the lifter's class count, or max_instances).  The Gaussians that are not lifter.seen(min_weight)
    belong to no group."""
    return group_stats(lifter_labels(lifter, min_weight), xyz, lifter.L, weight=weight, features=features, cov=cov)


def select_groups(groups, feature_mean, text_features, score_threshold=None, positive_ids=(0,), variant="select"):
    """One decision per group: edit.selection_mask, unchanged, on the (G, C) table of mean features - the reference's
    calculate_selection_score (variant "select") or calculate_selection_score_delete ("delete") with a group's mean feature in
    the place of a Gaussian's.  Returns (group_mask (G,) bool, mask (P,) bool): mask[i] = group_mask[groups[i]], False for an id
    outside [0, G) - what edit.apply_edit takes.  An empty group (a zero mean) decides as the kernel decides a zero row; nobody
    carries its id."""
    import edit
    _need_device(groups, "groups")
    if groups.dim() != 1 or groups.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"groups: an int32 or int64 (P,) tensor expected, got {_describe(groups)}")
    if not torch.is_tensor(feature_mean) or feature_mean.dtype != torch.float32 or feature_mean.dim() != 2 \
            or feature_mean.device != groups.device:
        raise ValueError(f"feature_mean: a float32 (G, C) tensor on {groups.device} expected (group_stats' feature_mean), got "
                         f"{_describe(feature_mean)}")
    G = feature_mean.shape[0]
    with torch.no_grad():
        group_mask = edit.selection_mask(feature_mean, text_features, score_threshold=score_threshold, positive_ids=positive_ids,
                                         variant=variant) >= 0.5
        g = groups.detach().long()
        inside = (g >= 0) & (g < G)
        mask = inside & group_mask[g.clamp(0, max(G - 1, 0))] if G else torch.zeros_like(inside)
    return group_mask, mask


def merge_similar(groups, idx, feature_mean, min_cos, dist2=None, max_dist=None, mutual=False):
    """Unites the groups that are adjacent in the neighbour lists and whose mean features agree.  groups: (P,) int32 or int64 ids
    (an id outside [0, G) belongs to no group and comes back as -1).  idx (P, K) int32, dist2 (P, K) float32: neighbors.knn's lists.
    feature_mean: (G, C) float32, group_stats' (G <= 4096).

    Groups a != b are adjacent iff a Gaussian of a has a Gaussian of b in its list (within max_dist, if given; with mutual=True
    each must hold the other).  Adjacent groups are united iff the cosine of their mean features, in fp64, is >= min_cos; a zero
    or NaN mean unites with nobody.  Returns MergedGroups(groups (P,) int64: every id replaced by the smallest id of its merged
    set, group_root (G,) int64: that id per group - a group without members is its own root -, status: a 0-dim device tensor, 0)."""
    _need_device(groups, "groups")
    if groups.dim() != 1 or groups.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"groups: an int32 or int64 (P,) tensor expected, got {_describe(groups)}")
    P, dev = groups.shape[0], groups.device
    _check_lists(idx, dist2, P, dev)
    if not torch.is_tensor(feature_mean) or feature_mean.dtype != torch.float32 or feature_mean.dim() != 2 or feature_mean.device != dev \
            or not 1 <= feature_mean.shape[0] <= MERGE_MAX_GROUPS or not 1 <= feature_mean.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"feature_mean: a float32 (G, C) tensor on {dev} with 1 <= G <= {MERGE_MAX_GROUPS} and 1 <= C <= {MAX_CHANNELS} "
                         f"expected, got {_describe(feature_mean)}")
    if isinstance(min_cos, bool) or not isinstance(min_cos, (int, float)) or math.isnan(min_cos):
        raise ValueError(f"min_cos = {min_cos!r}: a number expected")
    limit2 = _max_dist2(max_dist, dist2)
    d2 = None if (dist2 is None or math.isinf(limit2)) else dist2.detach().contiguous()
    g32, _ = _group_ids(groups, feature_mean.shape[0], MERGE_MAX_GROUPS)
    with torch.no_grad():
        out, root, status = _C.group_merge(g32, idx.contiguous(), d2, limit2, bool(mutual), feature_mean.detach().contiguous(),
                                           float(min_cos), None)
    return MergedGroups(out.long(), root.long(), status.long())


__all__ = ["MAX_GROUPS", "MAX_CHANNELS", "MERGE_MAX_GROUPS", "GroupStats", "MergedGroups", "group_stats", "lifter_labels", "lifter_stats",
           "select_groups", "merge_similar"]
