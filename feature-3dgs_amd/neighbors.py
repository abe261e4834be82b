"""Neighbourhoods of the Gaussians in 3D: K-nearest-neighbour lists with indices, a mode filter of per-Gaussian labels, connected
components over the lists, and the two density tests: radius counts and statistical outlier removal.

LabelLifter, InstanceLifter and edit.selection_mask decide every Gaussian from 2D evidence alone.  This module looks at a
Gaussian's neighbours (csrc/neighbors.hip behind include/f3dgs.h: f3dgs_knn_neighbors, f3dgs_label_mode_filter):

    knn              the K nearest neighbours of every point, indices and squared distances, exact: row i holds the K points
                     j != i with the smallest (dist2, j) in lexicographic order - a function of the inputs alone
    mode_filter      every Gaussian takes the label with the largest weight among itself and its K neighbours (Jacobi steps:
                     each iteration reads the previous labels only), one launch per iteration
    smooth_labels    mode_filter over a LabelLifter's / InstanceLifter's labels(), weighted with confidence()
    clean_selection  the same filter on a boolean `mask` of edit.apply_edit: drops isolated selected Gaussians, fills pinholes

A vote is local.  The lists as a GRAPH (csrc/components.hip: f3dgs_knn_components, f3dgs_component_filter) answer what comes after
a selection exists:

    components       the connected components over the lists: per Gaussian the smallest index and the size of its component,
                     on request dense ids; edges join equal labels only, within max_dist, on request mutual neighbours only
    drop_small       labels or a bool mask without the connected parts below min_size Gaussians (the floaters)
    keep_largest     of every label only its largest connected part
    split_labels     every connected part of a label an id of its own: one instance id with two bodies becomes two ids

    idx, dist2 = neighbors.knn(gaussians.get_xyz.detach(), 8)
    labels = neighbors.smooth_labels(lifter, gaussians.get_xyz.detach(), k=8, iterations=2)
    mask = neighbors.clean_selection(lifter.select(cls), idx)
    mask = neighbors.keep_largest(mask, idx)
    ids = neighbors.split_labels(instance_lifter.labels(), idx, dist2=dist2, max_dist=0.1).comp

A component filter removes a floater only where it is a component of its own.  One that hangs on its object by a thin bridge, or
a sparse halo around a dense body, is one component with the body; the two DENSITY tests catch both (csrc/outliers.hip:
f3dgs_radius_count, f3dgs_knn_outliers):

    radius_count                 per point the number of other points within a radius (of the same label), exact, on request
                                 saturated at a cap; no lists: a fixed-radius walk of the search's leaves
    outlier_scores               per point the mean distance to its list's neighbours, per group the mean and the standard
                                 deviation of that score, and keep = score <= mean + ratio * std
    remove_statistical_outliers  labels, a bool mask or nothing in, the same without the statistical outliers out
    remove_radius_outliers       the same with "fewer than min_neighbors points within radius"

    keep = neighbors.remove_statistical_outliers(None, gaussians.get_xyz.detach(), k=8, ratio=2.0)
    densify.prune_points(model, ~keep)
    mask = neighbors.remove_radius_outliers(mask, gaussians.get_xyz.detach(), radius=0.05, min_neighbors=4)

HIP only; no CPU fallback.  Nothing is read back to the host.
"""
from __future__ import annotations

import collections
import math

import torch

from simple_knn import _C

MAX_NEIGHBORS = 16       # F3DGS_KNN_MAX_NEIGHBORS


def _describe(t):
    return f"{t.dtype} {tuple(t.shape)} on {t.device}" if torch.is_tensor(t) else type(t).__name__


def _need_device(t, name):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise ValueError(f"{name} must live on a HIP device (got {_describe(t)}): the neighbourhood kernels have no CPU path")


def knn(points, k, return_dist2=True):
    """The k nearest neighbours of every point.  points: (P, 3) float32 on the device.  1 <= k <= 16.
    Returns idx (P, k) int32 and dist2 (P, k) float32 (None with return_dist2=False).  Row i: the k points j != i with the smallest
    (dist2, j), ascending - among equal distances the lower index first; a duplicate of point i is its neighbour at distance 0.
    Every distance is ((dx*dx) + (dy*dy)) + (dz*dz) in float32, one rounding per operation.  Missing neighbours (P - 1 < k) hold
    idx -1 and dist2 FLT_MAX.  A point with a NaN or infinite coordinate is nobody's neighbour and has none."""
    _need_device(points, "points")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points: a float32 (P, 3) tensor expected, got {_describe(points)}")
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_NEIGHBORS:
        raise ValueError(f"k = {k!r}: an integer in 1 .. {MAX_NEIGHBORS} expected")
    with torch.no_grad():
        idx, dist2 = _C.knn_neighbors(points.detach(), k, bool(return_dist2))
    return idx, (dist2 if return_dist2 else None)


def _check_lists(idx, dist2, P, dev):
    if not torch.is_tensor(idx) or idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != P \
            or not 1 <= idx.shape[1] <= MAX_NEIGHBORS or idx.device != dev:
        raise ValueError(f"idx: an int32 ({P}, K) tensor on {dev} with 1 <= K <= {MAX_NEIGHBORS} expected (knn's result), "
                         f"got {_describe(idx)}")
    if dist2 is not None and (not torch.is_tensor(dist2) or dist2.dtype != torch.float32 or dist2.shape != idx.shape
                              or dist2.device != dev):
        raise ValueError(f"dist2: a float32 {tuple(idx.shape)} tensor on {dev} expected, got {_describe(dist2)}")


def _max_dist2(max_dist, dist2):
    """max_dist squared in float32 (the kernel compares float32 with float32); None is +inf"""
    if max_dist is None:
        return math.inf
    if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float)) or math.isnan(max_dist) or max_dist < 0:
        raise ValueError(f"max_dist = {max_dist!r}: a number >= 0 or None expected")
    if math.isinf(max_dist):
        return math.inf
    if dist2 is None:
        raise ValueError("a finite max_dist needs dist2, the squared distances of knn")
    r = torch.tensor(float(max_dist), dtype=torch.float32)
    return float(r * r)


def mode_filter(labels, idx, weight=None, dist2=None, max_dist=None, iterations=1, fill=True, return_share=False):
    """The mode filter over neighbour lists.  labels: (P,) int32 or int64 on the device, negative = unlabelled, a label is any
    value up to 2^31 - 1.  idx (P, K) int32 and dist2 (P, K) float32: knn's lists.  weight: (P,) float32 or None (1 each).

    Voters of Gaussian i, in this order: i itself, then idx[i, 0 .. K-1].  Voter j votes iff 0 <= j < P, labels[j] >= 0,
    0 < weight[j] < inf and - a neighbour - dist2[i, slot] <= max_dist^2 (max_dist=None: no limit, dist2 not needed).  A label's
    score is the float32 sum of its voters' weights in voter order.  The largest score wins; among equal scores i's own label if
    it is one of them, otherwise the smallest label.  No voter: -1.  fill=False: a Gaussian whose own label is negative stays -1.

    iterations: Jacobi steps, one launch each, ping-pong between two buffers; the weights stay as given.
    Returns the labels as int64 (like LabelLifter.labels()); with return_share also (P,) float32, the winner's score over the
    voters' total in the last step (0 where the result is -1)."""
    _need_device(labels, "labels")
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"labels: an int32 or int64 (P,) tensor expected, got {_describe(labels)}")
    P, dev = labels.shape[0], labels.device
    _check_lists(idx, dist2, P, dev)
    if weight is not None and (not torch.is_tensor(weight) or weight.dtype != torch.float32 or tuple(weight.shape) != (P,)
                               or weight.device != dev):
        raise ValueError(f"weight: a float32 ({P},) tensor on {dev} or None expected, got {_describe(weight)}")
    if not isinstance(iterations, int) or isinstance(iterations, bool) or iterations < 1:
        raise ValueError(f"iterations = {iterations!r}: an integer >= 1 expected")
    limit2 = _max_dist2(max_dist, dist2)
    with torch.no_grad():
        cur = labels.detach().clamp_min(-1).to(torch.int32).contiguous()      # a new tensor: the two buffers are written in turn
        nxt = torch.empty_like(cur)
        share = torch.empty(P, device=dev, dtype=torch.float32) if return_share else None
        w = None if weight is None else weight.detach().contiguous()
        d2 = None if (dist2 is None or math.isinf(limit2)) else dist2.detach().contiguous()
        lists = idx.contiguous()
        for it in range(iterations):
            _C.label_mode_filter(cur, w, lists, d2, limit2, bool(fill), nxt, share if it == iterations - 1 else None)
            cur, nxt = nxt, cur
        out = cur.long()
    return (out, share) if return_share else out


def smooth_labels(lifter, xyz, k=8, iterations=1, max_dist=None, fill=True, min_weight=0.0, return_share=False):
    """lifter.labels() smoothed over the k nearest neighbours in `xyz` ((P, 3) float32 on the device: the Gaussians' means), for a
    contrib.LabelLifter or an instances.InstanceLifter alike: the votes weigh lifter.confidence(); the Gaussians that are not
    lifter.seen(min_weight) enter as unlabelled (with fill they take their neighbours' label).  Returns (P,) int64."""
    for name in ("labels", "confidence", "seen"):
        if not callable(getattr(lifter, name, None)):
            raise ValueError(f"lifter: an object with labels(), confidence() and seen() expected (LabelLifter, InstanceLifter), "
                             f"got {type(lifter).__name__}")
    idx, dist2 = knn(xyz, k, return_dist2=max_dist is not None)
    labels = torch.where(lifter.seen(min_weight), lifter.labels(), torch.full((), -1, dtype=torch.int64, device=idx.device))
    return mode_filter(labels, idx, weight=lifter.confidence(), dist2=dist2, max_dist=max_dist, iterations=iterations, fill=fill,
                       return_share=return_share)


def clean_selection(mask, idx, weight=None, dist2=None, max_dist=None, iterations=1):
    """A boolean (P,) `mask` of edit.apply_edit (LabelLifter.select, MaskLifter.select, edit.selection_mask) through the mode
    filter as the two-label problem {0: not selected, 1: selected}: a selected Gaussian among unselected neighbours is dropped, a
    pinhole in a selected region is filled.  A tie keeps the Gaussian as it was.  Returns (P,) bool."""
    _need_device(mask, "mask")
    if mask.dtype != torch.bool or mask.dim() != 1:
        raise ValueError(f"mask: a bool (P,) tensor expected, got {_describe(mask)}")
    out = mode_filter(mask.to(torch.int32), idx, weight=weight, dist2=dist2, max_dist=max_dist, iterations=iterations, fill=True)
    return out == 1


# ---- the lists as a graph: connected components ----------------------------------------------------------------------------

Components = collections.namedtuple("Components", ["root", "size", "comp", "comp_root", "n_comp", "status"])
SplitLabels = collections.namedtuple("SplitLabels", ["comp", "n_comp", "comp_label"])


def _int_labels(labels, idx, name="labels"):
    """labels as the kernels take them: int32, contiguous, every negative value -1"""
    _need_device(labels, name)
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: an int32 or int64 (P,) tensor expected, got {_describe(labels)}")
    _check_lists(idx, None, labels.shape[0], labels.device)
    return labels.detach().clamp_min(-1).to(torch.int32).contiguous()


def _components(idx, labels32, dist2, max_dist, mutual, dense):
    """the int32 tensors of _C.knn_components; labels32: _int_labels' or None"""
    _need_device(idx, "idx")
    _check_lists(idx, dist2, idx.shape[0] if idx.dim() else -1, idx.device)
    limit2 = _max_dist2(max_dist, dist2)
    d2 = None if (dist2 is None or math.isinf(limit2)) else dist2.detach().contiguous()
    with torch.no_grad():
        return _C.knn_components(idx.contiguous(), d2, limit2, labels32, bool(mutual), bool(dense))


def components(idx, labels=None, dist2=None, max_dist=None, mutual=False, dense=False):
    """The connected components of the Gaussians over their neighbour lists.  idx (P, K) int32 and dist2 (P, K) float32: knn's
    lists (any integers are allowed in idx: an entry outside 0 .. P-1 or equal to its row is no edge).  labels: (P,) int32 or
    int64 or None; a negative label takes its Gaussian out of the graph (root -1, size 0, comp -1), and an edge joins equal labels
    only.  max_dist: an edge needs dist2[i, slot] <= max_dist^2 (None: no limit).  {i, j} is an edge if j is in i's list or i in
    j's; with mutual=True only if both.

    Returns Components(root, size, comp, comp_root, n_comp, status), int64 like LabelLifter.labels(): root[i] the smallest index
    of i's component, size[i] its number of members; with dense=True also comp[i] (the rank of root[i] among the roots),
    comp_root (P,) (the root of component c for c < n_comp, -1 behind) and n_comp (a 0-dim tensor on the device, never read here);
    without, the three are None.  status: a 0-dim device tensor, 0 (non-zero only if a union-find walk reached its cap)."""
    labels32 = None if labels is None else _int_labels(labels, idx)
    res = _components(idx, labels32, dist2, max_dist, mutual, dense)
    return Components(*(None if t is None else t.long() for t in res))


def _filter_components(labels_or_mask, idx, min_size, largest, num_labels, dist2, max_dist, mutual):
    if not isinstance(min_size, int) or isinstance(min_size, bool) or not 1 <= min_size < 2**31:
        raise ValueError(f"min_size = {min_size!r}: an integer >= 1 expected")
    _need_device(labels_or_mask, "labels")
    is_mask = labels_or_mask.dtype == torch.bool
    if is_mask:
        if labels_or_mask.dim() != 1:
            raise ValueError(f"mask: a bool (P,) tensor expected, got {_describe(labels_or_mask)}")
        _check_lists(idx, None, labels_or_mask.shape[0], labels_or_mask.device)
        labels32 = labels_or_mask.to(torch.int32) - 1             # selected: label 0, unselected: -1
        num_labels = 1
    else:
        labels32 = _int_labels(labels_or_mask, idx)               # a new tensor: filtered in place below
        if largest and (not isinstance(num_labels, int) or isinstance(num_labels, bool) or not 0 <= num_labels < 2**31):
            raise ValueError(f"num_labels = {num_labels!r}: keep_largest on labels needs the number of labels (a lifter's class count "
                             f"or max_instances), an integer >= 0")
    root, size = _components(idx, labels32, dist2, max_dist, mutual, False)[:2]
    with torch.no_grad():
        _C.component_filter(labels32, root, size, min_size, bool(largest), num_labels if largest else 0, labels32)
    return labels32 >= 0 if is_mask else labels32.long()


def drop_small(labels_or_mask, idx, min_size, dist2=None, max_dist=None, mutual=False):
    """Drops the connected parts below min_size Gaussians.  labels_or_mask: (P,) int32 / int64 labels (negative = unlabelled; a
    component joins equal labels only) or a bool `mask` of edit.apply_edit (selected = label 0).  Returns the labels as int64 with
    -1 where a part was dropped, or the mask as bool.  idx, dist2, max_dist, mutual: as for components()."""
    return _filter_components(labels_or_mask, idx, min_size, False, None, dist2, max_dist, mutual)


def keep_largest(labels_or_mask, idx, num_labels=None, min_size=1, dist2=None, max_dist=None, mutual=False):
    """Keeps, of every label, its largest connected part (among equal sizes the one that holds the lowest index) if it has
    min_size Gaussians; everything else becomes -1 (False for a bool mask).  On labels num_labels is needed - a lifter's class
    count or max_instances -, and a label >= num_labels is dropped; a bool mask needs none."""
    return _filter_components(labels_or_mask, idx, min_size, True, num_labels, dist2, max_dist, mutual)


def split_labels(labels, idx, dist2=None, max_dist=None, mutual=False):
    """Re-ids a label field whose ids have several bodies (an InstanceLifter's, where two chairs shared a mask): every connected
    part of a label becomes an id of its own.  Returns SplitLabels(comp, n_comp, comp_label): comp (P,) int64, the new id of every
    Gaussian (-1 where labels is negative), ascending in the parts' lowest index; n_comp, their number, a 0-dim device tensor;
    comp_label (P,) int64, the old label of id c for c < n_comp and -1 behind."""
    labels32 = _int_labels(labels, idx)
    _, _, comp, comp_root, n_comp, _ = _components(idx, labels32, dist2, max_dist, mutual, True)
    with torch.no_grad():
        comp_root = comp_root.long()
        old = labels32.long().gather(0, comp_root.clamp_min(0)) if labels32.shape[0] else labels32.long()
        comp_label = torch.where(comp_root >= 0, old, torch.full((), -1, dtype=torch.int64, device=old.device))
    return SplitLabels(comp.long(), n_comp.long(), comp_label)


# ---- density: radius counts and statistical outlier removal --------------------------------------------------------------------

Outliers = collections.namedtuple("Outliers", ["score", "keep", "stats"])


def _points(points, name="points"):
    _need_device(points, name)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{name}: a float32 (P, 3) tensor expected, got {_describe(points)}")
    return points.detach()


def _node_labels(labels, P, dev, name="labels"):
    """(P,) int32 / int64 labels on `dev` as the kernels take them: int32, contiguous, every negative value -1"""
    if not torch.is_tensor(labels) or labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64) or labels.shape[0] != P \
            or labels.device != dev:
        raise ValueError(f"{name}: an int32 or int64 ({P},) tensor on {dev} expected, got {_describe(labels)}")
    return labels.detach().clamp_min(-1).to(torch.int32).contiguous()


def _count(value, name, least):
    if not isinstance(value, int) or isinstance(value, bool) or not least <= value < 2**31:
        raise ValueError(f"{name} = {value!r}: an integer >= {least} expected")
    return value


def radius_count(points, radius, labels=None, cap=None):
    """The number of other points within `radius` of every point.  points: (P, 3) float32 on the device.  radius: a number >= 0
    (inf allowed), squared in float32; point j is within it iff ((dx*dx) + (dy*dy)) + (dz*dz) <= radius^2 in float32, knn's
    distance.  labels: (P,) int32 or int64 or None: only points of the same non-negative label are counted, and a point with a
    negative label gets 0.  cap: None or an integer >= 1, the result is min(count, cap) (the walk of a point ends there: ask for no
    more than the decision needs).  Self is excluded by index: duplicates are counted.  A point with a NaN or infinite coordinate has
    count 0 and is counted by nobody.  Returns (P,) int32, a function of the inputs alone."""
    pts = _points(points)
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or math.isnan(radius) or radius < 0:
        raise ValueError(f"radius = {radius!r}: a number >= 0 expected")
    r = torch.tensor(float(radius), dtype=torch.float32)
    radius2 = float(r * r)
    labels32 = None if labels is None else _node_labels(labels, pts.shape[0], pts.device)
    limit = 0 if cap is None else _count(cap, "cap", 1)
    with torch.no_grad():
        return _C.radius_count(pts, radius2, labels32, limit)


def _scores(idx, dist2, labels32, num_groups, ratio):
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not math.isfinite(ratio) or ratio < 0:
        raise ValueError(f"ratio = {ratio!r}: a finite number >= 0 expected")
    with torch.no_grad():
        return Outliers(*_C.knn_outliers(idx.contiguous(), dist2.detach().contiguous(), labels32, num_groups, float(ratio)))


def outlier_scores(idx, dist2, labels=None, num_labels=None, ratio=2.0):
    """Statistical outlier scores over knn's lists.  idx (P, K) int32, dist2 (P, K) float32 (any integers are allowed in idx).
    labels: (P,) int32 or int64 with num_labels, or None (one group).  Gaussian i is a member iff 0 <= labels[i] < num_labels; a
    slot of its row counts iff its entry j is in 0 .. P-1, is not i, carries i's label and its dist2 is < inf.

    Returns Outliers(score, keep, stats): score (P,) float32, the mean of sqrt(dist2) over the counting slots, formed in float64 and
    rounded once (+inf for a Gaussian that is no member or has no such slot); stats (G, 4) float64 on the device, never read
    here: per group {n, mean, std, threshold} over its members with a finite score, std the N - 1 form (0 for n < 2), threshold =
    mean + ratio * std; keep (P,) bool: score < inf and score <= threshold of its group."""
    _need_device(idx, "idx")
    P = idx.shape[0] if idx.dim() else -1
    _check_lists(idx, dist2, P, idx.device)
    if dist2 is None:
        raise ValueError("dist2: the squared distances of knn are needed, got None")
    if labels is None:
        if num_labels is not None:
            raise ValueError(f"num_labels = {num_labels!r} without labels: one group, None expected")
        return _scores(idx, dist2, None, 1, ratio)
    labels32 = _node_labels(labels, P, idx.device)
    return _scores(idx, dist2, labels32, _count(num_labels, "num_labels", 1), ratio)


def _density_input(labels_or_mask, xyz, num_labels, need_num_labels):
    """(xyz, labels32 or None, num_groups, kind) of labels, a bool mask or None over the points xyz"""
    pts = _points(xyz, "xyz")
    P, dev = pts.shape[0], pts.device
    if labels_or_mask is None:
        return pts, None, 1, "none"
    if torch.is_tensor(labels_or_mask) and labels_or_mask.dtype == torch.bool:
        if labels_or_mask.dim() != 1 or labels_or_mask.shape[0] != P or labels_or_mask.device != dev:
            raise ValueError(f"mask: a bool ({P},) tensor on {dev} expected, got {_describe(labels_or_mask)}")
        return pts, labels_or_mask.to(torch.int32) - 1, 1, "mask"                 # selected: label 0, unselected: -1
    labels32 = _node_labels(labels_or_mask, P, dev)
    if need_num_labels and (not isinstance(num_labels, int) or isinstance(num_labels, bool) or not 1 <= num_labels < 2**31):
        raise ValueError(f"num_labels = {num_labels!r}: the statistics of labels need the number of labels (a lifter's class count or "
                         f"max_instances), an integer >= 1")
    return pts, labels32, num_labels, "labels"


def _density_result(keep, labels32, kind):
    if kind == "labels":
        return torch.where(keep, labels32, torch.full((), -1, dtype=torch.int32, device=keep.device)).long()
    return keep


def remove_statistical_outliers(labels_or_mask, xyz, k=8, ratio=2.0, num_labels=None):
    """Statistical outlier removal: knn(xyz, k), outlier_scores per label, and what is not kept goes.  labels_or_mask: (P,) int32 /
    int64 labels with num_labels (negative = unlabelled; every label has its own mean and deviation, a label >= num_labels is
    dropped), a bool `mask` of edit.apply_edit (selected = one group, as drop_small treats it) or None (all points one group).
    Returns the labels as int64 with -1 for the outliers, the mask as bool, or - for None - the bool keep over all points."""
    pts, labels32, groups, kind = _density_input(labels_or_mask, xyz, num_labels, True)
    idx, dist2 = knn(pts, k)
    return _density_result(_scores(idx, dist2, labels32, groups, ratio).keep, labels32, kind)


def remove_radius_outliers(labels_or_mask, xyz, radius, min_neighbors):
    """Radius outlier removal: what has fewer than min_neighbors other points (of its label) within `radius` goes -
    radius_count(cap=min_neighbors) >= min_neighbors.  labels_or_mask and the result: as for remove_statistical_outliers (labels
    need no num_labels here)."""
    pts, labels32, _, kind = _density_input(labels_or_mask, xyz, None, False)
    limit = _count(min_neighbors, "min_neighbors", 1)
    keep = radius_count(pts, radius, labels32, cap=limit) >= limit
    return _density_result(keep, labels32, kind)


__all__ = ["MAX_NEIGHBORS", "knn", "mode_filter", "smooth_labels", "clean_selection", "Components", "SplitLabels", "components",
           "drop_small", "keep_largest", "split_labels", "Outliers", "radius_count", "outlier_scores", "remove_statistical_outliers",
           "remove_radius_outliers"]
