"""Neighbourhoods of the Gaussians in 3D: K-nearest-neighbour lists with indices, and a mode filter of per-Gaussian labels.

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


__all__ = ["MAX_NEIGHBORS", "knn", "mode_filter", "smooth_labels", "clean_selection", "Components", "SplitLabels", "components",
           "drop_small", "keep_largest", "split_labels"]
