"""Segmentation scores of rendered views in one pass: pixel accuracy and mean IoU of N (teacher, student[, gt]) label maps, and
the palette pictures of a label map, on the device.

Replaces the scoring half of the reference's semantic-segmentation evaluation - encoders/lseg_encoder/segmentation_metric.py

    accuracy = calculate_accuracy(gt_predict, pred_predict)            # :818-821, per test view
    iou = calculate_iou(gt_predict, pred_predict, 7)
    accuracy_accum += accuracy; iou_accum += iou                       # :827-832, the reported means

(and the ground-truth-masked `calculate_accuracy_mask`, `calculate_iou_mask`), which per view build two boolean maps and four
host sums per class - and the pictures segmentation.py:547-559 writes of a label map - with

    scores = segmentation_scores(teacher, student, gt, num_labels=150)     # SegScores of (N,) device tensors, no host read
    report = evaluate_segmentation(teachers, students, num_labels=150)     # the means, per-view lists and the pooled row, one host read
    import segmentation_metric, seg_metrics; seg_metrics.install(segmentation_metric)   # or: the reference's script, fused
    strip = overlay(labels, palette, image, strip=True)                    # [image | 0.4 image + 0.6 mask | mask] as uint8

Three launches per call (csrc/seg_metrics.hip behind include/f3dgs.h: f3dgs_seg_metrics): a clear, the per-label integer counts of
every view, and one workgroup per view - plus one for the POOLED row, the counters summed over the views - that ranks the labels
and forms the fp64 quotients.  A pixel counts when each of its labels lies in [0, num_labels); the others are reported in
`invalid`.  Where two labels are equally frequent at the `num_classes` cut the LOWER label is kept (segment.label_agreement's
rule; the reference's unstable argsort leaves it open).  Everything is integer counting and a handful of fp64 divisions: the
results are exact and the same bits from run to run.

HIP only; no CPU fallback; argument errors are raised as ValueError before any device work.
"""
from __future__ import annotations

import colorsys
from collections import namedtuple

import numpy as np
import torch

MAX_LABELS = 256                # F3DGS_SEGMENT_MAX_TEXTS
LABEL_DTYPES = (torch.uint8, torch.int32, torch.int64)

SegCounts = namedtuple("SegCounts", ["n_t", "n_s", "n_ts", "n_g", "m_g", "m_s", "m_gs", "valid", "equal", "invalid", "matched", "correct"])
SegScores = namedtuple("SegScores", ["accuracy", "iou", "accuracy_masked", "iou_masked", "invalid", "iou_per_label", "labels_ranked",
                                     "iou_per_label_masked", "labels_ranked_masked", "pooled"])
SegPooled = namedtuple("SegPooled", ["accuracy", "iou", "accuracy_masked", "iou_masked", "invalid", "iou_per_label", "labels_ranked",
                                     "iou_per_label_masked", "labels_ranked_masked", "counts", "scalars"])


def _C():
    from diff_gaussian_rasterization import _C as ext
    return ext


def _map(t, name):
    """One side as an (N,H,W) tensor; every check before device work."""
    if not torch.is_tensor(t):
        raise ValueError(f"{name}: a tensor expected, got {type(t).__name__}")
    if t.dtype not in LABEL_DTYPES:
        raise ValueError(f"{name}: uint8, int32 or int64 labels expected, got {t.dtype}")
    if t.dim() not in (2, 3):
        raise ValueError(f"{name}: (H,W) or (N,H,W) expected, got {tuple(t.shape)}")
    t = t.detach()
    if t.dim() == 2:
        t = t[None]
    if t.numel() == 0:
        raise ValueError(f"{name}: empty label map {tuple(t.shape)}")
    return t


def _carry(carry, num_labels, has_gt):
    """(counts, scalars) of an earlier call's pooled row, checked; or two empty tensors"""
    e = torch.Tensor([])
    if carry is None:
        return e, e
    if not isinstance(carry, (tuple, list)) or len(carry) != 2 or not all(torch.is_tensor(c) and c.dtype == torch.int64 for c in carry):
        raise ValueError("carry: the (counts, scalars) int64 tensors of an earlier call's pooled row expected")
    shape = (7 if has_gt else 3, num_labels)
    if tuple(carry[0].shape) != shape or tuple(carry[1].shape) != (5,):
        raise ValueError(f"carry: counts {shape} and scalars (5,) expected (the same num_labels, with or without gt as this call), got "
                         f"{tuple(carry[0].shape)} and {tuple(carry[1].shape)}")
    return carry[0], carry[1]


def _prepare(teacher, student, gt, num_labels, num_classes, carry=None):
    if not isinstance(num_labels, int) or isinstance(num_labels, bool) or not 1 <= num_labels <= MAX_LABELS:
        raise ValueError(f"num_labels {num_labels!r}: an integer from 1 to {MAX_LABELS} expected")
    if not isinstance(num_classes, int) or isinstance(num_classes, bool) or not 1 <= num_classes <= num_labels:
        raise ValueError(f"num_classes {num_classes!r}: an integer from 1 to num_labels = {num_labels} expected")
    sides = [("teacher", teacher), ("student", student)] + ([("gt", gt)] if gt is not None else [])
    maps = [_map(t, name) for name, t in sides]
    for (name, _), m in zip(sides[1:], maps[1:]):
        if m.shape != maps[0].shape:
            raise ValueError(f"teacher {tuple(maps[0].shape)} and {name} {tuple(m.shape)} shapes differ")
    carry = _carry(carry, num_labels, gt is not None)
    for (name, _), m in zip(sides, maps):          # last, so that every other error can be met without a device
        if m.device.type != "cuda":
            raise ValueError(f"{name} lives on {m.device}: the scores run on a HIP device only (no CPU path)")
        if m.device != maps[0].device:
            raise ValueError(f"teacher is on {maps[0].device}, {name} on {m.device}")
    return maps[0], maps[1], (maps[2] if gt is not None else None), carry


def _run(teacher, student, gt, num_labels, num_classes, carry=None, want_scores=True):
    t, s, g, (cc, cs) = _prepare(teacher, student, gt, num_labels, num_classes, carry)
    out = _C().seg_metrics(t, s, g if g is not None else torch.Tensor([]), num_labels, num_classes, cc, cs, want_scores)
    return out, t.shape[0], g is not None


@torch.no_grad()
def segmentation_counts(teacher, student, gt=None, *, num_labels) -> SegCounts:
    """The integer counters of every view, int64 device tensors.  Over the valid pixels (each label in [0, num_labels)), with
    match := (gt == teacher): n_t, n_s, n_g (N, L) the pixels of teacher / student / gt == i; n_ts teacher == i and student == i;
    m_g, m_s, m_gs match and gt == i / student == i / both; valid, equal (teacher == student), invalid (pixels left out), matched,
    correct (match and student == gt), (N,) each.  The gt-dependent ones are None without gt.
    teacher, student, gt: (H,W) or (N,H,W), uint8, int32 or int64, each side by itself."""
    (counts, scalars, _, _, _), N, has_gt = _run(teacher, student, gt, num_labels, 1, want_scores=False)      # no ranking, no quotients
    c = [counts[a, :N] for a in range(counts.shape[0])] + [None] * (7 - counts.shape[0])
    return SegCounts(n_t=c[0], n_s=c[1], n_ts=c[2], n_g=c[3], m_g=c[4], m_s=c[5], m_gs=c[6], valid=scalars[0, :N], equal=scalars[1, :N],
                     invalid=scalars[2, :N], matched=scalars[3, :N] if has_gt else None, correct=scalars[4, :N] if has_gt else None)


def _scores(out, N, has_gt):
    counts, scalars, scores, per_label, ranked = out

    def rows(sel):
        return dict(accuracy=scores[0][sel], iou=scores[1][sel], accuracy_masked=scores[2][sel] if has_gt else None,
                    iou_masked=scores[3][sel] if has_gt else None, invalid=scalars[2][sel], iou_per_label=per_label[0][sel],
                    labels_ranked=ranked[0][sel], iou_per_label_masked=per_label[1][sel] if has_gt else None,
                    labels_ranked_masked=ranked[1][sel] if has_gt else None)

    pooled = SegPooled(counts=counts[:, N], scalars=scalars[:, N], **rows(N))
    return SegScores(pooled=pooled, **rows(slice(0, N)))


@torch.no_grad()
def segmentation_scores(teacher, student, gt=None, *, num_labels, num_classes=7, carry=None) -> SegScores:
    """SegScores of float64 device tensors, one value per view: accuracy = equal / valid; iou = the mean intersection / union over
    the `num_classes` most frequent labels of teacher and student together (the lower label first among equal counts; only labels
    that occur); with gt also accuracy_masked = correct / matched and iou_masked, both over the pixels where gt == teacher, the
    labels ranked over all three maps and a label without such pixels skipped (None without gt).  0 / 0 is NaN, as in the
    reference.  invalid (N,) int64; iou_per_label (N, L), NaN where the label did not make the cut; labels_ranked (N, num_classes)
    int64, padded with -1 (and the same two for the masked ranking).  `pooled`: the same quantities (0-dim, (L,), (num_classes,))
    of the counters summed over the N views, with those counters (`pooled.counts` (3 or 7, L), `pooled.scalars` (5,)).
    carry: the (pooled.counts, pooled.scalars) of an earlier call with the same num_labels and the same sides, added into this
    call's pooled row - calls chained this way pool views of different sizes or types as one call would pool them stacked.
    1 <= num_classes <= num_labels <= 256.
    Nothing is read back to the host: the call may be captured in a graph."""
    out, N, has_gt = _run(teacher, student, gt, num_labels, num_classes, carry)
    return _scores(out, N, has_gt)


def evaluate_segmentation(teachers, students, gts=None, *, num_labels, num_classes=7) -> dict:
    """The segmentation scores of a test set as segmentation_metric.py:827-832 reports them: {"accuracy", "iou"} (with gts also
    {"accuracy_masked", "iou_masked"}) - the means over the views, a running sum divided by the count in Python floats -,
    {"per_view": {name: [...]}} in input order and {"pooled": {name: value}}, the scores of the counters summed over all views.
    teachers, students, gts: lists of (H,W) label maps of possibly different sizes and types; every run of equal-shaped, equally
    typed views goes to the device in one call and the host reads the results once, at the end.  A view with a label outside
    [0, num_labels) raises ValueError (after that read), naming the view and the number of such pixels."""
    if len(teachers) != len(students) or (gts is not None and len(gts) != len(teachers)):
        raise ValueError(f"{len(teachers)} teacher, {len(students)} student" + (f" and {len(gts)} gt" if gts is not None else "") + " label maps")
    has_gt = gts is not None
    names = ("accuracy", "iou") + (("accuracy_masked", "iou_masked") if has_gt else ())
    sides = (teachers, students) + ((gts,) if has_gt else ())

    def key(i):
        return tuple((tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t) else type(t) for t in (side[i] for side in sides))

    # argument errors of every view before any device work
    runs, i = [], 0
    while i < len(teachers):
        j = i + 1
        while j < len(teachers) and key(j) == key(i):
            j += 1
        for k in range(i, j):
            for side in sides:
                if torch.is_tensor(side[k]) and side[k].dim() == 3 and side[k].shape[0] != 1:
                    raise ValueError(f"view {k}: one label map per list entry expected, got a batch of {side[k].shape[0]}")
            _prepare(teachers[k], students[k], gts[k] if has_gt else None, num_labels, num_classes)
        runs.append((i, j))
        i = j
    if not runs:
        nan = float("nan")
        return {**{n: nan for n in names}, "per_view": {n: [] for n in names}, "pooled": {n: nan for n in names}}
    parts, carry, sc = [], None, None
    for i, j in runs:
        stacked = [torch.stack([t if t.dim() == 2 else t[0] for t in side[i:j]]) for side in sides]
        sc = segmentation_scores(stacked[0], stacked[1], stacked[2] if has_gt else None, num_labels=num_labels, num_classes=num_classes,
                                 carry=carry)
        carry = (sc.pooled.counts, sc.pooled.scalars)          # the last run's pooled row is the whole set's
        parts.append(torch.stack([getattr(sc, n) for n in names] + [sc.invalid.to(torch.float64)]))
    pooled = torch.stack([getattr(sc.pooled, n) for n in names] + [sc.pooled.invalid.to(torch.float64)])
    table = torch.cat(parts + [pooled[:, None]], dim=1).cpu()          # the one host read
    invalid = table[len(names)].tolist()
    for k, v in enumerate(invalid[:-1]):
        if v:
            raise ValueError(f"view {k}: {int(v)} pixels with a label outside [0, {num_labels})")
    out = {"per_view": {}, "pooled": {}}
    for row, name in enumerate(names):
        values = table[row].tolist()
        accum = 0.0
        for v in values[:-1]:
            accum += v
        out[name] = accum / len(values[:-1])
        out["per_view"][name] = values[:-1]
        out["pooled"][name] = values[-1]
    return out


# ---- drop-ins for segmentation_metric.py ------------------------------------------------------------------------------------
def _flat(x, name):
    """A numpy array or tensor of any integer type and shape as a flat tensor on the current device, with its (min, max)."""
    if isinstance(x, np.ndarray):
        if x.dtype.kind not in "iub":
            raise ValueError(f"{name}: integer labels expected, got {x.dtype}")
        if x.dtype not in (np.uint8, np.int32, np.int64):
            if x.dtype == np.uint64 and x.size and int(x.max()) >= 1 << 63:
                raise ValueError(f"{name}: label {int(x.max())}: at most {MAX_LABELS} label slots are supported")
            x = x.astype(np.int64)
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError(f"{name}: a numpy array or a tensor expected, got {type(x).__name__}")
    if x.dtype.is_floating_point or x.dtype.is_complex:
        raise ValueError(f"{name}: integer labels expected, got {x.dtype}")
    if x.numel() == 0:
        raise ValueError(f"{name}: empty label map")
    x = x.detach().reshape(-1)
    if x.dtype not in LABEL_DTYPES:
        x = x.to(torch.int64)
    return x


def _drop_in(gt, teacher, student, num_classes):
    sides = [("teacher", teacher), ("student", student)] + ([("gt", gt)] if gt is not None else [])
    flat = [_flat(x, name) for name, x in sides]
    for (name, _), f in zip(sides[1:], flat[1:]):
        if f.numel() != flat[0].numel():
            raise ValueError(f"teacher has {flat[0].numel()} pixels, {name} {f.numel()}")
    lo = min(int(f.min()) for f in flat)
    hi = max(int(f.max()) for f in flat)
    if lo < 0:
        raise ValueError(f"negative label {lo}")
    if hi + 1 > MAX_LABELS:
        raise ValueError(f"label {hi}: at most {MAX_LABELS} label slots are supported")
    if num_classes is not None and int(num_classes) < 1:
        raise ValueError(f"num_classes {num_classes}: at least 1 expected")
    dev = torch.device("cuda", torch.cuda.current_device())
    flat = [f.to(dev)[None, None] if f.device.type != "cuda" else f[None, None] for f in flat]
    L = hi + 1
    nc = L if num_classes is None else min(int(num_classes), L)
    return segmentation_scores(flat[0], flat[1], flat[2] if gt is not None else None, num_labels=L, num_classes=nc)


def calculate_accuracy(teacher, student):
    """Drop-in for segmentation_metric.py `calculate_accuracy`: the share of equal pixels, a Python float."""
    return float(_drop_in(None, teacher, student, None).accuracy[0])


def calculate_accuracy_mask(gt, teacher, student, i=None):
    """Drop-in for `calculate_accuracy_mask`: among the pixels where gt == teacher, the share where student == gt (`i`, the view
    number of the reference's commented-out mask dump, is ignored)."""
    return float(_drop_in(gt, teacher, student, None).accuracy_masked[0])


def calculate_iou(teacher, student, num_classes):
    """Drop-in for `calculate_iou`: the mean intersection / union over the num_classes most frequent labels."""
    return float(_drop_in(None, teacher, student, num_classes).iou[0])


def calculate_iou_mask(gt, teacher, student, num_classes):
    """Drop-in for `calculate_iou_mask`: the same over the pixels where gt == teacher, labels ranked over all three maps."""
    return float(_drop_in(gt, teacher, student, num_classes).iou_masked[0])


_DROP_INS = ("calculate_accuracy", "calculate_accuracy_mask", "calculate_iou", "calculate_iou_mask")


def install(module):
    """Sets the four `calculate_*` names on an imported `segmentation_metric`-like module, so that the reference's script scores
    its views with the fused kernels.  Returns the module."""
    if not any(hasattr(module, name) for name in _DROP_INS):
        raise AttributeError(f"{module.__name__} has none of {', '.join(_DROP_INS)}: not the reference's segmentation_metric")
    for name in _DROP_INS:
        setattr(module, name, globals()[name])
    return module


# ---- pictures ---------------------------------------------------------------------------------------------------------------
def default_palette(num_labels: int) -> torch.Tensor:
    """The project's own deterministic (num_labels, 3) uint8 palette (CPU tensor): label 0 black, label i > 0 the hue
    i * (golden ratio - 1) mod 1 at one of four saturation / value levels, so that neighbouring labels differ strongly and all
    256 rows are distinct.  (Not the reference's ADE20K list: a caller who wants that passes it in.)"""
    if not isinstance(num_labels, int) or isinstance(num_labels, bool) or not 1 <= num_labels <= MAX_LABELS:
        raise ValueError(f"num_labels {num_labels!r}: an integer from 1 to {MAX_LABELS} expected")
    levels = ((0.85, 1.0), (0.55, 0.85), (1.0, 0.7), (0.4, 1.0))
    rows = [(0, 0, 0)]
    for i in range(1, num_labels):
        s, v = levels[i % 4]
        r, g, b = colorsys.hsv_to_rgb((i * 0.6180339887498949) % 1.0, s, v)
        rows.append((int(r * 255 + 0.5), int(g * 255 + 0.5), int(b * 255 + 0.5)))
    return torch.tensor(rows[:num_labels], dtype=torch.uint8)


def _picture_args(labels, palette, image, fill):
    if not torch.is_tensor(labels):
        raise ValueError(f"labels: a tensor expected, got {type(labels).__name__}")
    if labels.dtype not in LABEL_DTYPES:
        raise ValueError(f"labels: uint8, int32 or int64 expected, got {labels.dtype}")
    if labels.dim() not in (2, 3) or labels.numel() == 0:
        raise ValueError(f"labels: a non-empty (H,W) or (N,H,W) map expected, got {tuple(labels.shape)}")
    single = labels.dim() == 2
    lab = labels.detach()[None] if single else labels.detach()
    pal = torch.as_tensor(np.asarray(palette)) if not torch.is_tensor(palette) else palette
    if pal.dim() != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= MAX_LABELS:
        raise ValueError(f"palette: (L,3) with 1 <= L <= {MAX_LABELS} expected, got {tuple(pal.shape)}")
    if pal.dtype != torch.uint8:
        if pal.dtype.is_floating_point or int(pal.min()) < 0 or int(pal.max()) > 255:
            raise ValueError(f"palette: byte values expected (uint8, or integers in 0..255), got {pal.dtype}")
        pal = pal.to(torch.uint8)
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or min(fill) < 0 or max(fill) > 255:
        raise ValueError(f"fill {fill}: three byte values expected")
    img = None
    if image is not None:
        if not torch.is_tensor(image) or image.dtype != torch.float32:
            raise ValueError("image: a float32 tensor expected")
        img = image.detach()[None] if image.dim() == 3 else image.detach()
        if img.dim() != 4 or tuple(img.shape) != (lab.shape[0], 3, lab.shape[1], lab.shape[2]):
            raise ValueError(f"image {tuple(image.shape)} does not match labels {tuple(labels.shape)}: (3,H,W) or (N,3,H,W) expected")
    if lab.device.type != "cuda":
        raise ValueError(f"labels live on {lab.device}: the pictures are made on a HIP device only (no CPU path)")
    if img is not None and img.device != lab.device:
        raise ValueError(f"labels are on {lab.device}, image on {img.device}")
    return lab, pal.to(lab.device), img, fill, single


@torch.no_grad()
def colorize(labels, palette, fill=(0, 0, 0)) -> torch.Tensor:
    """palette[labels] as uint8 (N,H,W,3), or (H,W,3) of an (H,W) map: the reference's mask PNG (segmentation.py:547-549).
    labels uint8 / int32 / int64 on the device; palette (L,3) byte values, L <= 256; a label outside [0, L) gets `fill`."""
    lab, pal, _, fill, single = _picture_args(labels, palette, None, fill)
    C = _C()
    out = C.seg_colorize(lab, pal, torch.Tensor([]), C.SEG_COLOR_MASK, 0.0, 1.0, fill)
    return out[0] if single else out


@torch.no_grad()
def overlay(labels, palette, image, weights=(0.4, 0.6), strip=False, fill=(0, 0, 0)) -> torch.Tensor:
    """trunc(255 (a image + b mask)) as uint8 (N,H,W,3), mask = palette[labels] / 255 and (a, b) = weights; with strip=True the
    reference's `_vis.png` (segmentation.py:552-559), (N,H,3W,3): [image | blend | mask].  image: float32 (3,H,W) or (N,3,H,W)
    in [0, 1].  The arithmetic is the reference's fp32 chain, one rounding per operation: byte / 255, image * a, mask * b, their
    sum, times 255, truncated.  The reference casts to uint8 without clamping, which leaves an image outside [0, 1] undefined;
    here such values are clamped to 0..255 first (NaN gives 0) - inside [0, 1] the clamp changes nothing."""
    if len(weights) != 2:
        raise ValueError(f"weights {weights!r}: (a, b) expected")
    if image is None:
        raise ValueError("image: needed for an overlay (colorize makes the mask alone)")
    lab, pal, img, fill, single = _picture_args(labels, palette, image, fill)
    C = _C()
    out = C.seg_colorize(lab, pal, img, C.SEG_COLOR_STRIP if strip else C.SEG_COLOR_BLEND, float(weights[0]), float(weights[1]), fill)
    return out[0] if single else out
