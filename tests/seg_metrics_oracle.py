"""numpy / fp64 restatement of the segmentation scores (include/f3dgs.h: f3dgs_seg_metrics) and of the palette pictures
(f3dgs_seg_colorize), for the tests: counts by np.bincount, then the finish rules - invalid pixels, the ranking with the lower
label first among equal counts, the cut at num_classes, NaN skipping, pooling over the views."""
import numpy as np

COUNT_NAMES = ("n_t", "n_s", "n_ts", "n_g", "m_g", "m_s", "m_gs")
SCALAR_NAMES = ("valid", "equal", "invalid", "matched", "correct")


def counts(teacher, student, gt=None, num_labels=None):
    """The counters of ONE view (maps of any shape and integer type), a dict of int64 arrays (L,) and Python ints."""
    L = int(num_labels)
    # Python-int comparison on int64 copies: the full-width value decides (uint64 beyond 2^63 is not a case of the tests)
    t = np.asarray(teacher).reshape(-1).astype(np.int64)
    s = np.asarray(student).reshape(-1).astype(np.int64)
    ok = (t >= 0) & (t < L) & (s >= 0) & (s < L)
    if gt is not None:
        g = np.asarray(gt).reshape(-1).astype(np.int64)
        ok &= (g >= 0) & (g < L)
    out = {"invalid": int((~ok).sum()), "valid": int(ok.sum())}
    t, s = t[ok], s[ok]

    def hist(labels, where=None):
        return np.bincount(labels if where is None else labels[where], minlength=L).astype(np.int64)

    out["n_t"], out["n_s"], out["n_ts"] = hist(t), hist(s), hist(t, t == s)
    out["equal"] = int((t == s).sum())
    if gt is not None:
        g = g[ok]
        match = g == t
        out["n_g"], out["m_g"], out["m_s"], out["m_gs"] = hist(g), hist(g, match), hist(s, match), hist(g, match & (s == g))
        out["matched"], out["correct"] = int(match.sum()), int((match & (s == g)).sum())
    return out


def pool(list_of_counts):
    """Label-wise and scalar sums of the counters of several views."""
    out = {}
    for k in list_of_counts[0]:
        out[k] = sum(c[k] for c in list_of_counts)
    return out


def _ranked_mean(key, inter, union, num_classes):
    L = len(key)
    order = sorted(range(L), key=lambda i: (-int(key[i]), i))          # descending count, the lower label first
    kept = [i for i in order[:num_classes] if key[i] > 0]
    per_label = np.full(L, np.nan)
    total, terms = 0.0, 0
    for i in kept:
        v = float(inter[i]) / float(union[i]) if union[i] > 0 else float("nan")
        per_label[i] = v
        if v == v:
            total += v
            terms += 1
    ranked = np.full(num_classes, -1, np.int64)
    ranked[:len(kept)] = kept
    return (total / terms if terms else float("nan")), per_label, ranked


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def finish(c, num_classes):
    """The scores of one row of counters (a view's or a pooled one)."""
    out = {"invalid": c["invalid"], "accuracy": _ratio(c["equal"], c["valid"])}
    both = c["n_t"] + c["n_s"]
    out["iou"], out["iou_per_label"], out["labels_ranked"] = _ranked_mean(both, c["n_ts"], both - c["n_ts"], num_classes)
    if "n_g" in c:
        out["accuracy_masked"] = _ratio(c["correct"], c["matched"])
        out["iou_masked"], out["iou_per_label_masked"], out["labels_ranked_masked"] = _ranked_mean(
            c["n_g"] + both, c["m_gs"], c["m_g"] + c["m_s"] - c["m_gs"], num_classes)
    return out


def scores(teachers, students, gts=None, num_labels=None, num_classes=7):
    """(list of per-view score dicts, pooled score dict, list of per-view counter dicts) of N views (sequences of maps)."""
    cs = [counts(teachers[i], students[i], None if gts is None else gts[i], num_labels) for i in range(len(teachers))]
    return [finish(c, num_classes) for c in cs], finish(pool(cs), num_classes), cs


# ---- pictures: the reference's fp32 chain (segmentation.py:552-559) in numpy float32 ----------------------------------------
def _bytes(v):
    return np.clip(v * np.float32(255.0), np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def colorize(labels, palette, fill=(0, 0, 0)):
    """(..., 3) uint8: palette[label], `fill` where the label lies outside the palette."""
    labels = np.asarray(labels)
    palette = np.asarray(palette, np.uint8)
    wide = labels.astype(np.int64)
    ok = (wide >= 0) & (wide < len(palette))
    out = np.empty(labels.shape + (3,), np.uint8)
    out[...] = np.asarray(fill, np.uint8)
    out[ok] = palette[wide[ok]]
    return out


def overlay(labels, palette, image, weights=(0.4, 0.6), strip=False, fill=(0, 0, 0)):
    """image (3,H,W) or (N,3,H,W) float32 -> uint8 (H,W',3) or (N,H,W',3)."""
    mask8 = colorize(labels, palette, fill)
    mask = mask8.astype(np.float32) / np.float32(255.0)
    img = np.moveaxis(np.asarray(image, np.float32), -3, -1)
    blend = img * np.float32(weights[0]) + mask * np.float32(weights[1])
    if not strip:
        return _bytes(blend)
    return np.concatenate([_bytes(img), _bytes(blend), _bytes(mask)], axis=-2)      # (the chain gives every byte back: test_seg_metrics_cpu)
