"""TEST INFRASTRUCTURE - numpy restatement of the density kernels (csrc/outliers.hip), as plain as it gets.

radius_count: brute force in float32 with the kernel's operation order - dx = candidate - query, ((dx*dx) + (dy*dy)) + (dz*dz), one
rounding per operation -, self excluded by index, a non-finite point with count 0 and counted by nobody, equal non-negative labels,
the cap as a minimum at the end.
scores / outliers: the rules of include/f3dgs.h (f3dgs_knn_outliers) as a loop over the points; a score is the float64 mean of
float64 square roots rounded once to float32; the statistics of a group are math.fsum sums (exact, rounded once).
The two `clear` functions say how far an input is from a decision boundary: what lets a test compare decisions exactly."""
import math

import numpy as np


def _dist2_rows(p, a, n):
    """float32 squared distances of queries a .. a+n-1 (rows) to every point (columns)"""
    q = p[a:a + n]
    with np.errstate(over="ignore", invalid="ignore"):
        dx = p[None, :, 0] - q[:, None, 0]
        dy = p[None, :, 1] - q[:, None, 1]
        dz = p[None, :, 2] - q[:, None, 2]
        d = ((dx * dx) + (dy * dy)) + (dz * dz)
    assert d.dtype == np.float32
    return d


def radius_count(points, radius2, labels=None, cap=0, chunk=512):
    """points (P, 3) float32, radius2 a float32 value (inf allowed), labels (P,) integers or None -> count (P,) int32"""
    p = np.ascontiguousarray(points, np.float32)
    P = p.shape[0]
    r2 = np.float32(radius2)
    assert r2 >= 0 and cap >= 0
    out = np.zeros(P, np.int32)
    finite = np.isfinite(p).all(1)
    lab = None if labels is None else np.asarray(labels).astype(np.int64)
    for a in range(0, P, chunk):
        d = _dist2_rows(p, a, chunk)
        n = d.shape[0]
        with np.errstate(invalid="ignore"):
            hit = (d <= r2) & finite[None, :] & finite[a:a + n, None]
        hit[np.arange(n), a + np.arange(n)] = False
        if lab is not None:
            hit &= (lab[None, :] == lab[a:a + n, None]) & (lab[a:a + n, None] >= 0)
        out[a:a + n] = hit.sum(1)
    return np.minimum(out, cap).astype(np.int32) if cap > 0 else out


def pair_dist2(points, lo2, hi2, chunk=512):
    """the float32 squared distances d of the pairs i < j with lo2 <= d <= hi2, sorted"""
    p = np.ascontiguousarray(points, np.float32)
    P = p.shape[0]
    found = []
    for a in range(0, P, chunk):
        d = _dist2_rows(p, a, chunk)
        n = d.shape[0]
        upper = np.arange(P)[None, :] > (a + np.arange(n))[:, None]
        with np.errstate(invalid="ignore"):
            found.append(d[upper & (d >= np.float32(lo2)) & (d <= np.float32(hi2))])
    return np.sort(np.concatenate(found)) if found else np.zeros(0, np.float32)


def radius_clearance(points, radius):
    """min over the pairs of |dist / radius - 1|, the distance taken from the float32 squared distance: beyond 1e-5 a float32
    and a float64 search agree on every pair.  radius: a float32 value; it is squared in float32 as the Python layer does."""
    r = np.float32(radius)
    r2 = np.float64(r * r)
    near = pair_dist2(points, np.float32(r2 * 0.99), np.float32(r2 * 1.01)).astype(np.float64)
    if not len(near):
        return 0.01 / 2
    return float(np.abs(np.sqrt(near / r2) - 1.0).min())


def clear_radius(points, about):
    """a float32 radius near `about` in the widest gap between two consecutive pair distances within 2 % of it"""
    lo, hi = np.float64(about) * 0.98, np.float64(about) * 1.02
    d = np.sqrt(pair_dist2(points, np.float32(lo * lo), np.float32(hi * hi)).astype(np.float64))
    d = np.concatenate([[lo], d[(d > lo) & (d < hi)], [hi]])
    k = int(np.argmax(np.diff(np.log(d))))
    return np.float32(math.sqrt(d[k] * d[k + 1]))


def scores(idx, dist2, labels=None, num_groups=1):
    """idx (P, K) integers, dist2 (P, K) float32, labels (P,) integers or None -> score (P,) float32"""
    idx = np.asarray(idx)
    dist2 = np.asarray(dist2, np.float32)
    P, K = idx.shape
    g = np.zeros(P, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    assert labels is not None or num_groups == 1
    out = np.full(P, np.inf, np.float32)
    for i in range(P):
        if not 0 <= g[i] < num_groups:
            continue
        total, n = np.float64(0), 0
        for s in range(K):
            j, d = int(idx[i, s]), dist2[i, s]
            if not 0 <= j < P or j == i or g[j] != g[i] or not d < np.inf:
                continue
            total = total + np.sqrt(np.float64(d))        # slot order, one rounding per operation
            n += 1
        if n:
            out[i] = np.float32(total / np.float64(n))
    return out


def group_of(labels, P, num_groups):
    """(P,) int64: the group of every point, -1 for a point that is no member"""
    g = np.zeros(P, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    return np.where((g >= 0) & (g < num_groups), g, -1)


def outliers(idx, dist2, labels=None, num_groups=1, ratio=2.0, sc=None):
    """-> score (P,) float32, keep (P,) bool, stats (G, 4) float64 {n, mean, std, threshold}; sc: scores() of the same, if at hand"""
    sc = scores(idx, dist2, labels, num_groups) if sc is None else sc
    P = len(sc)
    g = group_of(labels, P, num_groups)
    stats = np.zeros((num_groups, 4), np.float64)
    r = float(np.float32(ratio))
    for q in range(num_groups):
        v = [float(x) for x in sc[(g == q) & (sc < np.inf)]]
        n = len(v)
        if n == 0:
            continue
        mean = math.fsum(v) / n
        std = math.sqrt(math.fsum((x - mean) * (x - mean) for x in v) / (n - 1)) if n >= 2 else 0.0
        stats[q] = (n, mean, std, mean + r * std)
    keep = np.zeros(P, bool)
    m = (g >= 0) & (sc < np.inf)
    keep[m] = sc[m].astype(np.float64) <= stats[g[m], 3]
    return sc, keep, stats


def threshold_clearance(sc, labels, num_groups, stats):
    """min over the finite scores of |score - threshold| / (n 2^-50 (mean + std)) of its group (inf if there is none): above 1 the
    comparison score <= threshold has one answer for every threshold within the error bound of an fp64 evaluation in any order"""
    g = group_of(labels, len(sc), num_groups)
    m = (g >= 0) & (sc < np.inf)
    if not m.any():
        return math.inf
    n, mean, std, thr = (stats[g[m], c] for c in range(4))
    with np.errstate(divide="ignore"):
        return float((np.abs(sc[m].astype(np.float64) - thr) / (n * 2.0 ** -50 * (mean + std))).min())
