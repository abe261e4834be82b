"""TEST INFRASTRUCTURE - numpy restatement of the neighbourhood kernels (csrc/neighbors.hip), as plain as it gets.

knn: brute force in float32 with the kernel's operation order - dx = candidate - query, ((dx*dx) + (dy*dy)) + (dz*dz), one rounding
per operation -, the order by lexsort on (distance, index), self excluded by index, a distance that is not < inf excluded, a
non-finite point without neighbours and nobody's neighbour, missing neighbours as (-1, FLT_MAX).
mode_filter: the vote of include/f3dgs.h (f3dgs_label_mode_filter) as a loop over the Gaussians."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max


def knn(points, K, chunk=512):
    """points (P, 3) float32 -> idx (P, K) int32, dist2 (P, K) float32"""
    p = np.ascontiguousarray(points, np.float32)
    P = p.shape[0]
    idx = np.full((P, K), -1, np.int32)
    dist2 = np.full((P, K), FLT_MAX, np.float32)
    if P == 0:
        return idx, dist2
    finite = np.isfinite(p).all(1)
    cols = np.arange(P)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, P, chunk):
            q = p[a:a + chunk]
            dx = p[None, :, 0] - q[:, None, 0]
            dy = p[None, :, 1] - q[:, None, 1]
            dz = p[None, :, 2] - q[:, None, 2]
            d = ((dx * dx) + (dy * dy)) + (dz * dz)
            assert d.dtype == np.float32
            for r in range(q.shape[0]):
                i = a + r
                if not finite[i]:
                    continue
                ok = finite & (cols != i) & (d[r] < np.inf)
                cand = cols[ok]
                order = np.lexsort((cand, d[r][ok]))[:K]      # by distance, then by index
                n = len(order)
                idx[i, :n] = cand[order]
                dist2[i, :n] = d[r][ok][order]
    return idx, dist2


def mode_filter_step(labels, idx, weight=None, dist2=None, max_dist2=np.inf, fill=True):
    """One Jacobi step.  labels (P,) integers, idx (P, K), weight (P,) float32 or None, dist2 (P, K) float32 or None.
    Returns labels_out (P,) int64 and share (P,) float32."""
    labels = np.asarray(labels).astype(np.int64)
    idx = np.asarray(idx)
    P, K = idx.shape
    w_all = None if weight is None else np.asarray(weight, np.float32)
    limit = np.float32(max_dist2)
    out = np.full(P, -1, np.int64)
    share = np.zeros(P, np.float32)
    for i in range(P):
        voters = [(i, True)] + [(int(idx[i, s]), bool(np.isinf(limit)) or bool(np.float32(dist2[i, s]) <= limit)) for s in range(K)]
        score = {}          # label -> float32 sum in voter order
        total = np.float32(0)
        for j, near in voters:
            if not near or not 0 <= j < P or labels[j] < 0:
                continue
            w = np.float32(1) if w_all is None else w_all[j]
            if not (w > 0 and w < np.inf):
                continue
            score[labels[j]] = np.float32(score.get(labels[j], np.float32(0)) + w)
            total = np.float32(total + w)
        if not score or (not fill and labels[i] < 0):
            continue
        top = max(score.values())
        tied = sorted(l for l, s in score.items() if s == top)
        out[i] = labels[i] if labels[i] in tied else tied[0]
        share[i] = np.float32(top) / np.float32(total)
    return out, share


def mode_filter(labels, idx, weight=None, dist2=None, max_dist2=np.inf, fill=True, iterations=1):
    share = None
    for _ in range(iterations):
        labels, share = mode_filter_step(labels, idx, weight, dist2, max_dist2, fill)
    return labels, share
