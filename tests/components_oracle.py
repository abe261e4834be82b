"""TEST INFRASTRUCTURE - numpy restatement of the component kernels (csrc/components.hip; include/f3dgs.h: f3dgs_knn_components,
f3dgs_component_filter), as plain as it gets: the edge rules as array expressions, the components by lowering every node onto the
smallest label among itself and its neighbours until nothing moves."""
import numpy as np


def active_of(P, labels):
    """(active (P,) bool, lab (P,) int64): labels None -> every node active with label 0"""
    if labels is None:
        return np.ones(P, bool), np.zeros(P, np.int64)
    lab = np.asarray(labels).astype(np.int64)
    assert lab.shape == (P,)
    return lab >= 0, lab


def edges(idx, labels=None, dist2=None, max_dist2=np.inf, mutual=False):
    """The undirected edges as an (E, 2) int64 array of pairs (i, j), i < j, each once, ascending."""
    idx = np.asarray(idx).astype(np.int64)
    P, K = idx.shape
    active, lab = active_of(P, labels)
    rows = np.repeat(np.arange(P, dtype=np.int64), K).reshape(P, K)
    ok = (idx >= 0) & (idx < P) & (idx != rows)
    j = np.where(ok, idx, 0)
    ok &= active[rows] & active[j] & (lab[rows] == lab[j])
    limit = np.float32(max_dist2)
    if limit < np.inf:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(dist2, np.float32) <= limit          # a NaN distance: no edge
    directed = set(zip(rows[ok].tolist(), j[ok].tolist()))         # i -> j
    if mutual:
        und = {(min(a, b), max(a, b)) for a, b in directed if (b, a) in directed}
    else:
        und = {(min(a, b), max(a, b)) for a, b in directed}
    return np.array(sorted(und), np.int64).reshape(-1, 2)


def components(idx, labels=None, dist2=None, max_dist2=np.inf, mutual=False):
    """root (P,), size (P,), comp (P,), comp_root (P,), n_comp - int64"""
    P = np.asarray(idx).shape[0]
    active, _ = active_of(P, labels)
    e = edges(idx, labels, dist2, max_dist2, mutual)
    root = np.where(active, np.arange(P, dtype=np.int64), -1)
    for _ in range(P + 1):                                         # min-label propagation with pointer jumping
        old = root.copy()
        if len(e):
            np.minimum.at(root, e[:, 0], old[e[:, 1]])
            np.minimum.at(root, e[:, 1], old[e[:, 0]])
        root[active] = root[root[active]]
        if np.array_equal(root, old):
            break
    else:
        raise AssertionError("no fixed point")
    size = np.zeros(P, np.int64)
    count = np.bincount(root[active], minlength=P) if P else np.zeros(0, np.int64)
    size[active] = count[root[active]]
    roots = np.flatnonzero(root == np.arange(P))
    rank = np.full(P, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    comp = np.where(active, rank[np.maximum(root, 0)], -1) if P else np.zeros(0, np.int64)
    comp_root = np.full(P, -1, np.int64)
    comp_root[:len(roots)] = roots
    return root, size, comp, comp_root, len(roots)


def component_filter(labels, root, size, min_size=1, largest=False, num_labels=0):
    """labels_out (P,) int64.  labels None: every node label 0."""
    P = len(root)
    active, lab = active_of(P, labels)
    out = np.full(P, -1, np.int64)
    best = {}                                                      # label -> (size, -root) of its best component
    for r in np.flatnonzero(np.asarray(root) == np.arange(P)):
        if active[r] and lab[r] < num_labels:
            best[lab[r]] = max(best.get(lab[r], (-1, 0)), (int(size[r]), -int(r)))
    for i in range(P):
        if not active[i] or size[i] < min_size:
            continue
        if largest and best.get(lab[i]) != (int(size[i]), -int(root[i])):
            continue
        out[i] = lab[i]
    return out


def clean(labels_or_mask, idx, min_size=1, largest=False, num_labels=0, dist2=None, max_dist2=np.inf, mutual=False):
    """drop_small / keep_largest of neighbors.py: labels -> int64 labels, a bool mask -> a bool mask"""
    a = np.asarray(labels_or_mask)
    if a.dtype == bool:
        lab = np.where(a, 0, -1)
        root, size = components(idx, lab, dist2, max_dist2, mutual)[:2]
        return component_filter(lab, root, size, min_size, largest, 1) >= 0
    lab = np.maximum(a.astype(np.int64), -1)
    root, size = components(idx, lab, dist2, max_dist2, mutual)[:2]
    return component_filter(lab, root, size, min_size, largest, num_labels)
