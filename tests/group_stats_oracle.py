"""TEST INFRASTRUCTURE - numpy fp64 restatement of the group statistics and the group merge (csrc/group_stats.hip; include/f3dgs.h:
f3dgs_group_stats, f3dgs_group_merge): the contract as array expressions, group by group, and for every float output the BOUND
the GPU test uses - derived, not measured.

The bound of a value S / M, S a sum of n terms t_k and M the mass (n terms as well):
    bar = ulp32(want) + 4 n 2^-53 sum|t_k| / M
Any two fp64 summation orders each lie within (n - 1) 2^-53 sum|t_k| of the true sum (the terms w x and w f are exact products of
two float32 values); the same holds for M, and the factor 4 covers the four; the final rounding to float32 moves one ulp when the
two fp64 quotients straddle a rounding boundary.  For cov the terms are w d_a d_b about THIS judge's centroid, and the kernel's
fp64 centroid differs from it by at most delta (the fp64 part of the centroid's bound: the second pass centres on the fp64
centroid, not on its float32 rounding), which moves the sum by |delta_a| sum w|d_b| / M + |delta_b| sum w|d_a| / M + |delta_a delta_b|."""
import numpy as np

U = 2.0 ** -53
COV_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))          # xx xy xz yy yz zz: the reference's strip_symmetric order


def ulp32(v):
    """the spacing of float32 at |v| (fp64 array); 0 where v is not finite"""
    a = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.spacing(a).astype(np.float64)
    return np.where(np.isfinite(s), s, 0.0)


def members(groups, xyz, G, weight=None):
    """(P,) bool: 0 <= id < G, finite coordinates, 0 < weight < inf (a NaN weight: no member)"""
    g = np.asarray(groups).astype(np.int64)
    ok = (g >= 0) & (g < G) & np.isfinite(np.asarray(xyz, np.float32)).all(axis=1)
    if weight is not None:
        w = np.asarray(weight, np.float32)
        with np.errstate(invalid="ignore"):
            ok &= (w > 0) & (w < np.inf)
    return ok


def order_key(v):
    """the order-preserving map of float32 bits onto integers: -0 < +0"""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b >> 31, b ^ 0xFFFFFFFF, b ^ 0x80000000)


def group_stats(groups, xyz, G, weight=None, features=None):
    """A dict: count (G,) int64; mass (G,), centroid (G, 3), cov (G, 6), aabb (G, 6), feature_mean (G, C) float32 (None without
    features); mass_bar, centroid_bar, cov_bar, feature_bar: the bounds, fp64, same shapes."""
    g = np.asarray(groups).astype(np.int64)
    x32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    P = len(g)
    w32 = np.ones(P, np.float32) if weight is None else np.asarray(weight, np.float32)
    f32 = None if features is None else np.asarray(features, np.float32)
    assert f32 is None or (f32.ndim == 2 and len(f32) == P)
    C = 0 if f32 is None else f32.shape[1]
    ok = members(g, x32, G, weight)
    out = dict(count=np.zeros(G, np.int64), mass=np.zeros(G, np.float32), centroid=np.zeros((G, 3), np.float32),
               cov=np.zeros((G, 6), np.float32), aabb=np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, np.float32), (G, 1)),
               feature_mean=None if f32 is None else np.zeros((G, C), np.float32),
               mass_bar=np.zeros(G), centroid_bar=np.zeros((G, 3)), cov_bar=np.zeros((G, 6)),
               feature_bar=None if f32 is None else np.zeros((G, C)))
    rows = np.flatnonzero(ok)
    rows = rows[np.argsort(g[rows], kind="stable")]
    ids, first = np.unique(g[rows], return_index=True)
    for k, gid in enumerate(ids):
        sel = rows[first[k]:first[k + 1] if k + 1 < len(ids) else len(rows)]
        n = len(sel)
        w = w32[sel].astype(np.float64)
        x = x32[sel].astype(np.float64)
        M = w.sum()
        out["count"][gid] = n
        out["mass"][gid] = np.float32(M)
        out["mass_bar"][gid] = ulp32(M) + 4 * n * U * M
        wx = w[:, None] * x
        c = wx.sum(0) / M
        out["centroid"][gid] = c.astype(np.float32)
        delta = 4 * n * U * np.abs(wx).sum(0) / M
        out["centroid_bar"][gid] = ulp32(c) + delta
        d = x - c
        wd = (w[:, None] * np.abs(d)).sum(0) / M
        for q, (a, b) in enumerate(COV_PAIRS):
            t = w * d[:, a] * d[:, b]
            v = t.sum() / M if n > 1 else 0.0
            out["cov"][gid, q] = np.float32(v)
            out["cov_bar"][gid, q] = ulp32(v) + 4 * n * U * np.abs(t).sum() / M + delta[a] * wd[b] + delta[b] * wd[a] + delta[a] * delta[b]
        key = order_key(x32[sel])
        lo, hi = key.argmin(0), key.argmax(0)
        for a in range(3):
            out["aabb"][gid, a] = x32[sel[lo[a]], a]
            out["aabb"][gid, 3 + a] = x32[sel[hi[a]], a]
        if f32 is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                t = w[:, None] * f32[sel].astype(np.float64)
                v = t.sum(0) / M                                   # a non-finite element propagates into its channel
                out["feature_mean"][gid] = v.astype(np.float32)
                bar = ulp32(v) + 4 * n * U * np.abs(t).sum(0) / M
            out["feature_bar"][gid] = np.where(np.isfinite(v), bar, 0.0)
    return out


FLOAT_FIELDS = (("mass", "mass_bar"), ("centroid", "centroid_bar"), ("cov", "cov_bar"), ("feature_mean", "feature_bar"))


def within(got, want, bar):
    """elementwise: |got - want| <= bar in fp64; a non-finite `want` needs the same value (NaN matches NaN)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        near = np.abs(got - want) <= bar
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return np.where(np.isfinite(want), near, same)


# ---- the merge ----------------------------------------------------------------------------------------------------------------

def adjacency(groups, idx, G, dist2=None, max_dist2=np.inf, mutual=False):
    """The adjacent pairs of groups as an (E, 2) int64 array (a, b), a < b, each once, ascending."""
    g = np.asarray(groups).astype(np.int64)
    idx = np.asarray(idx).astype(np.int64)
    P, K = idx.shape
    rows = np.repeat(np.arange(P, dtype=np.int64), K).reshape(P, K)
    ok = (idx >= 0) & (idx < P) & (idx != rows)
    j = np.where(ok, idx, 0)
    inside = (g >= 0) & (g < G)
    ok &= inside[rows] & inside[j] & (g[rows] != g[j])
    limit = np.float32(max_dist2)
    if limit < np.inf:
        with np.errstate(invalid="ignore"):
            ok &= np.asarray(dist2, np.float32) <= limit           # a NaN distance: no edge
    directed = set(zip(rows[ok].tolist(), j[ok].tolist()))          # i -> j
    if mutual:
        directed = {(a, b) for a, b in directed if (b, a) in directed}
    pairs = {(min(g[a], g[b]), max(g[a], g[b])) for a, b in directed}
    return np.array(sorted(pairs), np.int64).reshape(-1, 2)


def cosines(pairs, feature_mean):
    """fp64 on the float32 rows: dot(a, b) / sqrt(dot(a, a) dot(b, b)); NaN for a zero norm"""
    m = np.asarray(feature_mean, np.float32).astype(np.float64)
    a, b = m[pairs[:, 0]], m[pairs[:, 1]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        aa, bb = (a * a).sum(1), (b * b).sum(1)
        cos = (a * b).sum(1) / np.sqrt(aa * bb)
    return np.where((aa > 0) & (bb > 0), cos, np.nan)


def group_merge(groups, idx, feature_mean, min_cos, dist2=None, max_dist2=np.inf, mutual=False):
    """(groups_out (P,), group_root (G,)) int64.  Asserts the condition under which the result is a function of the inputs alone:
    no adjacent pair's cosine within 8 C 2^-53 of min_cos."""
    fm = np.asarray(feature_mean, np.float32)
    G, C = fm.shape
    pairs = adjacency(groups, idx, G, dist2, max_dist2, mutual)
    cos = cosines(pairs, fm)
    near = np.abs(cos - np.float32(min_cos).astype(np.float64)) <= 8 * C * U
    assert not near.any(), f"the cosine of groups {pairs[near][0]} lies within rounding of min_cos: choose other inputs"
    with np.errstate(invalid="ignore"):
        e = pairs[cos >= np.float64(np.float32(min_cos))]
    root = np.arange(G, dtype=np.int64)
    for _ in range(G + 1):                                          # min-label propagation with pointer jumping
        old = root.copy()
        if len(e):
            np.minimum.at(root, e[:, 0], old[e[:, 1]])
            np.minimum.at(root, e[:, 1], old[e[:, 0]])
        root = root[root]
        if np.array_equal(root, old):
            break
    else:
        raise AssertionError("no fixed point")
    g = np.asarray(groups).astype(np.int64)
    inside = (g >= 0) & (g < G)
    return np.where(inside, root[np.where(inside, g, 0)], -1), root
