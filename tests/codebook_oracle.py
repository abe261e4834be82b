"""The judge of the feature codebooks (csrc/codebook.hip; codebook.py), in numpy fp64.  No GPU, no product code.

The device takes score_ik = |c_k|^2 - 2 x_i.c_k (L2) or -x_i.c^_k (cosine) as ONE fp32 fmaf chain over the channels, with |c_k|^2
(or c^_k) rounded once from fp64 and one more rounding for the score: with u = 2^-24 it differs from the fp64 score by at most
    e_ik = (C + 2) u (2 sum_c |x_ic c_kc| + |c_k|^2)          (cosine: (C + 2) u sum_c |x_ic c^_kc|)
(gamma_C of the chain, to first order, and the two single roundings).  A device code k^ is therefore RIGHT iff
    s_ik^ - e_ik^ <= s_ik* + e_ik*,      k* the fp64 arg-min with ties to the lowest k
and the number of rows with k^ != k* is bounded separately (1 % on random-normal data), so that the allowance cannot hide a
broken epilogue.  Everything else the device computes in fp64 and rounds once: a value that sums n terms t lies within
ulp32(v) / 2 + 4 n 2^-53 sum|t| of the judge's."""
import numpy as np

U = 2.0 ** -24
METRICS = ("l2", "cosine")
MUL, ADD = 2654435761, 40503          # the reseeding rule: row (k * MUL + iteration * ADD) mod P, in uint64


def finite_rows(a):
    return np.isfinite(np.asarray(a, np.float64)).all(axis=1)


def unit_rows(cent):
    """c / |c| in fp64; zeros for a zero row"""
    c = np.asarray(cent, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt((c * c).sum(1))
    out = np.zeros_like(c)
    ok = np.isfinite(n) & (n > 0)
    out[ok] = c[ok] / n[ok, None]
    return out


def scores(x, cent, metric="l2"):
    """(s (P, K) fp64 scores - +inf for a centroid with a non-finite element -, e (P, K) the device's allowance).  Rows of x that
    are not finite hold garbage: assign() never looks at them."""
    assert metric in METRICS
    x = np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    c = np.asarray(cent, np.float64)
    good = finite_rows(c)
    c = np.where(good[:, None], c, 0.0)
    C = x.shape[1]
    if metric == "cosine":
        c = unit_rows(c)
        s = -(x @ c.T)
        e = (C + 2) * U * (np.abs(x) @ np.abs(c).T)
    else:
        n2 = (c * c).sum(1)
        s = n2[None, :] - 2.0 * (x @ c.T)
        e = (C + 2) * U * (2.0 * (np.abs(x) @ np.abs(c).T) + n2[None, :])
    s[:, ~good] = np.inf
    e[:, ~good] = 0.0
    return s, e


def assign(x, cent, metric="l2"):
    """the fp64 codes k* (P,) int32: ties to the lowest k, -1 for a row that is not finite and where no centroid is finite"""
    s, _ = scores(x, cent, metric)
    k = np.argmin(s, axis=1).astype(np.int32) if s.shape[0] else np.zeros(0, np.int32)          # (the first minimum: the lowest k)
    none = ~finite_rows(x) | ~np.isfinite(s[np.arange(len(k)), k])
    k[none] = -1
    return k


def adjudicate(codes, x, cent, metric="l2"):
    """(right (P,) bool, differs (P,) bool): a device code is right iff it equals k* or its score is within the allowances of
    k*'s; where k* is -1 only -1 is right."""
    codes = np.asarray(codes)
    s, e = scores(x, cent, metric)
    star = assign(x, cent, metric)
    P, K = s.shape
    right = codes == star
    maybe = (star >= 0) & (codes >= 0) & (codes < K) & ~right
    i = np.nonzero(maybe)[0]
    kh, ks = codes[i], star[i]
    right[i] = np.isfinite(s[i, kh]) & (s[i, kh] - e[i, kh] <= s[i, ks] + e[i, ks])
    return right, codes != star


def clear_of_rounding(x, cent, metric="l2"):
    """(P,) bool: the fp64 winner beats every other centroid by more than both allowances - the device has no choice"""
    s, e = scores(x, cent, metric)
    star = assign(x, cent, metric)
    ok = np.ones(len(star), bool)
    for i in np.nonzero(star >= 0)[0]:
        hi = s[i, star[i]] + e[i, star[i]]
        lo = s[i] - e[i]
        lo[star[i]] = np.inf
        ok[i] = hi < lo.min() if len(lo) > 1 else True
    return ok


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def dist2(x, cent, codes, metric="l2"):
    """(d (P,) fp64, bound (P,)): sum (x - c)^2 of the given codes, or 1 - cos; 0 for code -1"""
    x, c, codes = np.asarray(x, np.float64), np.asarray(cent, np.float64), np.asarray(codes)
    P, C = x.shape
    d, terms = np.zeros(P), np.zeros(P)
    m = codes >= 0
    xm, cm = x[m], c[codes[m]]
    if metric == "cosine":
        xx, cc = (xm * xm).sum(1), (cm * cm).sum(1)
        ok = (xx > 0) & (cc > 0)
        den = np.where(ok, np.sqrt(xx * cc), 1.0)
        d[m] = 1.0 - np.where(ok, (xm * cm).sum(1) / den, 0.0)
        terms[m] = 1.0 + np.where(ok, np.abs(xm * cm).sum(1) / den, 0.0)
    else:
        d[m] = ((xm - cm) ** 2).sum(1)
        terms[m] = d[m]
    return d, ulp32(d) / 2 + 4 * C * 2.0 ** -53 * terms


def member(codes, K, w=None):
    codes = np.asarray(codes)
    m = (codes >= 0) & (codes < K)
    if w is not None:
        w = np.asarray(w, np.float64)
        with np.errstate(invalid="ignore"):
            m &= (w > 0) & (w < np.inf)
    return m


def inertia(d32, codes, K, w=None):
    """the fp64 sum of w * dist2 over the device's own fp32 dist2"""
    m = member(codes, K, w)
    ww = np.ones(len(d32)) if w is None else np.asarray(w, np.float64)
    return float((ww[m] * np.asarray(d32, np.float64)[m]).sum())


def update(x, codes, cent, metric="l2", w=None, reseed=False, iteration=0):
    """(centroids (K, C) float32: the fp64 result rounded once, count (K,) int64, the fp64 result, bound (K, C): what a device
    value may differ from the fp64 result by)"""
    x, old = np.asarray(x, np.float64), np.asarray(cent, np.float32)
    P, C = x.shape
    K = old.shape[0]
    m = member(codes, K, w)
    ids = np.asarray(codes)[m]
    ww = (np.ones(P) if w is None else np.asarray(w, np.float64))[m]
    mass = np.bincount(ids, ww, K)
    count = np.bincount(ids, minlength=K).astype(np.int64)
    sums, mags = np.zeros((K, C)), np.zeros((K, C))
    np.add.at(sums, ids, ww[:, None] * x[m])
    np.add.at(mags, ids, np.abs(ww[:, None] * x[m]))
    out64 = old.astype(np.float64)
    bound = np.zeros((K, C))
    have = mass > 0
    mean = sums[have] / mass[have, None]
    b = 4 * count[have, None] * 2.0 ** -53 * mags[have] / mass[have, None]
    if metric == "cosine":
        n = np.sqrt((mean * mean).sum(1))
        ok = n > 0
        n1 = np.where(ok, n, 1.0)[:, None]
        unit = mean / n1
        b = np.where(ok[:, None], b / n1 + np.abs(unit) * (np.abs(mean) * b).sum(1)[:, None] / n1 ** 2 + 4 * C * 2.0 ** -53 * np.abs(unit), b)
        mean = unit
    out64[have] = mean
    bound[have] = b
    if reseed and P > 0:
        for k in np.nonzero(~have)[0]:
            row = (int(k) * MUL + int(iteration) * ADD) % P
            if np.isfinite(x[row]).all():
                out64[k] = x[row]
    out = out64.astype(np.float32)
    return out, count, out64, bound + ulp32(out64) / 2


def init_rows(P, K):
    return (np.arange(K, dtype=np.int64) * P) // K


def lloyd(x, k, iterations, metric="l2", init=None, w=None, fit_stride=1, reseed=True):
    """The judge's own k-means on data it can decide: every assign must be exact (integer-valued operands small enough that every
    fp32 product and sum is exact) or clear of rounding, else AssertionError.  Returns dict(centroids float32, codes, count, moved)."""
    x32 = np.asarray(x, np.float32)
    fit = x32[::fit_stride]
    wf = None if w is None else np.asarray(w, np.float32)[::fit_stride]
    cent = (fit[init_rows(len(fit), k)] if init is None else np.asarray(init, np.float32)).copy()
    prev = np.full(len(fit), -1, np.int32)
    moved = []

    def decided(rows, cent):
        exact = all(np.array_equal(a, np.round(a)) and np.abs(a[np.isfinite(a)]).max(initial=0) <= 8 for a in (rows, cent)) \
            and rows.shape[1] <= 64
        assert exact or clear_of_rounding(rows, cent, metric).all(), "the judge cannot decide this case: a score within rounding of the best"
        return assign(rows, cent, metric)

    for it in range(iterations):
        codes = decided(fit, cent)
        moved.append(int((codes != prev).sum()))
        prev = codes
        cent = update(fit, codes, cent, metric, wf, reseed, it)[0]
    codes = decided(x32, cent)
    return dict(centroids=cent, codes=codes, count=np.bincount(codes[codes >= 0], minlength=k).astype(np.int64),
                moved=np.array(moved, np.int32))


def scores32(x, cent, metric="l2"):
    """the device's scores restated in float32 numpy (any summation order obeys the same bound): (P, K) float32"""
    x = np.asarray(x, np.float32)
    c64 = np.asarray(cent, np.float64)
    if metric == "cosine":
        return -(x @ unit_rows(c64).astype(np.float32).T)
    n2 = (c64 * c64).sum(1).astype(np.float32)
    return (np.float32(-2) * (x @ np.asarray(cent, np.float32).T) + n2[None, :]).astype(np.float32)


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------------------------------

# (P, K, C): a covering subset of P in {0, 1, 31, 32, 33, 127, 128, 129, 257, 1000} x K in {1, 2, 31, 32, 33, 127, 128, 129, 300}
# x C in {1, 3, 16, 31, 32, 33, 64, 128, 129, 512} - every value at least once, every tile edge of the kernel (32 rows a wave, 128
# a workgroup, 32 centroids a sub-tile, 128 a tile, 32 channels a chunk, 4 a vector load) from both sides - and the two limits
SHAPES = [(0, 2, 3), (1, 1, 1), (31, 2, 3), (32, 31, 16), (33, 32, 31), (127, 33, 32), (128, 127, 33), (129, 128, 64),
          (257, 129, 128), (1000, 300, 129), (129, 2, 512), (1000, 31, 3), (33, 300, 16), (257, 32, 1), (128, 1, 64), (1000, 128, 32),
          (64, 65536, 4), (33, 2, 4096)]
MAX_DIFFERENT = 0.01                  # the share of rows whose code may differ from k* on random-normal data


def random_case(P, K, C, seed=0):
    """random-normal features (P, C) and centroids (K, C), float32"""
    g = np.random.default_rng([P, K, C, seed])
    return g.normal(0, 1, (P, C)).astype(np.float32), g.normal(0, 1, (K, C)).astype(np.float32)


def integer_blobs(P, K, C, seed=0, spread=1):
    """integer-valued rows, |v| <= 8: K centres with coordinates in {-6, 0, 6}, a row = a centre + integers in [-spread, spread];
    returns (x (P, C) float32, centres (K, C) float32, the centre of every row)"""
    g = np.random.default_rng([P, K, C, seed, 7])
    centres = np.unique(g.integers(-1, 2, (4 * K + 8, C)) * 6, axis=0)
    g.shuffle(centres)
    centres = centres[:K]
    assert len(centres) == K, "not enough distinct centres"
    which = g.integers(0, K, P)
    x = centres[which] + g.integers(-spread, spread + 1, (P, C))
    return x.astype(np.float32), centres.astype(np.float32), which
