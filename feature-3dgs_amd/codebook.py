"""Feature codebooks: nearest-centroid codes, k-means and product quantisation of the per-Gaussian semantic features.

The semantic features are the bulk of a Feature-3DGS model (C = 32 ... 512 floats per Gaussian beside 59 others), and the labels
the rest of the package reasons with come from a teacher (a label map, SAM instances).  This module shrinks the first and
replaces the second (csrc/codebook.hip behind include/f3dgs.h: f3dgs_codebook_assign, f3dgs_codebook_update):

    assign       the index of the nearest centroid per row (L2 or cosine), on the matrix pipe; the (P, K) scores never exist
    kmeans       Lloyd's iteration with a fixed iteration count: no host read, the whole call is capturable
    quantize     product quantisation: one codebook per equal column slice of the features, each slice read in place
    dequantize   the features back from the codes (a gather)

Groups without a teacher - the ids feed what lifted labels feed:

    cb = codebook.kmeans(gaussians.get_semantic_feature, 64, metric="cosine")
    idx, dist2 = neighbors.knn(xyz, 8)
    split = neighbors.split_labels(cb.codes.long(), idx, dist2=dist2, max_dist=0.1)
    kept = neighbors.drop_small(split.comp, idx, 50, dist2=dist2, max_dist=0.1)
    st = groups.group_stats(kept, xyz, int(split.n_comp), features=gaussians.get_semantic_feature)     # (the caller's host read)

A smaller model - 1M x 128 floats become 1M x 8 bytes and eight (256, 16) tables:

    q = codebook.quantize(gaussians.get_semantic_feature, 256, subspaces=8, narrow=True)
    gaussians.rewrite_semantic_feature(codebook.dequantize(q)[:, None, :])          # what a reader of the codes renders with

HIP only; no CPU fallback.  Nothing is read back to the host.
"""
from __future__ import annotations

import collections

import torch

from simple_knn import _C
from neighbors import _describe

MAX_CENTROIDS = 65536        # F3DGS_CODEBOOK_MAX_CENTROIDS
MAX_CHANNELS = 4096          # F3DGS_CODEBOOK_MAX_CHANNELS
METRICS = ("l2", "cosine")

Assignment = collections.namedtuple("Assignment", ["codes", "dist2", "inertia", "moved"])
Codebook = collections.namedtuple("Codebook", ["centroids", "codes", "count", "inertia", "moved"])
Quantized = collections.namedtuple("Quantized", ["codebooks", "codes", "count", "inertia", "moved"])


def _features2(features, name="features"):
    """the (P, C) view the kernels read: the model's (P, 1, C) tensor, a column slice and a row-strided view as they are"""
    if not torch.is_tensor(features) or features.device.type != "cuda":
        raise ValueError(f"{name} must live on a HIP device (got {_describe(features)}): the codebooks have no CPU path")
    f2 = features
    if f2.dim() == 3 and f2.shape[1] == 1:
        f2 = f2[:, 0, :]
    if f2.dtype != torch.float32 or f2.dim() != 2 or not 1 <= f2.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"{name}: a float32 (P, C) or (P, 1, C) tensor with 1 <= C <= {MAX_CHANNELS} expected, got {_describe(features)}")
    f2 = f2.detach()
    if (f2.shape[1] > 1 and f2.stride(1) != 1) or (f2.shape[0] > 1 and f2.stride(0) < f2.shape[1]):
        f2 = f2.contiguous()                          # (a transposed or expanded view: the kernels read rows)
    return f2


def _flags(metric):
    if metric not in METRICS:
        raise ValueError(f"metric = {metric!r}: one of {METRICS} expected")
    return _C.CODEBOOK_COSINE if metric == "cosine" else 0


def _centroids(centroids, x, name="centroids"):
    C = x.shape[1]
    if not torch.is_tensor(centroids) or centroids.dtype != torch.float32 or centroids.dim() != 2 or centroids.shape[1] != C \
            or centroids.device != x.device or not 1 <= centroids.shape[0] <= MAX_CENTROIDS:
        raise ValueError(f"{name}: a float32 (K, {C}) tensor on {x.device} with 1 <= K <= {MAX_CENTROIDS} expected, got {_describe(centroids)}")
    return centroids.detach().contiguous()


def _rows(t, x, dtype, name):
    P = x.shape[0]
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (P,) or t.device != x.device:
        raise ValueError(f"{name}: a {dtype} ({P},) tensor on {x.device} or None expected, got {_describe(t)}")
    return t.detach()


def assign(features, centroids, metric="l2", prev_codes=None, weight=None, return_dist2=False, out=None):
    """The nearest centroid of every row.  features: (P, C) or the model's (P, 1, C) float32 on the device; a column slice
    [:, a:b] and a row-strided view [::s] are read in place.  centroids: (K, C) float32.  metric "l2" minimises |c|^2 - 2 x.c,
    "cosine" maximises x . c / |c| (a zero centroid scores 0).  The dot products are one fp32 fmaf chain each, channels ascending;
    ties go to the lowest index; a row with a non-finite element gets -1, a centroid with one never wins.

    Returns codes (P,) int32 - written into `out` if given, which may be prev_codes.  With return_dist2 or prev_codes:
    Assignment(codes, dist2 (P,) float32: sum (x - c)^2 of the winner in fp64, rounded once (1 - cos under "cosine"; 0 for code
    -1), inertia: a 0-dim float64 device tensor, sum weight * dist2 over the rows with a code and 0 < weight < inf, moved: a 0-dim
    int32 device tensor, the rows whose code differs from prev_codes) - dist2 and inertia None without return_dist2, moved None
    without prev_codes.  `weight` (P,) float32 never changes a code."""
    x = _features2(features)
    cb = _centroids(centroids, x)
    flags = _flags(metric)
    prev = _rows(prev_codes, x, torch.int32, "prev_codes")
    w = _rows(weight, x, torch.float32, "weight")
    dst = _rows(out, x, torch.int32, "out")
    for name, t in (("prev_codes", prev), ("out", dst)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor expected, got strides {t.stride()} of {_describe(t)}")
    with torch.no_grad():
        inertia = torch.zeros(1, dtype=torch.float64, device=x.device) if return_dist2 else None
        moved = torch.zeros(1, dtype=torch.int32, device=x.device) if prev is not None else None
        codes, dist2 = _C.codebook_assign(x, cb, flags, prev, None if w is None else w.contiguous(), dst, bool(return_dist2), inertia, moved)
    if not return_dist2 and prev is None:
        return codes
    return Assignment(codes, dist2, None if inertia is None else inertia[0], None if moved is None else moved[0])


def update(features, codes, centroids, metric="l2", weight=None, reseed_empty=False, iteration=0):
    """One centroid move: returns (centroids (K, C) float32, count (K,) int64).  centroid k becomes the weighted mean of the rows
    with codes == k and 0 < weight < inf, every sum in fp64 and rounded once (normalised in fp64 under "cosine"); a centroid
    without members keeps its row, or with reseed_empty takes row (k * 2654435761 + iteration * 40503) mod P of the features
    (keeps it if that row is not finite).  The given centroids are not modified."""
    x = _features2(features)
    cb = _centroids(centroids, x).clone()
    flags = _flags(metric) | (_C.CODEBOOK_RESEED_EMPTY if reseed_empty else 0)
    c = _rows(codes, x, torch.int32, "codes")
    if c is None:
        raise ValueError(f"codes: a torch.int32 ({x.shape[0]},) tensor on {x.device} expected, got NoneType")
    w = _rows(weight, x, torch.float32, "weight")
    if not isinstance(iteration, int) or isinstance(iteration, bool) or iteration < 0:
        raise ValueError(f"iteration = {iteration!r}: a non-negative integer expected")
    with torch.no_grad():
        count = torch.empty(cb.shape[0], dtype=torch.int32, device=x.device)
        _C.codebook_update(x, c.contiguous(), None if w is None else w.contiguous(), cb, flags, iteration, count)
    return cb, count.long()


def kmeans(features, k, iterations=10, metric="l2", init=None, weight=None, fit_stride=1, reseed_empty=True):
    """Lloyd's iteration, `iterations` times (assign, update), then one assign of ALL rows against the final centroids.

    features as for assign.  init: (k, C) float32 centroids, or None for the rows floor(j * P' / k), j = 0 .. k - 1, of the rows
    fitted on.  fit_stride = s fits on the view features[::s] (P' rows, read in place; weight[::s] with it) - the closing assign
    is over every row.  weight, reseed_empty: as for update; the iteration number of the reseeding rule counts from 0.

    Returns Codebook(centroids (k, C) float32, codes (P,) int32 against them, count (k,) int64: the rows per code, inertia
    (iterations,) float64 and moved (iterations,) int32 on the device: per iteration, of its assign (before its update), the sum of
    weight * dist2 and the rows fitted on whose code changed - against -1 in iteration 0).  The iteration count is fixed: no host
    read, the whole call is capturable."""
    x = _features2(features)
    flags = _flags(metric)
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_CENTROIDS:
        raise ValueError(f"k = {k!r}: an integer in 1 .. {MAX_CENTROIDS} expected")
    if not isinstance(iterations, int) or isinstance(iterations, bool) or iterations < 0:
        raise ValueError(f"iterations = {iterations!r}: a non-negative integer expected")
    if not isinstance(fit_stride, int) or isinstance(fit_stride, bool) or fit_stride < 1:
        raise ValueError(f"fit_stride = {fit_stride!r}: a positive integer expected")
    w = _rows(weight, x, torch.float32, "weight")
    fit = x[::fit_stride] if fit_stride > 1 else x
    w_fit = None if w is None else (w[::fit_stride] if fit_stride > 1 else w).contiguous()
    n, dev = fit.shape[0], x.device
    with torch.no_grad():
        if init is None:
            if n < 1:
                raise ValueError(f"features: no row to take centroids from, got {_describe(features)} with fit_stride = {fit_stride}")
            cb = fit[(torch.arange(k, device=dev, dtype=torch.int64) * n) // k].contiguous()
        else:
            cb = _centroids(init, x, "init")
            if cb.shape[0] != k:
                raise ValueError(f"init: a float32 ({k}, {x.shape[1]}) tensor expected, got {_describe(init)}")
            cb = cb.clone()
        inertia = torch.zeros(iterations, dtype=torch.float64, device=dev)
        moved = torch.zeros(iterations, dtype=torch.int32, device=dev)
        codes_fit = torch.full((n,), -1, dtype=torch.int32, device=dev)
        step_flags = flags | (_C.CODEBOOK_RESEED_EMPTY if reseed_empty else 0)
        for it in range(iterations):
            _C.codebook_assign(fit, cb, flags, codes_fit, w_fit, codes_fit, False, inertia[it:it + 1], moved[it:it + 1])
            _C.codebook_update(fit, codes_fit, w_fit, cb, step_flags, it, None)
        codes, _ = _C.codebook_assign(x, cb, flags, None, None, None, False, None, None)
        count = torch.zeros(k, dtype=torch.int64, device=dev).scatter_add_(0, codes.clamp(min=0).long(), (codes >= 0).long())
    return Codebook(cb, codes, count, inertia, moved)


def quantize(features, k, subspaces=1, narrow=False, **kmeans_args):
    """Product quantisation: the C channels in `subspaces` = M equal column slices (C % M == 0), one kmeans(slice, k,
    **kmeans_args) each - a slice is read in place through the row stride.  An `init` is (M, k, C / M).

    Returns Quantized(codebooks (M, k, C / M) float32, codes (P, M), count (M, k) int64, inertia (M, iterations) float64, moved
    (M, iterations) int32).  codes are int32 with -1 for a row whose slice is not finite; with narrow=True they are uint8 for
    k <= 255 (255: no code) and int16 for k <= 32767."""
    x = _features2(features)
    C = x.shape[1]
    if not isinstance(subspaces, int) or isinstance(subspaces, bool) or subspaces < 1 or C % subspaces:
        raise ValueError(f"subspaces = {subspaces!r}: a positive divisor of C expected, got {_describe(features)}")
    M, d = subspaces, C // subspaces
    init = kmeans_args.pop("init", None)
    if init is not None and (not torch.is_tensor(init) or init.dim() != 3 or init.shape[0] != M):
        raise ValueError(f"init: a float32 ({M}, {k}, {d}) tensor expected, got {_describe(init)}")
    parts = [kmeans(x[:, m * d:(m + 1) * d], k, init=None if init is None else init[m], **kmeans_args) for m in range(M)]
    codes = torch.stack([p.codes for p in parts], dim=1)
    if narrow and k <= 255:
        codes = torch.where(codes < 0, torch.full_like(codes, 255), codes).to(torch.uint8)
    elif narrow and k <= 32767:
        codes = codes.to(torch.int16)
    return Quantized(torch.stack([p.centroids for p in parts]), codes, torch.stack([p.count for p in parts]),
                     torch.stack([p.inertia for p in parts]), torch.stack([p.moved for p in parts]))


def dequantize(q):
    """(P, C) float32 from quantize's result (or any object with codebooks (M, K, C / M) and codes (P, M)): row i is the
    concatenation of codebooks[m, codes[i, m]]; zeros where a slice has no code."""
    books, codes = q.codebooks, q.codes
    if not torch.is_tensor(books) or books.dtype != torch.float32 or books.dim() != 3:
        raise ValueError(f"codebooks: a float32 (M, K, C / M) tensor expected, got {_describe(books)}")
    M, K, d = books.shape
    if not torch.is_tensor(codes) or codes.dim() != 2 or codes.shape[1] != M or codes.device != books.device \
            or codes.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"codes: an integer (P, {M}) tensor on {books.device} expected, got {_describe(codes)}")
    idx = codes.long()
    none = (idx == 255) if codes.dtype == torch.uint8 else (idx < 0)
    none = none | (idx >= K)
    rows = books[torch.arange(M, device=books.device)[None, :], idx.clamp(0, K - 1)]          # (P, M, d)
    return torch.where(none[:, :, None], torch.zeros((), dtype=books.dtype, device=books.device), rows).reshape(codes.shape[0], M * d)


__all__ = ["MAX_CENTROIDS", "MAX_CHANNELS", "METRICS", "Assignment", "Codebook", "Quantized", "assign", "update", "kmeans", "quantize",
           "dequantize"]
