"""fp64 judge of the contribution pass (csrc/contrib.hip): a numpy walk over the CPU oracle's forward state.

`walk` reads what `oracle.oracle.Oracle.read` exposes after a forward call - means2D, conic_opacity, depths, point_list,
ranges, n_contrib - and re-walks every pixel's tile list in float64 with the reference's formulas (forward.cu:336-377).  The
set of contributors is the oracle's own n_contrib, as the pass takes the product forward's.  It returns, per pixel, alpha =
1 - T, the median depth (the float32 depth of the first blended entry after which T < 0.5, else 0), the index and weight of the
entry of largest weight, the second largest weight, and a `borderline` flag; and per Gaussian the float64 sums
acc[g, k] = sum_p w masks[k, p] (k < K) and acc[g, K] = sum_p w, the largest weight wmax[g] and the pixel it is reached at.

A pixel is borderline when a discrete decision of the walk sits within float32 round-off of its threshold, so that a correct
float32 implementation may decide it the other way:
  * an entry up to and including position n_contrib with |255 alpha - 1| <= 1e-4 or 0 < power < 1e-6;
  * the entry that ends the walk with T (1 - alpha) within 1e-3 relative of 1e-4;
  * the two largest weights within 1e-4 relative of each other;
  * some prefix T within 1e-5 of 0.5.
"""
from __future__ import annotations

import numpy as np

TILE = 16


def oracle_state(o) -> dict:
    """The arrays `walk` needs, read from an Oracle after forward()."""
    return {k: o.read(k) for k in ("means2D", "conic_opacity", "depths", "point_list", "ranges", "n_contrib", "final_T")}


def walk(state: dict, W: int, H: int, masks=None) -> dict:
    means = state["means2D"].astype(np.float64).reshape(-1, 2)
    co = state["conic_opacity"].astype(np.float64).reshape(-1, 4)
    depths = state["depths"].astype(np.float32)
    plist = state["point_list"]
    ranges = state["ranges"].reshape(-1, 2)
    ncon = state["n_contrib"].astype(np.int64)
    P = len(depths)
    K = 0 if masks is None else int(masks.shape[0])
    m64 = None if K == 0 else np.asarray(masks, np.float64).reshape(K, H * W)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    HW = H * W
    alpha_out = np.zeros(HW)
    median = np.zeros(HW, np.float32)
    ids = np.full(HW, -1, np.int64)
    top1, top2 = np.zeros(HW), np.zeros(HW)
    border = np.zeros(HW, bool)
    acc = np.zeros((P, K + 1))
    wmax, wpix = np.zeros(P), np.full(P, -1, np.int64)      # largest weight of a Gaussian, and the pixel it is reached at
    for t in range(gx * gy):
        tx, ty = t % gx, t // gx
        lo, hi = int(ranges[t, 0]), int(ranges[t, 1])
        ys, xs = np.meshgrid(np.arange(ty * TILE, min(H, (ty + 1) * TILE)), np.arange(tx * TILE, min(W, (tx + 1) * TILE)), indexing="ij")
        pix = (ys * W + xs).reshape(-1)
        fx, fy = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
        n = len(pix)
        nc = ncon[pix]
        T = np.ones(n)
        med = np.zeros(n, np.float32)
        best = np.full(n, -1, np.int64)
        w1, w2 = np.zeros(n), np.zeros(n)
        bl = np.zeros(n, bool)
        ended = np.zeros(n, bool)          # the entry that ends the walk has been seen
        mt = None if K == 0 else m64[:, pix]
        for k in range(lo, hi):
            pos = k - lo + 1
            g = int(plist[k])
            dx, dy = means[g, 0] - fx, means[g, 1] - fy
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            araw = co[g, 3] * np.exp(np.minimum(power, 0.0))
            alpha = np.minimum(0.99, araw)
            within = pos <= nc
            bl |= within & ((np.abs(255.0 * araw - 1.0) <= 1e-4) | ((power > 0.0) & (power < 1e-6)))
            valid = ~(power > 0.0) & ~(alpha < 1.0 / 255.0)
            if not valid.any():
                continue
            test_T = T * (1.0 - alpha)
            ok = valid & within
            after = valid & ~within & ~ended
            bl |= after & (np.abs(test_T - 1e-4) <= 1e-7)
            ended |= after
            if ok.any():
                w = np.where(ok, alpha * T, 0.0)
                cross = ok & (T >= 0.5) & (test_T < 0.5)
                med = np.where(cross, depths[g], med)
                T = np.where(ok, test_T, T)
                bl |= ok & (np.abs(T - 0.5) <= 1e-5)
                better = w > w1
                w2 = np.where(better, w1, np.maximum(w2, w))
                best = np.where(better, g, best)
                w1 = np.where(better, w, w1)
                acc[g, K] += w.sum()
                i = int(np.argmax(w))
                if w[i] > wmax[g]:
                    wmax[g], wpix[g] = w[i], pix[i]
                if K:
                    acc[g, :K] += mt @ w
            if (pos >= nc).all() and ended.all():
                break
        bl |= (w1 > 0) & (w1 - w2 <= 1e-4 * w1)
        alpha_out[pix], median[pix], ids[pix], top1[pix], top2[pix], border[pix] = 1.0 - T, med, best, w1, w2, bl
    shape = (H, W)
    return dict(alpha=alpha_out.reshape(shape), median_depth=median.reshape(shape), ids=ids.reshape(shape), top1=top1.reshape(shape),
                top2=top2.reshape(shape), borderline=border.reshape(shape), acc=acc, wmax=wmax, wmax_pixel=wpix)


def top_two(state: dict, W: int, H: int, pixels) -> dict:
    """{pixel: (id of the largest weight, id of the second largest)} for a handful of flat pixel indices - the slow, direct
    walk, for the borderline pixels only."""
    means = state["means2D"].astype(np.float64).reshape(-1, 2)
    co = state["conic_opacity"].astype(np.float64).reshape(-1, 4)
    plist, ranges, ncon = state["point_list"], state["ranges"].reshape(-1, 2), state["n_contrib"]
    gx = (W + TILE - 1) // TILE
    out = {}
    for p in pixels:
        y, x = divmod(int(p), W)
        t = (y // TILE) * gx + x // TILE
        lo = int(ranges[t, 0])
        T, ws = 1.0, []
        for pos in range(1, int(ncon[p]) + 1):
            g = int(plist[lo + pos - 1])
            dx, dy = means[g, 0] - x, means[g, 1] - y
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            if power > 0:
                continue
            a = min(0.99, co[g, 3] * np.exp(power))
            if a < 1.0 / 255.0:
                continue
            ws.append((a * T, -pos, g))
            T *= 1.0 - a
        ws.sort(reverse=True)
        out[int(p)] = tuple(g for _, _, g in ws[:2]) + (-1,) * (2 - min(2, len(ws)))
    return out
