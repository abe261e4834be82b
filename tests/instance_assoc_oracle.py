"""fp64 judge of the instance association (csrc/instances.hip: f3dgs_instance_associate, f3dgs_instance_merge), in numpy.

One view's label vote, acc_view (P, M + 1), is set against the global accumulator acc (P, L + 1) of which `count` instance
slots are in use (include/f3dgs.h has the contract word for word):

  global_labels   gl[g]: the lowest index of the largest of acc[g][0..L), -1 when that maximum is <= 0
  overlap_table   T (M + 1, L + 1) in float64 over the Gaussians with acc_view[g][M] > 0: T[m][c] += acc_view[g][m] with c = gl[g]
                  or L; row M receives max(0, total - sum_m acc_view[g][m]) - that residual alone is formed in float32, in
                  ascending m, as the contract says
  match           from ANY table (the judge's own, or the device's: the decisions are then judged from what the device summed):
                  row / rowall / col sums, iou = T / ((row + col) - T), the best instance per mask (lowest l among equals), the
                  winner per instance (largest IoU, lowest m among equals), new ids in ascending m while they last
  merge           acc[g][mapping[m]] += acc_view[g][m] (targets in [0, L), repeats add up), acc[g][L] += total, seen rows only
  associate       overlap_table + match
"""
from __future__ import annotations

import numpy as np


def global_labels(acc, L):
    a = np.asarray(acc)[:, :L]
    if a.shape[0] == 0:
        return np.zeros(0, np.int64)
    gl = a.argmax(1)                                   # the first of equal maxima
    return np.where(a.max(1) > 0, gl, -1)


def overlap_table(acc_view, acc, M, L):
    av = np.asarray(acc_view, np.float32).reshape(-1, M + 1)
    T = np.zeros((M + 1, L + 1))
    seen = av[:, M] > 0
    if not seen.any():
        return T
    gl = global_labels(np.asarray(acc).reshape(-1, L + 1)[seen], L)
    c = np.where(gl < 0, L, gl)
    v = av[seen]
    np.add.at(T[:M].T, c, v[:, :M].astype(np.float64))                   # T[m][c[g]] += v[g][m] (a view: added in place)
    s = np.cumsum(v[:, :M], axis=1, dtype=np.float32)[:, -1]             # sequential float32 sum in ascending m
    rest = np.maximum(np.float32(0), v[:, M] - s).astype(np.float64)
    np.add.at(T[M], c, rest)
    return T


def iou_table(T, M, L, count):
    """(iou (M, count), rowall (M)) in float64 from a table of any float type"""
    T = np.asarray(T, np.float64)
    row = np.array([T[m, :L].sum() for m in range(M)])
    rowall = row + T[:M, L]
    col = T[:, :count].sum(0)
    x = T[:M, :count]
    den = (row[:, None] + col[None, :]) - x
    iou = np.where(den == 0, 0.0, x / np.where(den == 0, 1.0, den))
    return iou, rowall


def match(T, M, L, count, iou_thresh=0.5, min_weight=0.0):
    """-> dict(mapping, best_label, best_iou, count, dropped (the increase), gap): gap is the smallest distance of a decision
    from going the other way - best against second best IoU of a mask, best IoU against iou_thresh, a winner against the next
    claimant, rowall against min_weight - or inf where there is none.  A tie decided by the index rules counts as gap 0.  A
    mask whose IoUs are all exactly 0, or whose rowall is exactly 0, is left out of the gap: a sum of zeros is 0 in any order."""
    iou, rowall = iou_table(T, M, L, count)
    best_label = np.full(M, -1, np.int64)
    best_iou = np.zeros(M)
    gap = np.inf
    if count > 0:
        best_label = iou.argmax(1)                     # the lowest l of the largest
        best_iou = iou.max(1)
        best_label = np.where(best_iou > 0, best_label, -1)
        live = best_iou > 0
        if count > 1 and live.any():
            top = np.sort(iou[live], 1)
            gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
        gap = min(gap, float(np.abs(best_iou - iou_thresh).min()))
    mapping = np.full(M, -1, np.int64)
    claims = (best_label >= 0) & (best_iou >= iou_thresh)
    for l in np.unique(best_label[claims]):
        ms = np.flatnonzero(claims & (best_label == l))
        q = best_iou[ms]
        mapping[ms[q.argmax()]] = l                    # the lowest m of the largest
        if len(ms) > 1:
            top = np.sort(q)
            gap = min(gap, float(top[-1] - top[-2]))
    if (rowall != 0).any():
        gap = min(gap, float(np.abs(rowall[rowall != 0] - min_weight).min()))
    new_count, dropped = int(count), 0
    for m in range(M):
        if mapping[m] >= 0 or not rowall[m] > min_weight:
            continue
        if new_count < L:
            mapping[m] = new_count
            new_count += 1
        else:
            dropped += 1
    return dict(mapping=mapping, best_label=best_label, best_iou=best_iou, count=new_count, dropped=dropped, gap=gap)


def associate(acc_view, acc, M, L, count, iou_thresh=0.5, min_weight=0.0):
    T = overlap_table(acc_view, acc, M, L)
    out = match(T, M, L, count, iou_thresh, min_weight)
    out["table"] = T
    return out


def merge(acc_view, mapping, acc, M, L):
    """the merged accumulator in float64 (the inputs are left alone)"""
    av = np.asarray(acc_view, np.float64).reshape(-1, M + 1)
    out = np.array(acc, np.float64).reshape(-1, L + 1)
    seen = av[:, M] > 0
    for m in range(M):
        t = int(mapping[m])
        if 0 <= t < L:
            out[seen, t] += av[seen, m]
    out[seen, L] += av[seen, M]
    return out


def sequence(views, P, M, L, iou_thresh=0.5, min_weight=0.0):
    """views: acc_view arrays in order.  -> (list of match dicts, the final float64 accumulator, count, dropped)"""
    acc = np.zeros((P, L + 1))
    count, dropped, outs = 0, 0, []
    for av in views:
        o = associate(av, acc, M, L, count, iou_thresh, min_weight)
        acc = merge(av, o["mapping"], acc, M, L)
        count, dropped = o["count"], dropped + o["dropped"]
        outs.append(o)
    return outs, acc, count, dropped
