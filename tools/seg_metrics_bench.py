"""Development aid (GPU): time of the fused segmentation scores (seg_metrics.py: evaluate_segmentation, one host read for the whole
test set) against the two other routes to the same numbers, on a Replica-sized test set: 80 views of 360 x 480 with 150 labels.

  label_agreement   segment.label_agreement per view on the same device tensors: torch ops with a host read per class
  numpy on the host segmentation_metric.py's route restated (the label maps are numpy arrays there): per view the label counts,
                    and per class two boolean maps and two sums

A host clock around every route, ending in a device synchronise (each route ends in host reads of its own: they are part of what
is measured); the three routes alternate, median and minimum of `--reps` rounds after `--warmup` warm-up rounds, in one process.
The fused call is timed on int64 labels (what segment() returns) and on uint8 labels (what a label PNG holds), and its kernels
alone (segmentation_scores on the stacked views, device events, no host read).  Writes profiles/seg_metrics_bench.md (`--out`).

Algorithmic bytes of the fused call: every label map is read once - 8 or 1 bytes per pixel and side - and nothing of view size is
written."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

from seg_metrics import evaluate_segmentation, segmentation_scores
from segment import label_agreement

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=80)
ap.add_argument("--height", type=int, default=360)
ap.add_argument("--width", type=int, default=480)
ap.add_argument("--labels", type=int, default=150)
ap.add_argument("--classes", type=int, default=7)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_metrics_bench.md"))
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs a GPU"
dev = "cuda:0"
N, H, W, L, NC = args.views, args.height, args.width, args.labels, args.classes


def views(seed):
    """teacher: blocks of one label over a skewed distribution; student: the teacher with 30 % of the pixels redrawn"""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(L, 0.1))
    coarse = rng.choice(L, size=(N, (H + 23) // 24, (W + 23) // 24), p=p)
    t = np.repeat(np.repeat(coarse, 24, axis=1), 24, axis=2)[:, :H, :W]
    s = t.copy()
    w = rng.random(t.shape) < 0.3
    s[w] = rng.choice(L, size=int(w.sum()), p=p)
    return np.ascontiguousarray(t), s


def numpy_route(teachers, students):
    acc = iou = 0.0
    for t, s in zip(teachers, students):
        acc += float(np.sum(t == s)) / t.size
        labels, counts = np.unique(np.concatenate((t, s)), return_counts=True)
        values = []
        for i in labels[np.argsort(-counts, kind="stable")][:NC]:
            a, b = t == i, s == i
            values.append(np.sum(a & b) / np.sum(a | b))
        iou += float(np.nanmean(values))
    return acc / len(teachers), iou / len(teachers)


def agreement_route(teachers, students):
    acc = iou = 0.0
    for t, s in zip(teachers, students):
        a, i = label_agreement(t, s, NC)
        acc += a
        iou += i
    return acc / len(teachers), iou / len(teachers)


def fused_route(teachers, students):
    r = evaluate_segmentation(teachers, students, num_labels=L, num_classes=NC)
    return r["accuracy"], r["iou"]


t_np, s_np = views(1)
t64, s64 = torch.from_numpy(t_np).to(dev), torch.from_numpy(s_np).to(dev)
t8, s8 = t64.to(torch.uint8), s64.to(torch.uint8)
routes = [("numpy on the host, per view and class", lambda: numpy_route(list(t_np), list(s_np))),
          ("label_agreement per view (torch, device)", lambda: agreement_route(list(t64), list(s64))),
          ("evaluate_segmentation, int64 labels", lambda: fused_route(list(t64), list(s64))),
          ("evaluate_segmentation, uint8 labels", lambda: fused_route(list(t8), list(s8)))]
times = {name: [] for name, _ in routes}
results = {}
for rep in range(args.warmup + args.reps):
    for name, fn in routes:                      # alternating: every round runs every route once
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results[name] = fn()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            times[name].append((time.perf_counter() - t0) * 1e3)


def kernels_ms(t, s, reps=30, warm=5):
    for _ in range(warm):
        segmentation_scores(t, s, num_labels=L, num_classes=NC)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        segmentation_scores(t, s, num_labels=L, num_classes=NC)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out)


lines = [f"# Segmentation scores of a test set: {N} views of {H} x {W}, {L} labels, num_classes {NC}", "",
         f"`python tools/seg_metrics_bench.py` on {torch.cuda.get_device_name(0)}; host clock around each route (its host reads "
         f"included), routes alternating, {args.reps} rounds after {args.warmup} warm-up rounds.", "",
         "| route | median ms | min ms | per view us | against numpy | accuracy | iou |", "|---|---|---|---|---|---|---|"]
base = statistics.median(times[routes[0][0]])
for name, _ in routes:
    med = statistics.median(times[name])
    lines.append(f"| {name} | {med:.3f} | {min(times[name]):.3f} | {med / N * 1e3:.1f} | {base / med:.1f}x | {results[name][0]:.12f} | "
                 f"{results[name][1]:.12f} |")
lines += ["", "The kernels alone (segmentation_scores on the stacked views: clear, count, finish; device events, no host read, "
          "median / min of 30):", ""]
for name, (t, s), nbytes in (("int64", (t64, s64), 16), ("uint8", (t8, s8), 2)):
    med, best = kernels_ms(t, s)
    total = nbytes * N * H * W
    lines.append(f"- {name} labels: {med * 1e3:.1f} / {best * 1e3:.1f} us for {total / 1e6:.1f} MB of labels read once "
                 f"({total / med / 1e9:.2f} TB/s; the set fits the 256 MiB Infinity Cache: not an HBM figure)")
text = "\n".join(lines) + "\n"
print(text, flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
