"""Development aid (GPU): time and peak memory of the fused SAM mask pass (sam_masks.py: mask_pass, masks_to_rle) against the
reference's torch chain on the same device, restated here: two F.interpolate calls around the crop (Sam.postprocess_masks),
calculate_stability_score, the threshold, batched_mask_to_box and mask_to_rle_pytorch with its per-mask host loop.

Workload: one batch of 64 points x 3 masks, 256 x 256 logits, img_size 1024, input (576, 1024), a 1080 x 1920 frame; and a whole
32 x 32 point grid as 16 such batches.  Smooth random logits (blobs), so that the run lengths are those of masks, not of noise.
Each route is warmed up, then timed `--repeats` times with a host clock around work that ends in a device synchronise; the
median and the min..max spread are reported, with torch.cuda.max_memory_allocated of one call.  Writes profiles/sam_masks_bench.md
(`--out`).  Not imported by the product; bench.py does not know it.

    python tools/sam_masks_bench.py [--repeats 10] [--rle-masks 24]
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "feature-3dgs_amd"))
from sam_masks import mask_pass, masks_to_rle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--rle-masks", type=int, default=24, help="masks whose run lengths are made (both routes)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_masks_bench.md"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = "cuda:0"
M, h, S, INP, ORIG = 192, 256, 1024, (576, 1024), (1080, 1920)
T, OFF = 0.0, 1.0


def logits(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    coarse = 4 * torch.randn(M, 1, 9, 9, device=dev, generator=g)
    return F.interpolate(coarse, (h, h), mode="bicubic", align_corners=True)[:, 0].contiguous()


def chain(lr, n_rle):
    v = F.interpolate(lr[:, None], (S, S), mode="bilinear", align_corners=False)[..., :INP[0], :INP[1]]
    v = F.interpolate(v, ORIG, mode="bilinear", align_corners=False)[:, 0]
    inter = (v > T + OFF).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    union = (v > T - OFF).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    stability = inter / union
    masks = v > T
    Hh, Ww = masks.shape[-2:]
    in_h = masks.amax(-1)
    ch = in_h * torch.arange(Hh, device=dev)[None]
    bottom, top = ch.amax(-1), (ch + Hh * (~in_h)).amin(-1)
    in_w = masks.amax(-2)
    cw = in_w * torch.arange(Ww, device=dev)[None]
    right, left = cw.amax(-1), (cw + Ww * (~in_w)).amin(-1)
    boxes = torch.stack([left, top, right, bottom], -1) * (~((right < left) | (bottom < top)))[:, None]
    flat = masks[:n_rle].permute(0, 2, 1).flatten(1)
    change = (flat[:, 1:] ^ flat[:, :-1]).nonzero()
    out = []
    for i in range(flat.shape[0]):
        cur = change[change[:, 0] == i, 1]
        cur = torch.cat([cur.new_zeros(1), cur + 1, cur.new_full((1,), Hh * Ww)])
        out.append(([] if flat[i, 0] == 0 else [0]) + (cur[1:] - cur[:-1]).cpu().tolist())
    return stability, boxes, out


def fused(lr, n_rle):
    st = mask_pass(lr, S, INP, ORIG, mask_threshold=T, stability_offset=OFF)
    return st.stability, st.box, [r["counts"] for r in masks_to_rle(st.packed, torch.arange(n_rle, device=dev))]


def measure(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times), peak / 2 ** 20


batches = [logits(s) for s in range(16)]
a, b = chain(batches[0], args.rle_masks), fused(batches[0], args.rle_masks)
agree = dict(boxes=float((a[1] == b[1]).float().mean()), rle=sum(x == y for x, y in zip(a[2], b[2])) / max(len(a[2]), 1))
rows = []
for label, n_rle in (("pass only (no run lengths)", 0), (f"pass + run lengths of {args.rle_masks} masks", args.rle_masks)):
    for name, fn in (("torch chain", chain), ("fused", fused)):
        rows.append((f"one batch, {label}", name) + measure(lambda: fn(batches[0], n_rle)))
        rows.append((f"32 x 32 grid = 16 batches, {label}", name) + measure(lambda: [fn(x, n_rle) for x in batches]))
lines = ["# SAM mask post-processing: fused pass against the torch chain", "",
         f"`python tools/sam_masks_bench.py --repeats {args.repeats} --rle-masks {args.rle_masks}` on {torch.cuda.get_device_name(0)}; host clock "
         "around each route, ending in a device synchronise; median (min .. max) of the repeats after two warm-up calls; peak = "
         "torch.cuda.max_memory_allocated above the inputs, one call.", "",
         f"{M} masks of {h} x {h} logits, img_size {S}, input {INP}, frame {ORIG}.  Agreement of the two routes on batch 0: boxes "
         f"{agree['boxes']:.4f} of the entries equal, run-length lists {agree['rle']:.4f} equal (they may differ on pixels within rounding of a threshold).", "",
         "| workload | route | ms median | ms min .. max | peak MiB |", "|---|---|---|---|---|"]
for w, n, med, lo, hi, peak in rows:
    lines.append(f"| {w} | {n} | {med:.2f} | {lo:.2f} .. {hi:.2f} | {peak:.0f} |")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
