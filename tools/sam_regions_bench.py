"""Development aid (GPU): time and peak memory of the small-region removal on the device (sam_masks.py:postprocess_small_regions,
csrc/mask_regions.hip) against the route the reference takes (automatic_mask_generator.py:postprocess_small_regions): the masks
unpacked to dense bool, copied to the host, labelled there twice per mask (utils/amg.py:remove_small_regions, restated over
scipy.ndimage.label in OpenCV's place) and the boxes taken from the dense stack.  Where scipy does not import, the device-to-host
copy of the dense masks alone is reported: a floor that the host route cannot beat.

Workload: K = 24 and K = 96 masks of a 1080 x 1920 frame, blobs (a smooth random field above a threshold) with a sprinkle of
specks and pinholes, min_area 100; and one pathological mask, a 1080 x 1920 checkerboard (about a million runs in one component),
so that the worst case is a known number.  Each route is warmed up, then timed `--repeats` times with a host clock around work that
ends in a device synchronise; the median and the min..max spread are reported, with torch.cuda.max_memory_allocated of one call
above the inputs.  Writes profiles/sam_regions_bench.md (`--out`).  Not imported by the product; bench.py does not know it.

    python tools/sam_regions_bench.py [--repeats 10]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "feature-3dgs_amd"))
import sam_masks as sm  # noqa: E402

try:
    import scipy.ndimage as ndi
except ImportError:
    ndi = None

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--min-area", type=float, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_regions_bench.md"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = "cuda:0"
FH, FW = 1080, 1920


def blobs(K, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    coarse = torch.randn(K, 1, 7, 11, device=dev, generator=g)
    field = F.interpolate(coarse, (FH, FW), mode="bicubic", align_corners=True)[:, 0]
    masks = field > 0.8
    masks ^= torch.rand(K, FH, FW, device=dev, generator=g) < 2e-4          # specks outside, pinholes inside
    return sm.pack_masks(masks)


def device_route(packed):
    return sm.postprocess_small_regions(packed, args.min_area)


def host_label(mask, thresh, holes):
    """utils/amg.py:remove_small_regions with scipy.ndimage.label for cv2.connectedComponentsWithStats"""
    working = ~mask if holes else mask
    labels, n = ndi.label(working, structure=np.ones((3, 3), int))
    sizes = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
    small = [i + 1 for i, s in enumerate(sizes) if s < thresh]
    if not small:
        return mask, False
    fill = [0] + small
    if not holes:
        fill = [i for i in range(n + 1) if i not in fill] or [int(np.argmax(sizes)) + 1]
    return np.isin(labels, fill), True


def host_route(packed):
    dense = sm.unpack_masks(packed).cpu()                                    # the copy the reference's route begins with
    if ndi is None:
        return dense
    new, changed = [], []
    for m in dense.numpy():
        m, a = host_label(m, args.min_area, True)
        m, b = host_label(m, args.min_area, False)
        new.append(torch.as_tensor(m))
        changed.append(a or b)
    masks = torch.stack(new)
    rows, cols = masks.any(2), masks.any(1)                                   # batched_mask_to_box on the dense stack
    ys, xs = torch.arange(FH), torch.arange(FW)
    box = torch.stack([(cols * xs + FW * ~cols).amin(1), (rows * ys + FH * ~rows).amin(1), (cols * xs).amax(1), (rows * ys).amax(1)], 1)
    return masks, changed, box * masks.flatten(1).any(1)[:, None]


def measure(fn, repeats):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times), peak / 2 ** 20


def runs_of(packed, holes):
    return sm._C().mask_regions(packed.words, None, FH, float(args.min_area), holes, 0)[4]       # (no room: only the count comes back)


host_name = "host route (unpack, copy, scipy.ndimage.label twice, boxes)" if ndi is not None else "device-to-host copy of the dense masks alone (no scipy here: a floor for the host route)"
rows, notes = [], []
for K in (24, 96):
    packed = blobs(K, K)
    sr = device_route(packed)
    if ndi is not None:
        masks, changed, box = host_route(packed)
        same = bool((sm.unpack_masks(sr.packed).cpu() == masks).all()) and sr.changed.cpu().tolist() == changed and bool((sr.box.cpu() == box).all())
        notes.append(f"K = {K}: the two routes agree on every bit, flag and box: {same}; {int(sr.changed.sum())} of {K} masks changed.")
    notes.append(f"K = {K}: runs per mask {runs_of(packed, True) / K:.0f} (background) and {runs_of(packed, False) / K:.0f} (foreground); "
                 f"the packed input is {packed.words.numel() * 4 / 2 ** 20:.1f} MiB.")
    rows.append((f"K = {K} blobs", "device (postprocess_small_regions)") + measure(lambda: device_route(packed), args.repeats))
    rows.append((f"K = {K} blobs", host_name) + measure(lambda: host_route(packed), max(1, min(args.repeats, 3 if ndi is not None else args.repeats))))
board = sm.pack_masks(((torch.arange(FH, device=dev)[:, None] + torch.arange(FW, device=dev)[None]) % 2 == 1)[None])
notes.append(f"checkerboard: {runs_of(board, False)} foreground runs in one component (the provision of 4 FW + 64 runs per mask is outgrown: "
             "every labelling runs twice).")
rows.append(("1 checkerboard", "device (postprocess_small_regions)") + measure(lambda: device_route(board), args.repeats))

lines = ["# Small-region removal: bit-packed labelling on the device against the reference's host route", "",
         f"`python tools/sam_regions_bench.py --repeats {args.repeats}` on {torch.cuda.get_device_name(0)}; host clock around each route, ending in "
         "a device synchronise; median (min .. max) of the repeats (the host route: up to 3) after a warm-up call; peak = "
         "torch.cuda.max_memory_allocated above the inputs, one call (device memory only: the host route's dense arrays live in host memory).", "",
         f"Masks of a {FH} x {FW} frame, min_area {args.min_area:g}; holes, then islands, with the area and box of the result.", ""]
lines += [f"- {n}" for n in notes]
lines += ["", "| workload | route | ms median | ms min .. max | peak MiB |", "|---|---|---|---|---|"]
for w, n, med, lo, hi, peak in rows:
    lines.append(f"| {w} | {n} | {med:.2f} | {lo:.2f} .. {hi:.2f} | {peak:.0f} |")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
