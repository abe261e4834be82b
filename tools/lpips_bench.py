"""Development aid (GPU): time and peak memory of the fused LPIPS (lpips_vgg.py: lpips_views) against a plain torch fp32 chain
of the same network on the same device (tests/lpips_oracle.py, the tests' oracle, moved to the GPU: F.conv2d / F.max_pool2d /
the reference's tap arithmetic, x and y one after the other as the reference runs them), and against the fp32 matrix floor:
305,856 multiply-adds per input pixel (38,592 + 55,296 + 92,160 + 92,160 + 27,648 over the five blocks, the pools taken as
exact quarters) x 2 images x 2 at the 157 TFLOP/s peak of v_mfma_f32_32x32x2_f32 - 16.2 ms per 1080p pair.

Workloads: one 1080p pair, eight 1080p pairs, one 540 x 960 pair.  Weights and images from the tests' recipe
(tests/lpips_cases.py).  Each route is warmed up twice, then timed `--repeats` times with a host clock around work that ends in a
device synchronise; the median and the min..max spread are reported, with torch.cuda.max_memory_allocated of one call above the
inputs and weights.  Writes profiles/lpips_bench.md (`--out`).  Not imported by the product; bench.py does not know it.

    python tools/lpips_bench.py [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")]
import lpips_cases as cases  # noqa: E402
import lpips_oracle as oracle  # noqa: E402
import lpips_vgg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_bench.md"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = "cuda:0"
MAC_PER_PIXEL = 305856
PEAK_TFLOPS = 157.0

host_w = cases.make_weights(cases.SEED)
weights = lpips_vgg.LpipsWeights.from_state_dicts({k: torch.from_numpy(v) for k, v in host_w.items()}, device=dev)
dev_w = {k: torch.from_numpy(v).to(dev) for k, v in host_w.items()}


def images(n, H, W):
    case = cases.Case("bench", H, W, ("other",), False, 0)
    x, y = cases.make_pairs(case, cases.SEED)
    x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    shift = lambda t, k: torch.roll(t, (3 * k, 5 * k), (2, 3))
    return torch.cat([shift(x, k) for k in range(n)]), torch.cat([shift(y, k) for k in range(n)])


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


rows, agree = [], []
for label, n, H, W in (("one 1080p pair", 1, 1080, 1920), ("eight 1080p pairs", 8, 1080, 1920), ("one 540 x 960 pair", 1, 540, 960)):
    x, y = images(n, H, W)
    floor = 2 * n * H * W * MAC_PER_PIXEL * 2 / (PEAK_TFLOPS * 1e12) * 1e3
    fused = lambda: lpips_vgg.lpips_views(x, y, weights)
    chain = lambda: torch.cat([oracle.layer_terms(dev_w, x[k:k + 1], y[k:k + 1], torch.float32)[1] for k in range(n)])      # a pair at a time
    a, b = fused(), chain()
    agree.append((label, float(((a - b).abs() / b).max())))
    for name, fn in (("torch fp32 chain", chain), ("fused", fused)):
        rows.append((label, name) + measure(fn) + (floor,))
    del x, y
    torch.cuda.empty_cache()

lines = ["# LPIPS (VGG16): fused kernels against a torch fp32 chain and the fp32 matrix floor", "",
         f"`python tools/lpips_bench.py --repeats {args.repeats}` on {torch.cuda.get_device_name(0)}; host clock around each route, ending in a "
         "device synchronise; median (min .. max) of the repeats after two warm-up calls; peak = torch.cuda.max_memory_allocated above the "
         "inputs and weights, one call.  The torch chain is the tests' oracle in fp32 on the device (F.conv2d, F.max_pool2d, the reference's "
         "tap arithmetic), one pair at a time, x then y, as the reference's metrics.py runs it; its convolutions are the vendor library's.", "",
         f"Floor: {MAC_PER_PIXEL:,} multiply-adds per input pixel x 2 images x 2 at {PEAK_TFLOPS:.0f} TFLOP/s (the peak rate of "
         "v_mfma_f32_32x32x2_f32); it bounds the matrix work only, not the loads, the taps or the launches.", "",
         "Agreement of the two routes (max relative difference of the totals): " + "; ".join(f"{w}: {v:.3g}" for w, v in agree) + ".", "",
         "| workload | route | ms median | ms min .. max | peak MiB | matrix floor ms | floor / median |", "|---|---|---|---|---|---|---|"]
for w, n, med, lo, hi, peak, floor in rows:
    lines.append(f"| {w} | {n} | {med:.2f} | {lo:.2f} .. {hi:.2f} | {peak:.0f} | {floor:.2f} | {floor / med:.3f} |")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
