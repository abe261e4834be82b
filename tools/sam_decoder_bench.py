"""Development aid (GPU): time and peak memory of the fused SAM prompt encoder + mask decoder (sam_decoder.py: plan, predict)
against a plain torch fp32 implementation of the same chain on the same device (tests/sam_decoder_oracle.py, the tests' oracle,
moved to the GPU: about 150 torch launches per batch, the image tokens repeated per prompt, the upscaled embedding
materialised), and against the fp32 matrix floor: the FLOPs of the fused design counted from the shapes below, at the measured
155 TFLOP/s of v_mfma_f32_32x32x2_f32.

Workload: a 64 x 64 embedding grid (input 1024 x 1024), one point per prompt (7 tokens), three masks; one batch of 64 prompts,
and 1024 prompts = a 32 x 32 point grid as 16 batches.  Weights and features from the tests' recipe (tests/sam_decoder_cases.py).
Each route is warmed up twice, then timed `--repeats` times with a host clock around work that ends in a device synchronise; the
median and the min..max spread are reported, with torch.cuda.max_memory_allocated of one call above the inputs.  Writes
profiles/sam_decoder_bench.md (`--out`).  Not imported by the product; bench.py does not know it.

    python tools/sam_decoder_bench.py [--repeats 10]
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
import sam_decoder  # noqa: E402
import sam_decoder_cases as cases  # noqa: E402
import sam_decoder_oracle as oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_decoder_bench.md"))
args = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU"
dev = "cuda:0"
H = W = 64
B, NB, T, NM = 64, 16, 7, 3
MFMA_TFLOPS = 155.0


def flops(b, hw=H * W, t=T, nm=NM):
    """the fused design's multiply-adds x 2, from the layer shapes: (per predict call of b prompts, per plan)"""
    D, DI, MLP = 256, 128, 2048
    rows = b * t
    tok = 2 * (4 * 2 * D * D + 2 * 2 * D * DI + 2 * 2 * D * MLP + 2 * 2 * D * DI) + 2 * 2 * D * DI          # the token-side linears
    tok = rows * tok + b * (nm * 2 * (2 * D * D + D * 32) + 2 * (2 * D * D + D * 32))                       # + the heads
    attn = 2 * 2 * t * DI * hw                                     # scores and attn V of one attention over the image tokens
    t2i = 3 * attn + 2 * (2 * 2 * hw * D * DI)                     # layer 1 and the final attention project K and V per prompt
    i2t = 2 * (attn + 2 * hw * DI * D) + 2 * hw * D * DI           # out_proj twice, the q projection in layer 1
    up = 2 * hw * D * D + 4 * 2 * hw * 64 * 128 + 2 * hw * 16 * 32 * nm
    return tok + b * (t2i + i2t + up), 3 * 2 * hw * D * DI


case = cases.Case("bench", (H, W), B, labels=[1], input_size=(1024, 1024))
host_w = cases.make_weights()
weights = sam_decoder.SamDecoderWeights.from_state_dict({k: torch.from_numpy(v) for k, v in host_w.items()}, device=dev)
dev_w = oracle.as_torch(host_w, dev)
features = torch.from_numpy(cases.make_features(case)).to(dev)
pe = oracle.dense_pe(oracle.as_torch(host_w), H, W).to(dev)
rng = np.random.default_rng(11)
coords = [torch.from_numpy((rng.uniform(0, 1024, (B, 1, 2))).astype(np.float32)).to(dev) for _ in range(NB)]
labels = torch.ones((B, 1), dtype=torch.int32, device=dev)


def fused(n):
    p = sam_decoder.plan(weights, features)
    return [sam_decoder.predict(p, coords[i], labels) for i in range(n)]


def torch_chain(n):
    out = []
    for i in range(n):
        sparse = oracle.sparse_tokens(dev_w_cpu, coords[i].cpu(), labels.cpu(), None, (1024, 1024)).to(dev)
        low, iou, _ = oracle.decode(dev_w, features, sparse, True, torch.float32, pe=pe, device=dev, want_info=False)
        out.append((low, iou))
    return out


dev_w_cpu = oracle.as_torch(host_w)


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


a, b = fused(1)[0], torch_chain(1)[0]
agree = float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()), float(((a[0] > 0) == (b[0] > 0)).float().mean())
plan_ms = measure(lambda: sam_decoder.plan(weights, features))
rows = []
for label, n in ((f"one batch of {B} prompts", 1), (f"{B * NB} prompts = {NB} batches", NB)):
    f_call, f_plan = flops(B)
    floor = (n * f_call + f_plan) / (MFMA_TFLOPS * 1e12) * 1e3
    for name, fn in (("torch fp32 chain", torch_chain), ("fused", fused)):
        rows.append((label, name) + measure(lambda: fn(n)) + (floor, (n * f_call + f_plan) / 1e9))
lines = ["# SAM prompt encoder + mask decoder: fused kernels against a torch fp32 chain and the fp32 matrix floor", "",
         f"`python tools/sam_decoder_bench.py --repeats {args.repeats}` on {torch.cuda.get_device_name(0)}; host clock around each route, ending in a "
         "device synchronise; median (min .. max) of the repeats after two warm-up calls; peak = torch.cuda.max_memory_allocated above the "
         "inputs, one call.  The fused route includes its image plan (once per leg); the torch chain encodes its prompts on the host, as the tests' oracle does.", "",
         f"{H} x {W} grid, {T} tokens per prompt, {NM} masks.  Floor: the fused design's FLOPs counted from the shapes at {MFMA_TFLOPS:.0f} TFLOP/s "
         "(v_mfma_f32_32x32x2_f32, measured rate); it bounds the matrix work only, not the loads, the softmaxes or the launches.", "",
         f"Agreement of the two routes on batch 0: max |logit difference| {agree[0]:.3g}, max |iou difference| {agree[1]:.3g}, {agree[2]:.6f} of the binary mask pixels equal.", "",
         f"Image plan alone: {plan_ms[0]:.3f} ms ({plan_ms[1]:.3f} .. {plan_ms[2]:.3f}).", "",
         "| workload | route | ms median | ms min .. max | peak MiB | GFLOP counted | matrix floor ms | floor / median |", "|---|---|---|---|---|---|---|---|"]
for w, n, med, lo, hi, peak, floor, gf in rows:
    tail = f"{gf:.0f} | {floor:.2f} | {floor / med:.3f}" if n == "fused" else "- | - | -"
    lines.append(f"| {w} | {n} | {med:.2f} | {lo:.2f} .. {hi:.2f} | {peak:.0f} | {tail} |")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
open(args.out, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
