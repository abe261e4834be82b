"""Development aid (GPU): time of the fused language-guided selection (edit.py, csrc/edit.hip) against the reference's own
calculate_selection_score (the bytecode under oracle/_ref/, about ten torch ops over the feature table) on the same GPU in
the same process, at (P, C, K) = (1M, 32, 5), (2M, 256, 5), (1M, 512, 5), (1M, 512, 64).

Protocol: 10 warm-up calls, then 50 calls each timed by its own pair of device events; the median is reported.  Algorithmic
bytes of the fused call: P*C*4 in, P*4 out, plus P*C*4 when the normalised rows are written back.  The (1M, 32) table
(128 MB) fits in the 256 MiB Infinity Cache, so its byte rate is not an HBM figure; the others are.  The reference's
function normalises in place, so it is timed on the already-normalised table (as every frame after the first sees it).
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import edit

dev = "cuda:0"
THR, POS = 0.198, [0]


def reference_function():
    try:
        import test_gpu_edit as T
        pyc = os.path.join(T.ru.REF_DIR, "ref_gaussian_renderer.pyc")
        return T._reference_module("ref_gr_bench").calculate_selection_score if os.path.exists(pyc) else None
    except BaseException as e:      # pytest.skip raises outside of a test run
        print("reference bytecode not available:", e)
        return None


def median_ms(fn, warm=10, n=50):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


ref = reference_function()
print(f"{'P':>8s} {'C':>4s} {'K':>3s}  {'fused':>9s} {'GB/s':>7s}  {'+write-back':>11s} {'GB/s':>7s}  {'reference':>10s} {'speed-up':>8s}")
for P, C, K in ((1 << 20, 32, 5), (2 << 20, 256, 5), (1 << 20, 512, 5), (1 << 20, 512, 64)):
    g = torch.Generator().manual_seed(0)
    f = torch.randn(P, C, generator=g).to(dev)
    t = (torch.randn(K, C, generator=g) + torch.randn(C, generator=g)).to(dev)
    pos = POS if K > 1 else [0]
    plain = median_ms(lambda: edit.selection_mask(f, t, THR, pos))
    back = median_ms(lambda: edit.selection_mask(f, t, THR, pos, normalize_inplace=True))
    nb, nbw = P * C * 4 + P * 4, 2 * P * C * 4 + P * 4
    if ref is not None:
        r = median_ms(lambda: ref(f, t, score_threshold=THR, positive_ids=pos))
        tail = f"{r:10.3f} {r / back:7.1f}x"
    else:
        tail = f"{'n/a':>10s}"
    print(f"{P:8d} {C:4d} {K:3d}  {plain:6.3f} ms {nb / plain / 1e6:7.0f}  {back:8.3f} ms {nbw / back / 1e6:7.0f}  {tail}", flush=True)
