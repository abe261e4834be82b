"""Timing of the fused open-vocabulary segmentation (segment.segment, csrc/segment.hip) against the two ways to get the same
labels without it, on the same GPU in the same process:

  (a) the torch chain: F.interpolate -> 1x1 conv -> .half() -> normalise -> matmul -> max (render.py:168-180 followed by
      encoders/lseg_encoder/segmentation.py:526-540);
  (b) fused_feature_decode(half=True) followed by torch's normalise, matmul and max.

10 warm-up calls, 50 calls timed by device events, median.  Also prints, per shape, the share of pixels whose label differs
from the float64 chain's and tau (tests/segment_oracle.py).  One JSON line per shape, then a table.

    python tools/segment_bench.py [--small]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from feature_loss import fused_feature_decode      # noqa: E402
from segment import segment                        # noqa: E402
import segment_oracle as O                         # noqa: E402

DEV = "cuda:0"


def median_ms(fn, warmup=10, calls=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def tail(x, text):
    f = x.float().permute(1, 2, 0).reshape(-1, x.shape[0])
    f = f / f.norm(dim=-1, keepdim=True)
    t = text / text.norm(dim=-1, keepdim=True)
    return torch.max(f @ t.t(), 1)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="a 270 x 480 source instead of 1080p")
    args = ap.parse_args()
    H, W = (270, 480) if args.small else (1080, 1920)
    Hs, Ws = 360, 480
    N = Hs * Ws
    rows = []
    for C, Cout, K in ((32, 128, 150), (128, 512, 150), (512, None, 150), (512, None, 20)):
        g = torch.Generator().manual_seed(C + K)
        fm = torch.randn(C, H, W, generator=g).to(DEV)
        w = b = None
        if Cout is not None:
            w = (torch.randn(Cout, C, generator=g) / C ** 0.5).to(DEV)
            b = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
        text = torch.randn(K, Cout or C, generator=g).to(DEV)

        def chain_a():
            x = F.interpolate(fm[None], size=(Hs, Ws), mode="bilinear", align_corners=True)
            if w is not None:
                x = F.conv2d(x, w[:, :, None, None], b)
            return tail(x[0].half(), text)

        def chain_b():
            return tail(fused_feature_decode(fm, (Hs, Ws), w, b, half=True), text)

        def fused():
            return segment(fm, text, size=(Hs, Ws), weight=w, bias=b)

        with torch.no_grad():
            t_f, t_a, t_b = median_ms(fused), median_ms(chain_a), median_ms(chain_b)
            l64 = O.chain(fm, text, (Hs, Ws), w, b, torch.float64)
            l32 = O.chain(fm, text, (Hs, Ws), w, b, torch.float32)
            tau = O.tau_of(l32, l64)
            lab, score = segment(fm, text, size=(Hs, Ws), weight=w, bias=b, return_score=True)
            fig = O.judge(lab, l64, tau, score)
            fig32 = O.judge(O.labels_of(l32), l64, tau)
        co = Cout or C
        flop = 2.0 * N * co * ((C if Cout else 0) + K)
        row = {"C": C, "Cout": Cout, "K": K, "source": [H, W], "fused_ms": t_f, "torch_ms": t_a, "decode_torch_ms": t_b,
               "tflops": flop / (t_f * 1e-3) / 1e12, "tau": tau, "share": fig["share"], "differing": fig["differing"],
               "max_shortfall": fig["max_shortfall"], "score_err": fig["score_err"], "torch_share": fig32["share"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del fm, l64, l32
        torch.cuda.empty_cache()
    print("\n   C  Cout    K      fused   TFLOP/s   (a) torch   (b) decode+torch   (b)/fused        tau      share   score err")
    for r in rows:
        print(f"{r['C']:4d} {str(r['Cout'] or '-'):>5} {r['K']:4d} {r['fused_ms']:8.3f} ms {r['tflops']:8.1f} {r['torch_ms']:8.3f} ms "
              f"{r['decode_torch_ms']:12.3f} ms {r['decode_torch_ms'] / r['fused_ms']:10.2f}x {r['tau']:10.2e} {r['share']:10.2e} "
              f"{r['score_err']:10.2e}")


if __name__ == "__main__":
    main()
