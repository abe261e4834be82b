"""Restatement of the reference's segmentation chain (render.py:168-180 followed by
encoders/lseg_encoder/segmentation.py:501-540) in plain torch at a chosen dtype, the seeded input makers and the label rule
of the segmentation tests (tests/test_segment_cpu.py, tests/test_gpu_segment.py).

The JUDGE is this chain in float64 with the fp16 store applied; it is never the kernel's own output.  A pixel may differ from
the float64 label only if the float64 logit of the label it got lies within tau of the float64 maximum, and at most MAX_SHARE of a
case's pixels may differ at all.  tau is 4 x the largest |logit_fp32 - logit_fp64| of this same chain run in float32 (the
reference's own precision, dominated by fp16 neighbours flipping): the factor 4 because a kernel's summation order differs from
both chains and a maximum over 10^4 .. 10^5 pixels is a noisy statistic.
"""
import math

import torch
import torch.nn.functional as F

MAX_SHARE = 1e-3
TAU_FACTOR = 4.0

# name, C, Cout (None: no decoder), K, source (H, W), size (None: the map's own)
CASES = [
    ("dec32_k20", 32, 128, 20, (135, 180), (90, 120)),             # shrinking; 10 800 pixels: not a multiple of the 128-pixel tile
    ("dec32_k150", 32, 128, 150, (135, 180), (90, 120)),
    ("dec128_k150", 128, 512, 150, (100, 140), (90, 120)),
    ("nodec512_k150", 512, None, 150, (60, 80), (67, 91)),         # growing
    ("nodec48_k20", 48, None, 20, (80, 100), (37, 53)),            # a zero-padded last block of channels
    ("dec64_k1", 64, 256, 1, (50, 60), (41, 47)),
    ("dec32_k256", 32, 128, 256, (50, 60), (75, 90)),              # growing
    ("nodec512_none", 512, None, 150, (45, 60), None),             # size=None
    ("nodec3_k5", 3, None, 5, (33, 47), (40, 50)),                 # rows that cannot be read 16 bytes at a time
]
FAMILIES = ("random", "regions")


def case(name):
    return next(c for c in CASES if c[0] == name)


def make_inputs(name, family, seed=0):
    """{fm (C,H,W), weight (Cout,C) or None, bias or None, text (K,Cout), size} on the CPU, float32, seeded.
    random: everything N(0,1), decoder rows scaled by 1/sqrt(C), bias 0.1 N(0,1).
    regions: a chequered label field whose features are the pseudo-inverse images of the text embeddings (through the decoder,
    where there is one) plus 0.3 N(0,1) noise: large areas share a label and the boundaries are real."""
    _, C, Cout, K, (H, W), size = case(name)
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, name + family)))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    weight = bias = None
    if Cout is not None:
        weight = rn(Cout, C) / math.sqrt(C)
        bias = 0.1 * rn(Cout)
    text = rn(K, Cout if Cout is not None else C)
    if family == "random":
        fm = rn(C, H, W)
    else:
        by, bx = max(2, H // 5), max(2, W // 6)
        yy, xx = torch.meshgrid(torch.arange(H) // by, torch.arange(W) // bx, indexing="ij")
        field = (yy * 7 + xx * 3) % K                                      # (H, W) labels
        proto = text if weight is None else (text - bias) @ torch.linalg.pinv(weight).T      # (K, C): W proto + b ~ text
        fm = proto[field].permute(2, 0, 1) + 0.3 * rn(C, H, W)
    f32 = lambda t: None if t is None else t.to(torch.float32).contiguous()
    return {"fm": f32(fm), "weight": f32(weight), "bias": f32(bias), "text": f32(text), "size": size}


def add_special_pixels(fm):
    """A zero pixel, an inf, a NaN and a value that overflows fp16, apart from each other (for a map used with size=None)."""
    fm = fm.clone()
    fm[:, 3, 4] = 0.0
    fm[1, 10, 11] = float("inf")
    fm[2, 20, 5] = float("nan")
    fm[0, 30, 30] = 1.0e5
    return fm


def chain(fm, text, size, weight=None, bias=None, dtype=torch.float64, half=True, second_size=None):
    """The (Hs*Ws, K) logits of the reference chain at `dtype`, on fm's device.  half: the fp16 store of render.py:179-180.
    second_size: segmentation.py:501-521's resize of the stored map."""
    x = fm.to(dtype)
    if size is not None:
        x = F.interpolate(x[None], size=tuple(size), mode="bilinear", align_corners=True)[0]
    if weight is not None:
        x = F.conv2d(x[None], weight.to(dtype)[:, :, None, None], None if bias is None else bias.to(dtype))[0]
    if half:
        x = x.to(torch.float16)
    x = x.to(torch.float32 if dtype == torch.float32 else dtype)
    if second_size is not None:
        x = F.interpolate(x[None], size=tuple(second_size), mode="bilinear", align_corners=True)[0]
    f = x.permute(1, 2, 0).reshape(-1, x.shape[0])
    f = f / f.norm(dim=-1, keepdim=True)
    t = text.to(dtype)
    t = t / t.norm(dim=-1, keepdim=True)
    return f @ t.t()


def labels_of(logits):
    return torch.max(logits, 1)[1]


def tau_of(logits32, logits64):
    """4 x the reference chain's own float32 error, over the pixels whose float64 logits are all finite."""
    fin = torch.isfinite(logits64).all(dim=1)
    d = (logits32[fin].to(torch.float64) - logits64[fin]).abs()
    return TAU_FACTOR * float(d.max()) if d.numel() else 0.0


def judge(labels, logits64, tau, score=None):
    """Checks `labels` (N,) (and `score` (N,)) against the float64 logits.  Returns a dict of figures; raises AssertionError."""
    labels = labels.reshape(-1).to(logits64.device)
    fin = torch.isfinite(logits64).all(dim=1)
    lg = logits64[fin]
    top, lab64 = torch.max(lg, 1)
    got = labels[fin]
    assert int(got.min()) >= 0 and int(got.max()) < logits64.shape[1], "label out of range"
    diff = got != lab64
    shortfall = top - lg.gather(1, got[:, None])[:, 0]
    n = max(1, int(fin.sum()))
    out = {"pixels": int(fin.sum()), "differing": int(diff.sum()), "share": float(diff.sum()) / n,
           "max_shortfall": float(shortfall.max()) if shortfall.numel() else 0.0, "tau": tau}
    if score is not None:
        s = score.reshape(-1).to(logits64.device)[fin].to(torch.float64)
        out["score_err"] = float((s - top).abs().max()) if s.numel() else 0.0
    print("segment judge:", out)
    assert out["max_shortfall"] <= tau, f"a pixel's label is {out['max_shortfall']:.3e} below the float64 maximum, tau = {tau:.3e}"
    assert out["share"] <= MAX_SHARE, f"{out['differing']} of {out['pixels']} pixels differ from the float64 labels"
    if score is not None:
        assert torch.isfinite(s).all(), "a non-finite score on a finite pixel"
        assert out["score_err"] <= tau, f"score off the float64 maximum by {out['score_err']:.3e}, tau = {tau:.3e}"
    return out
