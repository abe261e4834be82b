"""The blend kernels at every channel-window edge, against the CPU oracle.

The feature width C is a run-time argument; the blend kernels cut it into channel windows and pick a kernel shape per window
from its width nc (csrc/render_fwd.hip: launch_render_forward, csrc/render_bwd_pl.hip: launch_render_backward_pl,
csrc/render_bwd.hip: launch_render_backward).  `window_plan` restates those three dispatchers; the CPU test below checks that
the ragged widths of CHANNELS reach, under the option families of FAMILIES, every (shape, first / later window) pair the
dispatchers can produce, and the GPU sweep holds each (family, C) to the oracle's bars - per channel as well as per tensor.

Channel c of the features is scaled by s_c = 2^((5c mod 9) - 4) and channel c of the upstream feature gradient by 1 / s_c: the
geometric gradients get a balanced share from every channel (a window dropped from them shows) and a value routed to the wrong
channel is off by at least a factor of 2.
"""
import numpy as np
import pytest

from util import _strict_compare

CHANNELS = [1, 2, 7, 17, 31, 33, 37, 63, 65, 67, 81, 97, 99, 131, 137, 150, 161, 193, 257]

# option families: the product options each sets, and the contraction f3dgs_last_backward_contraction must report (None: not
# asserted; 0 exact fp32 / instance-lane, 1 bf16 two-term, 2 hybrid first window)
FAMILIES = {
    "D": ({}, 1),                                          # defaults
    "E": ({"bwd_bf16": 0}, 0),                             # exact shapes: m44 first window, split16, split32, exact later windows
    "N": ({"fwd_wide": 0, "bwd_wide8": 0}, None),          # 64-channel forward windows, bf16 later windows of at most 64
    "V": ({"feature_mfma": 0}, None),                      # VALU forward shapes, instance-lane backward without the matrix pipe
    "I": ({"bwd_pl": 0}, 0),                               # instance-lane backward on the matrix pipe
    "H": ({"bwd_bf16_max_ratio": 1}, 2),                   # every frame "too long": the hybrid first window
}
H_CHANNELS = [1, 7, 17, 31, 33]

DEFAULTS = dict(feature_mfma=1, fwd_wide=1, bwd_pl=-1, bwd_m44=1, bwd_split16=1, bwd_bf16=-1, bwd_bf16_max_ratio=16, bwd_wide8=1)


def channel_scale(C: int) -> np.ndarray:
    return np.array([2.0 ** ((5 * c) % 9 - 4) for c in range(C)])


# ------------------------------------------------------------------------------------------------ the dispatchers, restated --
def _fwd_shape(nc: int, mf: bool) -> str:
    if nc <= 4:
        return "fwd<4,1>"
    if nc <= 16:
        return "fwd_mf<16>" if mf else "fwd<16,1>"
    if nc <= 32:
        return "fwd_mf<32>" if mf else "fwd<32,2>"
    if nc <= 64:
        return "fwd_mf<64>" if mf else "fwd<64,1>"
    return "fwd_mf<128>"


def window_plan(C: int, options: dict, long_frame: bool = False) -> list:
    """Every blend window one forward + backward call launches at feature width C > 0: dicts of pass ("fwd" / "bwd"), shape,
    first (the window that carries the colour / depth / geometric work), c0, nc and vec_ok (the forward's float4 feature rows).
    `long_frame`: the frame holds a Gaussian longer than bwd_bf16_max_ratio times its width (option bwd_bf16 = -1 then takes the
    hybrid first window)."""
    o = dict(DEFAULTS, **options)
    mf = o["feature_mfma"] != 0
    plan = []
    # forward (render_fwd.hip, launch_render_forward): 64-channel windows, 128 on the matrix pipe while more than 64 remain
    wide = 128 if (mf and o["fwd_wide"] != 0 and C > 64) else 64
    c0 = 0
    while c0 < C:
        win = wide if C - c0 > 64 else 64
        nc = min(win, C - c0)
        plan.append(dict(pass_="fwd", shape=_fwd_shape(nc, mf), first=c0 == 0, c0=c0, nc=nc, vec_ok=C % 4 == 0 and c0 % 4 == 0))
        c0 += win
    # backward contraction (api.hip): 1 bf16, 0 exact, 2 hybrid
    contraction = 1 if o["bwd_bf16"] > 0 else 0
    if o["bwd_bf16"] < 0:
        contraction = 2 if long_frame else 1
    pl = (o["bwd_pl"] > 0 or (o["bwd_pl"] < 0 and C > (0 if contraction else 4))) and mf
    vec = C % 4 == 0
    if pl:
        # pixel-lane (render_bwd_pl.hip, launch_render_backward_pl / launch_pl): the first window carries 32 channels
        nc = min(32, C)
        if contraction == 2:
            shape = "pl_hyb"
        elif contraction:
            shape = "pl_bf16"
        elif o["bwd_m44"]:
            shape = "pl_m44"
        else:
            shape = "pl_exact"
        split = contraction == 0 and o["bwd_split16"] != 0 and nc <= 16
        plan.append(dict(pass_="bwd", shape=shape + ("+split16" if split else ""), first=True, c0=0, nc=nc, vec_ok=vec))
        bf16 = 1 if (o["bwd_bf16"] < 0 or contraction >= 2) else contraction
        wide8 = bf16 and o["bwd_wide8"] != 0
        c0 = 32
        while c0 < C:
            left = C - c0
            if wide8 and left > 64:
                nc, shape = min(128, left), "pl_kernel8"
            else:
                nc = min(64, left)
                if bf16:
                    shape = "pl_bf16"
                else:
                    shape = "pl_exact" + ("+split32" if o["bwd_split16"] != 0 and nc <= 32 else "")
            plan.append(dict(pass_="bwd", shape=shape, first=False, c0=c0, nc=nc, vec_ok=vec))
            c0 += nc
    else:
        # instance-lane (render_bwd.hip, launch_render_backward): windows of 64
        for c0 in range(0, C, 64):
            nc = min(64, C - c0)
            if nc <= 4:
                shape = "il<4>"
            elif nc <= 16:
                shape = "il<16>"
            else:
                shape = ("il<32" if nc <= 32 else "il<64") + (",mf>" if mf else ">")
            plan.append(dict(pass_="bwd", shape=shape, first=c0 == 0, c0=c0, nc=nc, vec_ok=vec))
    return plan


def kernel_name(w: dict) -> str:
    """The kernel symbol (as a kernel trace names it, template arguments included) that runs window w."""
    s, first = w["shape"].split("+")[0], w["first"]
    b = "true" if first else "false"
    if s.startswith("fwd_mf<"):
        ch = int(s[7:-1])
        occ = "w4" if ch <= 32 else "w3" if ch <= 64 else "w2"
        return f"render_forward_mfma_kernel_{occ}<{ch}, {b}>"
    if s.startswith("fwd<"):
        return f"render_forward_kernel<{s[4:-1].replace(',', ', ')}>"
    if s == "pl_hyb":
        return "render_backward_pl_kernel_hyb"
    if s == "pl_kernel8":
        return "render_backward_pl_kernel8"
    if s.startswith("pl_"):
        tail = {"pl_bf16": "false, true", "pl_m44": "true, false", "pl_exact": "false, false"}[s]
        return f"render_backward_pl_kernel<{b}, 1, true, {tail}>"
    ch = int(s[3:].split(",")[0].rstrip(">"))
    mfa = "true" if s.endswith(",mf>") else "false"
    geo = "true" if first else "false"
    return f"render_backward_kernel{'_w3' if ch <= 32 else ''}<{ch}, 64, {mfa}, 4, {geo}, true>"


def _family_plans(channels, families=FAMILIES):
    for fam, (opts, _c) in families.items():
        for C in channels:
            if fam == "H" and C not in H_CHANNELS:
                continue
            yield fam, C, window_plan(C, opts, long_frame=fam == "H")


def _pairs(channels, families=FAMILIES):
    return {(w["shape"], w["first"]) for _f, _C, plan in _family_plans(channels, families) for w in plan}


def test_the_sweep_reaches_every_window_shape():
    """CPU: under the families, CHANNELS reaches every (shape, first / later) pair that any width from 1 to 512 reaches, the
    shapes the dispatchers name in later windows at ragged widths, and an unaligned (scalar) feature-row read there."""
    got = _pairs(CHANNELS)
    every = _pairs(range(1, 513), {f: FAMILIES[f] for f in FAMILIES if f != "H"}) | _pairs(H_CHANNELS, {"H": FAMILIES["H"]})
    assert every - got == set(), sorted(every - got)
    required = [
        ("fwd<4,1>", False), ("fwd_mf<16>", False), ("fwd_mf<32>", False), ("fwd_mf<64>", False), ("fwd_mf<128>", False),
        ("fwd<16,1>", False), ("fwd<32,2>", False), ("fwd<64,1>", False), ("fwd_mf<128>", True),
        ("pl_bf16", True), ("pl_m44", True), ("pl_m44+split16", True), ("pl_hyb", True),
        ("pl_bf16", False), ("pl_exact", False), ("pl_exact+split32", False), ("pl_kernel8", False),
        ("il<4>", False), ("il<16>", False), ("il<32,mf>", False), ("il<64,mf>", False), ("il<32>", False), ("il<64>", False),
    ]
    missing = [p for p in required if p not in got]
    assert not missing, missing
    later = [w for _f, _C, plan in _family_plans(CHANNELS) for w in plan if not w["first"]]
    # in a later window: a width that is not a multiple of 16 for every kind of kernel, and the scalar feature-row path
    for kind in ("fwd", "pl_kernel8", "pl_", "il<"):
        ragged = [w for w in later if w["shape"].startswith(kind) and w["nc"] % 16]
        assert ragged, f"no later {kind} window of a ragged width"
    assert any(w["pass_"] == "fwd" and not w["vec_ok"] for w in later)
    kernel8 = sorted({w["nc"] for w in later if w["shape"] == "pl_kernel8"})
    assert kernel8[0] < 96, kernel8            # a kernel8 window narrower than any the reference-width cases run
    assert 1 in {w["nc"] for w in later if w["shape"].startswith("pl_")}


def test_window_plan_restates_the_issue_examples():
    """CPU: the dispatch the plan restates, at the widths the sweep was chosen by (defaults unless stated)."""
    def shapes(C, opts=None, pass_=None):
        return [(w["shape"], w["nc"]) for w in window_plan(C, opts or {}) if pass_ is None or w["pass_"] == pass_]
    assert shapes(33, pass_="fwd") == [("fwd_mf<64>", 33)]
    assert shapes(33, pass_="bwd") == [("pl_bf16", 32), ("pl_bf16", 1)]
    assert shapes(33, {"bwd_bf16": 0}, "bwd") == [("pl_m44", 32), ("pl_exact+split32", 1)]
    assert shapes(65, pass_="fwd") == [("fwd_mf<128>", 65)]
    assert shapes(65, {"fwd_wide": 0}, "fwd") == [("fwd_mf<64>", 64), ("fwd<4,1>", 1)]
    assert shapes(97, pass_="bwd") == [("pl_bf16", 32), ("pl_kernel8", 65)]
    assert shapes(97, {"bwd_bf16": 0}, "bwd") == [("pl_m44", 32), ("pl_exact", 64), ("pl_exact+split32", 1)]
    assert shapes(131, pass_="fwd") == [("fwd_mf<128>", 128), ("fwd<4,1>", 3)]
    assert shapes(137, pass_="fwd") == [("fwd_mf<128>", 128), ("fwd_mf<16>", 9)]
    assert shapes(150, pass_="fwd") == [("fwd_mf<128>", 128), ("fwd_mf<32>", 22)]
    assert shapes(161, pass_="fwd") == [("fwd_mf<128>", 128), ("fwd_mf<64>", 33)]
    assert shapes(161, pass_="bwd") == [("pl_bf16", 32), ("pl_kernel8", 128), ("pl_bf16", 1)]
    assert shapes(193, pass_="fwd") == [("fwd_mf<128>", 128), ("fwd_mf<128>", 65)]
    assert shapes(257, pass_="fwd") == [("fwd_mf<128>", 128), ("fwd_mf<128>", 128), ("fwd<4,1>", 1)]
    assert shapes(257, pass_="bwd") == [("pl_bf16", 32), ("pl_kernel8", 128), ("pl_kernel8", 97)]
    assert shapes(7, {"bwd_bf16": 0}, "bwd") == [("pl_m44+split16", 7)]
    assert shapes(2, {"bwd_bf16": 0}, "bwd") == [("il<4>", 2)]
    assert shapes(131, {"bwd_pl": 0}, "bwd") == [("il<64,mf>", 64), ("il<64,mf>", 64), ("il<4>", 3)]
    assert shapes(81, {"feature_mfma": 0}) == [("fwd<64,1>", 64), ("fwd<32,2>", 17), ("il<64>", 64), ("il<32>", 17)]
    assert window_plan(31, {}, long_frame=True)[1]["shape"] == "pl_hyb"
    assert kernel_name(window_plan(137, {})[1]) == "render_forward_mfma_kernel_w4<16, false>"
    assert kernel_name(window_plan(33, {})[2]) == "render_backward_pl_kernel<false, 1, true, false, true>"


# ------------------------------------------------------------------------------------------------------------ the GPU sweep --
def _sweep_scene(C: int, family: str):
    """A small scene with a ragged tile grid (113 x 75 or 160 x 96), depth gradients on every other width, channels told apart.
    Every (family, C) draws its own scene: an output plane a kernel fails to write must not find the right values left in a
    recycled allocation by an earlier case of the same width."""
    import torch
    from synth import make_scene
    i = CHANNELS.index(C)
    W, H = ((113, 75), (160, 96))[i % 2]
    # scales within a factor 8 of each other: no Gaussian above the default bwd_bf16_max_ratio (16), so the defaults take bf16
    sc = make_scene(P=3000 + 50 * i, C=C, width=W, height=H, seed=500 + C + 1000 * list(FAMILIES).index(family),
                    with_depth_grad=(i // 2) % 2 == 0, scale_lo=0.01, scale_hi=0.08)
    s = torch.from_numpy(channel_scale(C)).float()
    sc["semantic_feature"] = (sc["semantic_feature"] * s).contiguous()
    sc["dL_dfeature"] = (sc["dL_dfeature"] / s[:, None, None]).contiguous()
    return sc


SWEEP = [(f, C) for f in FAMILIES for C in (H_CHANNELS if f == "H" else CHANNELS)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,C", SWEEP, ids=[f"{f}-C{C}" for f, C in SWEEP])
def test_channel_window_sweep_matches_the_oracle(family, C, option):
    """One (family, C): the HIP path against the CPU oracle at the north-star bars (tests/util.py: _strict_compare), plus the
    per-channel bars: feature-map channel c within 1e-4 s_c, column c of dL_dsemantic_feature held to the gradient bars alone."""
    from diff_gaussian_rasterization import _C
    opts, contraction = FAMILIES[family]
    for k, v in opts.items():
        option(k, v)
    _strict_compare(_sweep_scene(C, family), channel_scale=channel_scale(C))
    if contraction is not None:
        assert _C.last_backward_contraction() == contraction
