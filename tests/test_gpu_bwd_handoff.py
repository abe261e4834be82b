"""The bf16 hand-off of the pixel-lane blend backward at the edges its entry pairing creates.

Phase 1 of the bf16 shape (csrc/pl_phase1.h) converts and stores the blend weights w and the dL/dalpha terms s of two list
entries at a time, four entries to an 8-byte slot of a per-pixel row; phase 2 (csrc/render_bwd_pl.hip) reads the rows back
transposed.  What that pairing can get wrong shows at the ends of a tile's list: a deepest list position that is odd, 1 mod 4, or
not a multiple of the 16-entry chunk (a pair or a slot cut by the list end, whose missing entries must read as zeros), at a
window edge (64 entries), and in tiles where one quadrant alone holds the hits (the other three write zeros).  The scenes below
place, per 16 x 16 tile, exactly `depth` faint Gaussians around one pixel of one quadrant, so that tile's deepest list position
is `depth`; channel widths leave later windows of odd widths for the four- and eight-wave later-window kernels.
"""

import numpy as np
import pytest
import torch

from util import precompute_optionals, run_hip

# deepest list position per tile: odd, 1 mod 4, not a multiple of 16, at and across the chunk and window edges
DEPTHS = [1, 2, 3, 5, 7, 9, 13, 15, 16, 17, 21, 29, 31, 32, 33, 37, 45, 49, 63, 64, 65, 67, 71, 81, 97, 101, 113, 127, 129, 133]
TX, TY = 6, 5                  # tiles of the image: 96 x 80 pixels
# 1: one later window of 1 channel; 33, 45: later windows of 1 / 13 channels; 99: an eight-wave later window of 67;
# 161: eight waves on 128, then four on 1
CHANNELS = [1, 7, 32, 33, 45, 99, 161]


def handoff_scene(C: int, seed: int) -> dict:
    """Tile i (row-major) holds DEPTHS[i] Gaussians, all around one pixel of quadrant i mod 4, at distinct depths; opacity
    0.06 - 0.1 and ~1 px wide, so every one blends (transmittance stays far above its cut-off) and none reaches another quadrant
    or tile (radius 3 px from a pixel 4 px inside the quadrant)."""
    from synth import make_scene
    W, H = 16 * TX, 16 * TY
    P = sum(DEPTHS)
    sc = make_scene(P=P, C=C, width=W, height=H, seed=seed, with_depth_grad=True)
    g = torch.Generator().manual_seed(seed + 1)
    tx, ty = sc["tanfovx"], sc["tanfovy"]
    means, scales, opac = [], [], []
    for i, d in enumerate(DEPTHS):
        q = i % 4
        cx = 16 * (i % TX) + 8 * (q & 1) + 3.5 + 0.5 * ((i // TX) % 2)
        cy = 16 * (i // TX) + 8 * (q >> 1) + 3.5
        for k in range(d):
            z = 3.0 + 0.05 * k + 0.01 * float(torch.rand(1, generator=g))
            px = cx + float(torch.rand(1, generator=g)) - 0.5
            py = cy + float(torch.rand(1, generator=g)) - 0.5
            u, v = (2 * px + 1) / W - 1, (2 * py + 1) / H - 1
            means.append([u * tx * z, v * ty * z, z])
            s = 0.5 * 2 * tx * z / W                      # half a pixel at depth z
            scales.append([s, s * (0.8 + 0.4 * float(torch.rand(1, generator=g))), s])
            opac.append(0.06 + 0.04 * float(torch.rand(1, generator=g)))
    sc["means3D"] = torch.tensor(means, dtype=torch.float32)
    sc["scales"] = torch.tensor(scales, dtype=torch.float32)
    sc["opacities"] = torch.tensor(opac, dtype=torch.float32)[:, None].contiguous()
    return sc


def _deepest_positions(scene) -> np.ndarray:
    """Per tile: the largest n_contrib of its pixels (the CPU oracle's forward), i.e. the deepest list position phase 1 walks."""
    from util import run_oracle
    o, out, _ = run_oracle(scene, backward=False)
    n = o.read("n_contrib").astype(np.int64).reshape(16 * TY, 16 * TX)
    return n.reshape(TY, 16, TX, 16).max(axis=(1, 3)).reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("C", CHANNELS)
def test_bf16_handoff_matches_the_exact_contraction(C, option):
    """bf16 two-term contraction (option bwd_bf16 = 1) against the exact-fp32 one (0) on the edge scene: images bit-identical,
    every gradient element within 1e-4 |g| + 1e-5 max|g| (the bar of test_gpu_parity.py)."""
    sc = handoff_scene(C, seed=900 + C)
    option("bwd_bf16", 1)
    out1, g1 = run_hip(sc)
    option("bwd_bf16", 0)
    out0, g0 = run_hip(sc)
    for k in ("color", "feature_map", "depth", "radii"):
        assert np.array_equal(out1[k], out0[k]), k
    worst = {}
    for k, a in g1.items():
        if a is None or a.size == 0:
            continue
        b = g0[k].astype(np.float64)
        scale = float(np.abs(b).max()) + 1e-30
        worst[k] = float((np.abs(a - b) / (1e-4 * np.abs(b) + 1e-5 * scale)).max())
    print(f"C={C} bf16 vs fp32, worst element / (1e-4 |g| + 1e-5 max|g|):", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("C", [7, 33, 99])
def test_bf16_handoff_matches_the_reference(C, option):
    """The default contraction (bwd_bf16 = -1: bf16 on this well-conditioned scene) against the compiled reference, at the bars
    of test_gpu_vs_ref.py."""
    from test_gpu_vs_ref import _compare
    ref_c = min(c for c in (16, 32, 64, 128, 256, 512) if c >= C)
    st = _compare(precompute_optionals(handoff_scene(C, seed=950 + C)), ref_c)
    print(C, st)


def test_the_scene_reaches_the_listed_depths():
    """CPU: in every tile the deepest list position that blends is exactly the number of Gaussians placed there."""
    sc = handoff_scene(3, seed=7)
    assert sc["P"] == sum(DEPTHS) and len(DEPTHS) == TX * TY
    got = _deepest_positions(sc)
    assert got.tolist() == DEPTHS, got.tolist()
    assert {d % 2 for d in DEPTHS} == {0, 1} and any(d % 4 == 1 for d in DEPTHS) and any(d > 128 for d in DEPTHS)
