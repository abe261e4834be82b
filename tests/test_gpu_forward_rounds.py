"""The blend forward's rounds of 64 list positions and its queue of compacted entries (option fwd_round = 64, the default) against
the rounds of 32 (fwd_round = 32) on the designed lists of tests/forward_round_cases.py: list lengths on both sides of every
round and chunk edge, four hit patterns, the 5-, 16- and 32-channel shapes.  The two loops blend the same entries in the same
order: colour, feature map, depth, n_contrib, final T and tile_len are bit-equal, the images hold the forward bars against the
scalar oracle (1e-4 absolute outside proven threshold flips), and one backward after each forward gives gradients equal up to
the order of the atomic sums (2e-5 of the tensor's largest magnitude: the bound of test_scheduling_options_keep_the_results).

C = 40 runs as one 64-channel window (the 32-candidate loop under either setting); the LATER windows that take the new loop are
those of C = 137 (128 + 9: the 16-channel shape without its colour half) and C = 150 (128 + 22: the 32-channel one)."""
import functools

import numpy as np
import pytest
import torch

import forward_round_cases as fr
import refutil as ru
from util import run_oracle

pytestmark = pytest.mark.gpu

CASES = [(L, p, C) for C in (5, 16, 32) for p in fr.PLACEMENTS for L in fr.LENGTHS]
CASES += [(129, "full", 40), (97, "opaque", 40), (129, "full", 137), (95, "alt", 137), (200, "opaque", 137), (129, "full", 150),
          (65, "quad", 150), (200, "opaque", 150)]


@functools.lru_cache(maxsize=None)
def _oracle(L, placement, C):
    o, out, _ = run_oracle(fr.scene(L, placement, C), backward=False)
    want = dict(color=out["color"].copy(), feature_map=out["feature_map"].copy(), depth=out["depth"].copy(),
                n_contrib=o.read("n_contrib").copy(), final_T=o.read("final_T").copy(), ranges=o.read("ranges").copy())
    for v in want.values():
        v.setflags(write=False)
    return want


def _run(sc, C):
    mod = ru.product_module()
    d = ru.device_inputs(sc, C, "cuda:0")
    f = ru.raw_forward(mod, sc, d)
    W, H = sc["image_width"], sc["image_height"]
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    st = dict(color=f[1].cpu().numpy(), feature_map=f[2].cpu().numpy(), depth=f[3].cpu().numpy(), radii=f[4].cpu().numpy(),
              n_contrib=ru.product_read("n_contrib", sc, f, np.uint32, W * H), final_T=ru.product_read("final_T", sc, f, np.float32, W * H),
              tile_len=ru.product_read("tile_len", sc, f, np.uint32, tiles), ranges=ru.product_read("ranges", sc, f, np.uint32, 2 * tiles))
    g = {k: v.cpu().numpy() for k, v in ru.raw_backward(mod, sc, d, f).items()}
    return st, g


@pytest.mark.parametrize("L,placement,C", CASES, ids=[f"L{L}-{p}-C{C}" for L, p, C in CASES])
def test_rounds_of_64_blend_what_rounds_of_32_blend(L, placement, C, option):
    option("tile_cull", 0)            # the designed lists are the reference's
    sc = fr.scene(L, placement, C)
    want = _oracle(L, placement, C)
    option("fwd_round", 64)
    s64, g64 = _run(sc, C)
    option("fwd_round", 32)
    s32, g32 = _run(sc, C)
    # the list is the designed one
    assert np.array_equal(s64["ranges"], want["ranges"])
    lo, hi = s64["ranges"].reshape(-1, 2)[sc["case"]["tile_index"]]
    assert int(hi) - int(lo) == L
    # bit-equal between the two loops
    for k in ("color", "feature_map", "depth", "radii", "n_contrib", "final_T", "tile_len", "ranges"):
        assert np.array_equal(s64[k], s32[k]), k
    W, H = sc["image_width"], sc["image_height"]
    n = s64["n_contrib"].reshape(H, W).astype(np.int64)
    assert np.array_equal(s64["tile_len"], n.reshape(H // 16, 16, W // 16, 16).max(axis=(1, 3)).reshape(-1))
    # the forward bars against the oracle
    flips = ru.flip_pixels(dict(n_contrib=want["n_contrib"], final_T=want["final_T"]), s64)
    assert int(flips.sum()) <= 2, f"{int(flips.sum())} threshold-flip pixels"
    ok = ~flips
    for k in ("color", "feature_map", "depth"):
        err = np.abs(s64[k] - want[k]).reshape(want[k].shape[0], -1).max(0)
        assert err[ok].max() <= 1e-4, (k, float(err[ok].max()))
    # one backward after each: equal up to the order of the atomic sums
    for k, a in g64.items():
        if a.size == 0:
            continue
        b = g32[k]
        scale = float(np.abs(b).max()) + 1e-30
        assert float(np.abs(a - b).max()) <= 2e-5 * scale, (k, float(np.abs(a - b).max()) / scale)
