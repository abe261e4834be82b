"""CPU tests of the general-camera family (tests/util.py: general_view_scene): a camera with an arbitrary rotation, away
from the origin, with fx != fy, and SH inputs of every width.  (i) its matrices are the reference Camera's, frozen by
tests/golden/make_reference_camera_vectors.py; (ii) on such inputs the analytic backward of the C++ oracle equals the fp64
autograd restatement, as tests/test_oracle.py shows for the camera at the origin."""
import os

import numpy as np
import pytest
import torch

import refutil as ru
from util import ROOT, VIEWS, DEGREE_OF_M, assert_input_conditions, general_camera, grad_report, precompute_optionals, run_oracle, view_scene

GOLD = os.path.join(ROOT, "tests", "golden")


def test_general_cameras_match_the_reference_camera_class():
    """general_camera hands the op what the reference's getWorld2View2 / getProjectionMatrix / Camera composition give for
    the same R, T, FoVx, FoVy (tolerances of test_synthetic_cameras_match_the_reference_camera_class)."""
    g = np.load(os.path.join(GOLD, "reference_cameras.npz"))
    assert len(g["ids"]) == 8
    seen = set()
    for k, prm in zip(g["ids"], g["params"]):
        name, size = str(k).split("_")
        W, H = int(prm[0]), int(prm[1])
        assert size == f"{W}x{H}"
        v = VIEWS[name]
        assert [v["yaw"], v["pitch"], v["roll"], *v["campos"], v["fovx_deg"], v["pix_aspect"], v["znear"], v["zfar"]] == list(prm[2:]), k
        cam = general_camera(W, H, **v)
        # the same R, T (the reference stores the camera-to-world rotation) and fields of view went into both
        assert np.allclose(cam["R"].T, g[f"{k}_R"], rtol=0, atol=1e-15) and np.allclose(cam["t"], g[f"{k}_T"], rtol=0, atol=1e-15), k
        assert np.allclose(cam["viewmatrix"].numpy(), g[f"{k}_view"], rtol=0, atol=1e-7), k
        assert np.allclose(cam["projmatrix"].numpy(), g[f"{k}_full"], rtol=1e-6, atol=1e-7), k
        assert np.allclose(cam["campos"].numpy(), g[f"{k}_center"], rtol=0, atol=1e-7), k
        assert np.allclose([cam["tanfovx"], cam["tanfovy"]], g[f"{k}_tan"], rtol=1e-12), k
        # the camera position that went in comes back out
        assert np.allclose(cam["campos"].numpy(), v["campos"], rtol=0, atol=1e-6), k
        seen.add((name, W > H))
    assert seen == {(n, o) for n in "ABCD" for o in (True, False)}      # every view in landscape and in portrait


def test_general_view_scene_keeps_the_recipe():
    """The builder keeps make_scene's Gaussians: seen through its own camera they sit where make_scene put them (x, y
    rescaled to the frustum); view E is make_scene's camera itself; `shs` is cut to M coefficients."""
    from synth import make_scene
    base = make_scene(P=500, C=3, width=96, height=64, seed=3, sh_degree=1)
    e = view_scene("E", 500, 3, 96, 64, 3, M=4)
    for k in ("viewmatrix", "projmatrix", "campos", "means3D", "scales", "rotations", "opacities", "semantic_feature", "dL_dcolor"):
        assert torch.equal(e[k], base[k]), k
    assert (e["tanfovx"], e["tanfovy"], e["sh_degree"], e["M"]) == (base["tanfovx"], base["tanfovy"], 1, 4)
    assert torch.equal(e["shs"], base["shs"][:, :4]) and e["shs"].is_contiguous()
    for name in "ABCD":
        sc = view_scene(name, 500, 3, 96, 64, 3, M=9)
        assert sc["shs"].shape == (500, 9, 3) and sc["sh_degree"] == 2
        m = torch.cat([sc["means3D"].double(), torch.ones(500, 1, dtype=torch.float64)], 1) @ sc["viewmatrix"].double()
        want = base["means3D"].double().clone()
        want[:, 0] *= sc["tanfovx"] / base["tanfovx"]
        want[:, 1] *= sc["tanfovy"] / base["tanfovy"]
        assert float((m[:, :3] - want).abs().max()) < 2e-5, name      # positions of up to 20 units rounded to fp32 twice
        assert "colors_precomp" in precompute_optionals(sc)


# view, M, (W, H), seed: seeds chosen on the CPU so that every case holds the input conditions asserted below
CPU_CASES = [("A", 16, (96, 64), 1), ("A", 16, (48, 80), 1), ("B", 4, (96, 64), 1), ("B", 4, (48, 80), 1), ("C", 9, (96, 64), 1),
             ("C", 9, (48, 80), 5), ("D", 5, (96, 64), 1), ("D", 5, (48, 80), 1), ("E", 1, (96, 64), 2), ("E", 1, (48, 80), 10)]


@pytest.mark.parametrize("view,M,size,seed", CPU_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_analytic_backward_equals_torch_autograd_under_general_views(oracle_lib, view, M, size, seed):
    """tests/test_oracle.py::test_analytic_backward_equals_torch_autograd with its bars (images 5e-5, gradients mx < 2e-4 and
    bad < 1e-3) on general cameras and SH widths.  One correction: a threshold flip can leave n_contrib equal (an alpha flip in
    front of the last contributor), so the pixels where the two evaluations provably decided differently are found from
    n_contrib AND final T (refutil.flip_pixels), counted against max(2, npix // 10000), and removed exactly by zeroing their
    upstream gradients on both sides."""
    from oracle import torch_oracle
    W, H = size
    sc = view_scene(view, 1500, 5, W, H, seed, M=M, with_depth_grad=True, scale_lo=0.02, scale_hi=0.25, wide_scale=3.0)
    assert sc["sh_degree"] == DEGREE_OF_M[M] and sc["shs"].shape == (1500, M, 3)
    o, out, _ = run_oracle(sc, backward=False)
    assert_input_conditions(sc, out["radii"], o.read("clamped"), view)
    r = torch_oracle.forward_backward(sc, dtype=torch.float64)
    to = r["out"]
    assert out["num_rendered"] == to["num_rendered"]
    assert np.array_equal(out["radii"], to["radii"].numpy())
    assert np.array_equal(o.read("point_list"), to["point_list"])
    flips = ru.flip_pixels(dict(n_contrib=o.read("n_contrib"), final_T=o.read("final_T")),
                           dict(n_contrib=to["n_contrib"].reshape(-1).astype(np.uint32), final_T=to["final_T"].numpy().reshape(-1)))
    nflip = int(flips.sum())
    assert nflip <= max(2, W * H // 10000), f"{nflip} threshold-flip pixels"
    ok = ~flips.reshape(H, W)
    for k in ("color", "feature_map", "depth"):
        err = np.abs(out[k] - to[k].detach().numpy())[..., ok]
        print(view, M, size, k, "max abs err", err.max(), "flips", nflip)
        assert err.max() < 5e-5, (k, err.max())
    up = tuple(sc[k] * torch.from_numpy(ok)[None] for k in ("dL_dcolor", "dL_dfeature", "dL_ddepth"))
    if nflip:
        r = torch_oracle.forward_backward(sc, dtype=torch.float64, upstream=up)
    g = o.backward(*up)
    pairs = {"dL_dmeans3D": "means3D", "dL_dmeans2D": "means2D", "dL_dopacity": "opacities", "dL_dsemantic_feature": "semantic_feature",
             "dL_dsh": "shs", "dL_dscales": "scales", "dL_drotations": "rotations"}
    for a, b in pairs.items():
        assert g[a].size and float(np.abs(g[a]).max()) > 0, a
        mx, bad = grad_report(a, g[a], r["grads"][b].numpy().reshape(g[a].shape), rel=1e-3)
        print(view, M, size, a, "mx", mx, "bad", bad)
        assert mx < 2e-4 and bad < 1e-3, (a, mx, bad)
    assert g["dL_dsh"].shape == (1500, M, 3)
