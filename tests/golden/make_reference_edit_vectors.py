"""Generates tests/golden/reference_edit_vectors.npz by IMPORTING the reference's own selection functions
(gaussian_renderer/__init__.py:21-55: calculate_selection_score, calculate_selection_score_delete) and running them on CPU.

The module's imports are stubbed as tests/test_gpu_dropin.py stubs them (`scene.gaussian_model`; the rasterizer resolves
to this repository's package, which imports without a GPU).  On CPU the K = 1 branch of both functions and the thresholded
select branch run; the argmax / isin branches call `.cuda()` and are covered live by tests/test_gpu_edit.py instead.  The
fixture holds seeded inputs (tests/edit_oracle.py: make_inputs, with a zero, an inf and a NaN row in one case) and the masks
the reference returned.  torch's CPU comparison rounds the threshold to fp16 (`scalar="fp16"` in the oracle).  Run it where
the reference exists (the tests read only the npz):

    python tests/golden/make_reference_edit_vectors.py
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

# name: (P, C, K, seed, threshold, positive_ids, functions, special rows)
CASES = {
    "k1_c16": (1500, 16, 1, 11, 0.887, [0], ("select", "delete"), False),
    "k5_c16_thr0198": (1500, 16, 5, 12, 0.198, [0], ("select",), True),
    "k5_c64_two_positives": (500, 64, 5, 13, 0.4, [2, 0], ("select",), False),
    "k2_c16_second": (1000, 16, 2, 14, 0.5, [1], ("select",), False),
    "k1_c64_delete": (400, 64, 1, 15, 0.92, [0], ("delete",), False),
}


def main():
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "feature-3dgs_amd"), ROOT):
        sys.path.insert(0, p)
    import edit_oracle as O
    scene_pkg, gm = types.ModuleType("scene"), types.ModuleType("scene.gaussian_model")
    gm.GaussianModel = type("GaussianModel", (), {})
    scene_pkg.gaussian_model = gm
    sys.modules.update({"scene": scene_pkg, "scene.gaussian_model": gm})
    sys.path.append(REF)
    import gaussian_renderer as ref  # noqa: E402  (reference code)
    fns = {"select": ref.calculate_selection_score, "delete": ref.calculate_selection_score_delete}

    out = {}
    for name, (P, C, K, seed, thr, pos, which, special) in CASES.items():
        f, t = O.make_inputs(P, C, K, seed)
        if special:
            f[0] = 0.0
            f[1, 0] = np.inf
            f[2, C - 1] = np.nan
        out[f"{name}/features"], out[f"{name}/text"] = f, t
        out[f"{name}/threshold"], out[f"{name}/positive_ids"] = np.float64(thr), np.asarray(pos, np.int64)
        for v in which:
            ft, tt = torch.from_numpy(f.copy()), torch.from_numpy(t.copy())
            m = fns[v](ft, tt, score_threshold=thr, positive_ids=list(pos))
            assert m.dtype == torch.float32 and m.shape == (P,)
            out[f"{name}/mask_{v}"] = m.numpy().astype(np.uint8)
            if v == which[0]:
                out[f"{name}/text_normalized"] = tt.numpy()          # the in-place side effect on query_features
    path = os.path.join(HERE, "reference_edit_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(CASES)} cases)")


if __name__ == "__main__":
    main()
