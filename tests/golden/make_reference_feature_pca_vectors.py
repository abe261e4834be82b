"""Generates tests/golden/reference_feature_pca.npz by IMPORTING the reference's own render.feature_visualize_saving
(render.py:38-53) and running it on CPU.

The modules render.py imports that are not needed for this function (`scene`, `gaussian_renderer`, `torchvision`, `cv2`,
`clip`, `utils.clip_utils`) are stubbed in sys.modules where they are missing, and `Tensor.cuda` is the identity for the run.
Per case (tests/feature_pca_oracle.py: FIXTURE_CASES) the fixture holds the input map, the image the reference returned and
the errors of the float32 chain against the float64 oracle - the yardstick of the GPU tests:
    e_img    max |reference image - oracle image|
    e_cov    max |cov32 - cov64| / max |cov64|, cov32 = torch's float32 centred covariance of the float32-normalised samples
    e_mean   max |mean32 - mean64|, mean32 = the reference's own `f_samples.mean(0)`
    exact    0 where scikit-learn's PCA(3) picks its RANDOMIZED solver for the case's samples (more than 500 channels): the
             reference's error is then that solver's approximation (1e-5 to 1e-3 of a component here), not float32 rounding,
             and the case does not enter the GPU tests' yardstick
Run it where the reference and scikit-learn exist (the tests read only the npz):

    python tests/golden/make_reference_feature_pca_vectors.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


class _Anything(types.ModuleType):
    """A stub module: every attribute is a placeholder class."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def _import_reference_render():
    for name in ("scene", "gaussian_renderer", "torchvision", "cv2", "clip", "utils.clip_utils", "matplotlib",
                 "matplotlib.pyplot", "yaml", "tqdm", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Anything(name)
            if "." in name:
                parent, child = name.rsplit(".", 1)
                if parent in sys.modules:
                    setattr(sys.modules[parent], child, sys.modules[name])
    return importlib.import_module("render")


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import feature_pca_oracle as O
    sys.path.insert(0, REF)
    render = _import_reference_render()
    torch.Tensor.cuda = lambda self, *a, **k: self

    out = {}
    for name in O.FIXTURE_CASES:
        f = O.make_inputs(name)
        want = O.oracle(f, 3)
        got = render.feature_visualize_saving(torch.from_numpy(f.copy()))
        assert got.dtype == torch.float32 and tuple(got.shape) == (f.shape[1], f.shape[2], 3)
        img = got.numpy()
        e_img = float(np.abs(img.astype(np.float64) - want.image).max())
        s = torch.nn.functional.normalize(torch.from_numpy(f.copy())[None], dim=1)[0].permute(1, 2, 0).reshape(-1, f.shape[0])[::3]
        z = s - s.mean(0, keepdim=True)
        cov32 = (z.t() @ z / (s.shape[0] - 1)).numpy().astype(np.float64)
        e_cov = float(np.abs(cov32 - want.cov).max() / np.abs(want.cov).max())
        e_mean = float(np.abs(s.numpy().mean(0).astype(np.float64) - want.mean).max())
        import sklearn.decomposition
        probe = sklearn.decomposition.PCA(3, random_state=42).fit(s.numpy())
        exact = probe._fit_svd_solver != "randomized"
        assert e_img < (1e-5 if exact else 1e-3), (name, e_img)          # the float64 restatement IS the reference's function
        out[f"{name}/exact"] = np.int64(exact)
        out[f"{name}/feature"], out[f"{name}/image"] = f, img
        out[f"{name}/e_img"], out[f"{name}/e_cov"], out[f"{name}/e_mean"] = np.float64(e_img), np.float64(e_cov), np.float64(e_mean)
        print(f"{name}: exact {int(exact)} gaps {['%.3f' % g for g in O.gaps_of(f)]} e_img {e_img:.2e} e_cov {e_cov:.2e} e_mean {e_mean:.2e}")
    path = os.path.join(HERE, "reference_feature_pca.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(O.FIXTURE_CASES)} cases)")


if __name__ == "__main__":
    main()
