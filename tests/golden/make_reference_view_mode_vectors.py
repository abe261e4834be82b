"""Generates tests/golden/reference_view_modes.npz by IMPORTING the reference's own utils.image_utils (depth_to_normal,
gradient_map, colormap, render_net_image) and running it on CPU, in float32 (what the fixture records) and once more in
float64 (to show that tests/view_modes_oracle.py restates the reference's function: the two agree to 1e-9).

`Tensor.cuda` is the identity for the run, modules that utils.image_utils imports and that are missing are stubbed, and
`plt.cm.get_cmap`, which newer matplotlib releases no longer have, is pointed at `matplotlib.colormaps`.  Per case
(tests/view_modes_oracle.py: FIXTURE_CASES) the fixture holds

  depth cases   depth, projection_matrix, full_proj_transform (the inputs), normals (H, W, 3) and curvature (H, W) as the
                reference's float32 chain returned them, the palette indices of its 'Depth' and 'Curvature' frames (uint8;
                the generator checks that the frame IS turbo[index]) and of matplotlib's own `jet(depth / max)` call
                (render.py:155-161), and
                e_normals, e_curvature   median, 99th percentile and maximum of |reference float32 - float64 oracle| over the
                                         pixels whose depth footprint holds no zero (all pixels where there is no hole)
                band_depth, band_curvature   the share of pixels whose float64 scaled value lies inside the index band
  image cases   image (the input), edge (H, W) float32, its palette indices, e_edge and band_edge likewise
  turbo, jet    the two 256-entry tables: data the reference reads at run time

Run it where the reference and matplotlib exist (the tests read only the npz):

    python tests/golden/make_reference_view_mode_vectors.py
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
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {})


def _import_reference_image_utils():
    for name in ("sklearn", "sklearn.decomposition"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Anything(name)
    import matplotlib
    import matplotlib.pyplot as plt
    if not hasattr(plt.cm, "get_cmap"):
        plt.cm.get_cmap = lambda name: matplotlib.colormaps[name]
    sys.path.insert(0, REF)
    return importlib.import_module("utils.image_utils")


class _Float64:
    """the reference's code in float64: new tensors are double and `.float()` keeps them so"""

    def __enter__(self):
        self.float = torch.Tensor.float
        torch.set_default_dtype(torch.float64)
        torch.Tensor.float = lambda t: t.double()

    def __exit__(self, *exc):
        torch.set_default_dtype(torch.float32)
        torch.Tensor.float = self.float


def _index_of(frame, lut):
    """(H, W) uint8 with frame == lut[index] exactly; frame (3, H, W)"""
    px = frame.transpose(1, 2, 0).reshape(-1, 1, 3)
    hit = (px == lut[None]).all(-1)
    assert hit.any(1).all(), "a colour of the frame is not a row of the table"
    return hit.argmax(1).astype(np.uint8).reshape(frame.shape[1:])


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import view_modes_oracle as O
    U = _import_reference_image_utils()
    torch.Tensor.cuda = lambda self, *a, **k: self
    import matplotlib
    turbo = np.asarray(matplotlib.colormaps["turbo"].colors, np.float32)
    jet_cm = matplotlib.colormaps["jet"]
    jet = np.asarray(jet_cm(np.arange(256))[:, :3], np.float32)
    assert turbo.shape == jet.shape == (256, 3)
    items = ["RGB", "Depth", "Edge", "Normal", "Curvature", "Feature Map"]
    out = {"turbo": turbo, "jet": jet}

    def band(field):
        share = float(O.in_band(field).mean())
        assert share <= O.BAND_CAP, ("re-seed the case", share)
        return np.float64(share)

    for name in O.DEPTH_CASES:
        depth, proj, full = O.make_inputs(name)
        cam = O.Camera(torch.from_numpy(proj), torch.from_numpy(full))
        pkg = {"depth": torch.from_numpy(depth)[None]}
        n32 = U.depth_to_normal(pkg["depth"], cam).numpy()
        img_n = U.render_net_image(pkg, items, 3, cam).numpy()
        c32 = U.gradient_map((U.depth_to_normal(pkg["depth"], cam).permute(2, 0, 1) + 1) / 2)[0].numpy()
        frame_c = U.render_net_image(pkg, items, 4, cam).numpy()
        frame_d = U.render_net_image(pkg, items, 1, cam).numpy()
        assert n32.dtype == c32.dtype == frame_c.dtype == np.float32 and np.array_equal(img_n, (n32.transpose(2, 0, 1) + 1) / 2)
        with _Float64():
            cam64 = O.Camera(torch.from_numpy(proj).double(), torch.from_numpy(full).double())
            d64 = torch.from_numpy(depth).double()[None]
            n64 = U.depth_to_normal(d64, cam64).numpy()
            c64 = U.gradient_map((U.depth_to_normal(d64, cam64).permute(2, 0, 1) + 1) / 2)[0].numpy()
        want_n, want_c = O.depth_to_normal(depth, proj, full), O.curvature(depth, proj, full)
        # 1e-9 everywhere but at the corner pixel: there both vectors are -p1, numpy's cross product is exactly 0 and torch's
        # (fused multiply-add) leaves a residue of one rounding, which the division by 0 + 1e-8 lifts to 1e-8.  The oracle and
        # the kernels say 0; the residue reaches the curvature of the corner's 2 x 2 block.
        # Pixels with a zero in their depth footprint are left out as well: next to the zero padding their two vectors are
        # parallel to within 1e-8 and the cross product cancels to 2e-8 even in float64 (the GPU tests ask only for finite
        # values there).
        near = np.zeros(depth.shape, bool)
        near[-2:, -2:] = True
        clean_n, clean_c = O.clean_footprint(depth, 0, 1), O.clean_footprint(depth, 1, 2)
        corner = np.zeros(depth.shape, bool)
        corner[-1, -1] = True
        d_n, d_c = np.abs(n64 - want_n).max(-1), np.abs(c64 - want_c)
        assert n64.dtype == np.float64 and d_n[clean_n & ~corner].max(initial=0) <= 1e-9 and d_n[-1, -1] <= 1e-7, name
        assert d_c[clean_c & ~near].max(initial=0) <= 1e-9 and d_c[clean_c & near].max(initial=0) <= 1e-7, name
        e_n = O.error_stats(n32, want_n, O.clean_footprint(depth, 0, 1))
        e_c = O.error_stats(c32, want_c, O.clean_footprint(depth, 1, 2))
        idx_c, idx_d = _index_of(frame_c, turbo), _index_of(frame_d, turbo)
        jet_rgba = jet_cm((torch.from_numpy(depth) / float(depth.max())).numpy())
        idx_j = _index_of(np.asarray(jet_rgba[..., :3], np.float32).transpose(2, 0, 1), jet)
        out.update({f"{name}/depth": depth, f"{name}/projection_matrix": proj, f"{name}/full_proj_transform": full,
                    f"{name}/normals": n32, f"{name}/curvature": c32, f"{name}/e_normals": e_n, f"{name}/e_curvature": e_c,
                    f"{name}/idx_depth": idx_d, f"{name}/idx_curvature": idx_c, f"{name}/idx_jet": idx_j,
                    f"{name}/band_depth": band(depth), f"{name}/band_curvature": band(want_c)})
        print(f"{name:24s} e_normals {e_n[0]:.1e} {e_n[1]:.1e} {e_n[2]:.1e}  e_curvature {e_c[0]:.1e} {e_c[1]:.1e} {e_c[2]:.1e}  "
              f"idx: depth {int((idx_d != O.colormap_index(depth)).sum())} curvature "
              f"{int((idx_c != O.colormap_index(want_c)).sum())} jet {int((idx_j != O.max_index(depth)).sum())} pixels off the oracle")

    for name in O.IMAGE_CASES:
        img = O.make_inputs(name)
        pkg = {"render": torch.from_numpy(img)}
        e32 = U.gradient_map(pkg["render"])[0].numpy()
        with _Float64():
            e64 = U.gradient_map(torch.from_numpy(img).double())[0].numpy()
        want = O.gradient_map(img)
        assert e32.dtype == np.float32 and e64.dtype == np.float64 and np.abs(e64 - want).max() <= 1e-9, name
        e_e = O.error_stats(e32, want)
        out.update({f"{name}/image": img, f"{name}/edge": e32, f"{name}/e_edge": e_e, f"{name}/band_edge": band(want)})
        if want.max() > want.min():
            frame = U.render_net_image(pkg, items, 2, None).numpy()
            out[f"{name}/idx_edge"] = _index_of(frame, turbo)
        print(f"{name:24s} e_edge {e_e[0]:.1e} {e_e[1]:.1e} {e_e[2]:.1e}")

    path = os.path.join(HERE, "reference_view_modes.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(O.FIXTURE_CASES)} cases)")


if __name__ == "__main__":
    main()
