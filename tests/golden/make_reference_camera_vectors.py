"""Generates tests/golden/reference_cameras.npz by IMPORTING the reference's own camera code.

The general-view tests (tests/util.py: general_view_scene) hand the op cameras with an arbitrary rotation, a position away
from the origin and independent fields of view.  This script freezes what the reference builds for the same R, T, FoVx,
FoVy: `getWorld2View2` and `getProjectionMatrix` (utils/graphics_utils.py:38-71) composed as its Camera class composes
them (scene/cameras.py:55-58), for views A-D of tests/util.py at a landscape and a portrait size.  The rotation is
written out here on its own, from the angles, so that the fixture does not share tests/util.py's arithmetic.  Matrices
and scalars only.  Run where the reference can be imported:

    python tests/golden/make_reference_camera_vectors.py
"""
import math
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(160, 96), (96, 160)]
# id: yaw, pitch, roll (degrees), camera position (world), fovx (degrees), pixel aspect, near, far
VIEWS = [("A", 17.0, -11.0, 23.0, (0.7, -0.4, -1.3), 60.0, 1.0, 0.01, 100.0),
         ("B", -31.0, 8.0, -140.0, (-2.0, 1.5, 0.6), 35.0, 2.0, 0.01, 100.0),
         ("C", 5.0, 29.0, 90.0, (3.0, 0.2, -0.8), 100.0, 0.5, 0.5, 20.0),
         ("D", 12.0, -3.0, 7.0, (0.1, 0.1, 0.1), 60.0, 1.0, 0.01, 100.0)]


def main():
    sys.path.insert(0, REF)
    from utils.graphics_utils import getProjectionMatrix, getWorld2View2  # noqa: E402  (reference code)
    out = {}
    ids, params = [], []
    for name, yaw, pitch, roll, pos, fovx_deg, aspect, znear, zfar in VIEWS:
        a, b, c = math.radians(yaw), math.radians(pitch), math.radians(roll)
        ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
        # world-to-camera rotation Rz(roll) Rx(pitch) Ry(yaw), multiplied out entry by entry
        w2c = np.array([[cc * ca + sc * sb * sa, -sc * cb, -cc * sa + sc * sb * ca],
                        [sc * ca - cc * sb * sa, cc * cb, -sc * sa - cc * sb * ca],
                        [cb * sa, sb, cb * ca]])
        T = -w2c @ np.array(pos)
        R = w2c.T                           # the reference stores the camera-to-world rotation (cameras.py:21-22)
        for W, H in SIZES:
            fovx = math.radians(fovx_deg)
            fovy = 2 * math.atan(math.tan(fovx / 2) * H / W * aspect)
            view = torch.tensor(getWorld2View2(R, T)).transpose(0, 1)
            proj = getProjectionMatrix(znear=znear, zfar=zfar, fovX=fovx, fovY=fovy).transpose(0, 1)
            full = (view.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0)
            k = f"{name}_{W}x{H}"
            ids.append(k)
            params.append([W, H, yaw, pitch, roll, *pos, fovx_deg, aspect, znear, zfar])
            out[k + "_view"], out[k + "_full"] = view.numpy(), full.numpy()
            out[k + "_center"] = view.inverse()[3, :3].numpy()
            out[k + "_tan"] = np.array([math.tan(fovx * 0.5), math.tan(fovy * 0.5)])   # gaussian_renderer/__init__.py:189-190
            out[k + "_R"], out[k + "_T"] = R, T
    out["ids"] = np.array(ids)
    out["params"] = np.array(params, np.float64)
    np.savez_compressed(os.path.join(HERE, "reference_cameras.npz"), **out)
    print("wrote", os.path.join(HERE, "reference_cameras.npz"), len(ids), "cameras")


if __name__ == "__main__":
    main()
