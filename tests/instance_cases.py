"""The end-to-end inputs of the instance association tests, built with the judges alone (no GPU): three general-camera views
of one scene of tests/test_gpu_contrib.py, the Gaussians cut into five slabs along x, every view's instance map the slab of the
pixel's dominant Gaussian (the float64 walk of tests/contrib_oracle.py over the CPU oracle's forward state) under a fixed
per-view permutation of the ids.  tests/test_instance_assoc_cpu.py checks on the CPU oracle that the choice is a sound one;
tests/test_gpu_instance_assoc.py runs exactly these inputs through InstanceLifter."""
import math

import numpy as np

import contrib_oracle as co
import label_maps as lm
from util import general_camera

SCENE = "tiles"        # 400 Gaussians, 129 x 64: by the judge every matched IoU is above 0.89 ("chunks": 0.51, too near the threshold)
SLABS = 5
MAX_MASKS = 8          # three mask ids no view uses: empty masks take part
MAX_INSTANCES = 8
IOU_THRESH = 0.5
VIEWS = [dict(yaw=0.0, pitch=0.0, roll=0.0, campos=(0.0, 0.0, 0.0)), dict(yaw=6.0, pitch=-3.0, roll=10.0, campos=(0.3, -0.2, -0.5)),
         dict(yaw=-8.0, pitch=4.0, roll=-5.0, campos=(-0.4, 0.1, 0.4))]
PERMS = [(2, 0, 4, 1, 3), (4, 3, 2, 1, 0), (1, 4, 0, 3, 2)]      # view v shows slab s as mask PERMS[v][s]
_cache = {}


def slabs_of(means3D):
    """(P,) the slab of every Gaussian: equal counts along x"""
    x = np.asarray(means3D)[:, 0].astype(np.float64)
    edges = np.quantile(x, np.linspace(0, 1, SLABS + 1)[1:-1])
    return np.searchsorted(edges, x, side="right").astype(np.int64)


def cameras(W, H):
    """the three views' camera entries, tanfov as render() forms it from the FoV (2 atan, then tan of the half)"""
    out = []
    for v in VIEWS:
        cam = general_camera(W, H, **v)
        for k in ("R", "t", "fovx", "fovy"):
            cam.pop(k)
        out.append(cam)
    return out


def oracle_tan(cam):
    return math.tan(2 * math.atan(cam["tanfovx"]) * 0.5), math.tan(2 * math.atan(cam["tanfovy"]) * 0.5)


def build():
    """-> dict(scene, W, H, P, slab (P), cams, maps: the views' permuted instance maps (H, W) int64, -1 where nothing blended,
    plain: the same maps in slab ids, votes: the judge's float64 (P, MAX_MASKS + 1) sums of every view's permuted map)"""
    if _cache:
        return _cache
    from oracle.oracle import Oracle, scene_kwargs
    from test_gpu_contrib import CASES
    sc = CASES[SCENE]()
    W, H, P = sc["image_width"], sc["image_height"], sc["P"]
    slab = slabs_of(sc["means3D"].numpy())
    cams, maps, plain, votes = cameras(W, H), [], [], []
    for cam, perm in zip(cams, PERMS):
        so = dict(sc, **cam)
        so["tanfovx"], so["tanfovy"] = oracle_tan(cam)
        o = Oracle()
        o.forward(**scene_kwargs(so))
        state = co.oracle_state(o)
        ids = co.walk(state, W, H)["ids"]
        p = np.where(ids >= 0, slab[np.maximum(ids, 0)], -1)
        m = np.where(p >= 0, np.asarray(perm, np.int64)[np.maximum(p, 0)], -1)
        plain.append(p)
        maps.append(m)
        votes.append(co.walk(state, W, H, lm.one_hot(m, MAX_MASKS))["acc"])
    _cache.update(scene=sc, W=W, H=H, P=P, slab=slab, cams=cams, maps=maps, plain=plain, votes=votes)
    return _cache
