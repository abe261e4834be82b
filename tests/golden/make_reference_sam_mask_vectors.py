"""Generates tests/golden/reference_sam_masks.npz by running the reference's own code on the CPU:
encoders/sam_encoder/segment_anything/modeling/sam.py `Sam.postprocess_masks` (:133-162) and, of utils/amg.py,
`calculate_stability_score`, `batched_mask_to_box`, `is_box_near_crop_edge`, `uncrop_masks` and `mask_to_rle_pytorch`, chained as
automatic_mask_generator.py:300-319 chains them.

utils/amg.py needs numpy and torch alone and is loaded from its file (the package's __init__ imports torchvision, which does not
exist where this runs).  modeling/sam.py imports the networks: `postprocess_masks` is taken from the file's syntax tree and
compiled alone, and called with a stub `self` that carries `image_encoder.img_size`.

Per case: the logits (or, for the smooth cases, the small random grid that tests/sam_masks_oracle.py:expand_logits expands to
them exactly), the sizes, and of the reference
  dense32            the float32 result - whole for the exact cases and those of up to 2^15 pixels; for the larger ones, whose float images would not fit a
                     committed file, `sample_idx` / `sample32` / `sample64`: 4608 pixels (the first and last 256 and 4096 drawn)
  delta              4 x max |float32 result - float64 result of the same chain| (postprocess_masks called on float64 logits)
  certain, nopen     per mask and threshold (t + offset, t - offset, t): the pixels whose float64 value is > threshold + delta,
                     and those within delta of it (the OPEN pixels)
  set64, open        bit-packed (tests/sam_masks_oracle.py:pack) in the full frame: float64 value > t; open at t
  ref_counts, ref_stability, ref_boxes, ref_near_edge, ref_rle_lens / ref_rle_flat   what the reference makes of dense32
The EXACT cases (dyadic scales and weights, integer logits) assert float32 == float64 on every pixel and more than a hundred pixels
exactly on 0 and +-1 (in each of the 64 and 128 outputs; the 32 output prints its number).  Every case asserts that the open pixels are at most 0.1 % and takes the next seed otherwise; `edge_special`
asserts that there is none.

Run it where the reference exists (the tests read only the npz):

    python tests/golden/make_reference_sam_mask_vectors.py
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference/encoders/sam_encoder/segment_anything"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sam_masks_oracle as oracle  # noqa: E402  (expand_logits and pack only: the data layout, not the results)


def load_amg():
    spec = importlib.util.spec_from_file_location("ref_amg", os.path.join(REF, "utils", "amg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_postprocess():
    path = os.path.join(REF, "modeling", "sam.py")
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Sam"][0]
    fn = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "postprocess_masks"]
    assert len(fn) == 1
    from typing import Tuple
    ns = {"torch": torch, "F": F, "Tuple": Tuple}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns["postprocess_masks"]


AMG = load_amg()
POST = load_postprocess()
OUT = {}
T, OFFSET = 0.0, 1.0


def reference_dense(low_res, S, input_size, original_size, dtype):
    stub = types.SimpleNamespace(image_encoder=types.SimpleNamespace(img_size=S))
    x = torch.from_numpy(low_res).to(dtype)[:, None]
    return POST(stub, x, tuple(input_size), tuple(original_size))[:, 0].numpy()


def record(name, low_res, S, input_size, original_size, crop_box=None, frame_size=None, grid=None, exact=False, no_open=False, min_on=0):
    """False (nothing recorded) where the open-pixel cap does not hold"""
    H, W = original_size
    crop = [0, 0, W, H] if crop_box is None else list(crop_box)
    FH, FW = (H, W) if frame_size is None else frame_size
    d32 = reference_dense(low_res, S, input_size, original_size, torch.float32)
    d64 = reference_dense(low_res, S, input_size, original_size, torch.float64)
    assert d32.dtype == np.float32 and d64.dtype == np.float64 and d32.shape == (low_res.shape[0], H, W)
    gap = float(np.abs(d32.astype(np.float64) - d64).max())
    delta = 4 * gap
    if exact:
        assert gap == 0.0, (name, gap)
        on = sum(int((d32 == v).sum()) for v in (0.0, 1.0, -1.0))
        if on <= min_on:
            return False
        print(f"{name}: exact, {on} pixels on 0 and +-1")
    ths = [T + OFFSET, T - OFFSET, T]
    is_open = lambda th: (np.abs(d64 - th) <= delta) & (delta > 0)      # (exact arithmetic leaves nothing open)
    nopen = np.stack([is_open(th).sum((1, 2)) for th in ths], 1).astype(np.int32)
    certain = np.stack([(d64 > th + delta).sum((1, 2)) for th in ths], 1).astype(np.int32)
    if nopen.sum() > 0.001 * d64.size or (no_open and nopen.sum()):
        return False
    pre = name + "/"
    if grid is None:
        OUT[pre + "low_res"] = low_res
    else:
        OUT[pre + "grid"] = grid
        OUT[pre + "h"] = np.int64(low_res.shape[1])
    OUT[pre + "geom"] = np.array([S, *input_size, H, W, FH, FW, *crop], np.int64)
    OUT[pre + "delta"], OUT[pre + "gap"], OUT[pre + "max_logit"] = np.float64(delta), np.float64(gap), np.float64(np.abs(low_res).max())
    OUT[pre + "certain"], OUT[pre + "nopen"] = certain, nopen
    if exact or d32.size <= 1 << 15:
        OUT[pre + "dense32"] = d32
    else:
        rng = np.random.default_rng(7)
        idx = np.unique(np.concatenate([np.arange(256), d32.size - 1 - np.arange(256), rng.integers(0, d32.size, 4096)]))
        OUT[pre + "sample_idx"], OUT[pre + "sample32"], OUT[pre + "sample64"] = idx, d32.reshape(-1)[idx], d64.reshape(-1)[idx]
    OUT[pre + "set64"] = oracle.pack(np.asarray(AMG.uncrop_masks(torch.from_numpy(d64 > T), crop, FH, FW)))
    OUT[pre + "open"] = oracle.pack(np.asarray(AMG.uncrop_masks(torch.from_numpy(is_open(T)), crop, FH, FW)))
    # what the reference makes of its float32 masks (automatic_mask_generator.py:300-319)
    masks = torch.from_numpy(d32)
    with np.errstate(all="ignore"):
        OUT[pre + "ref_stability"] = AMG.calculate_stability_score(masks, T, OFFSET).numpy().astype(np.float32)
    OUT[pre + "ref_counts"] = np.stack([(d32 > np.float32(th)).sum((1, 2)) for th in ths], 1).astype(np.int32)
    binary = masks > T
    boxes = AMG.batched_mask_to_box(binary)
    OUT[pre + "ref_boxes"] = boxes.numpy().astype(np.int32)
    OUT[pre + "ref_near_edge"] = AMG.is_box_near_crop_edge(boxes, crop, [0, 0, FW, FH]).numpy()
    rles = AMG.mask_to_rle_pytorch(AMG.uncrop_masks(binary, crop, FH, FW))
    assert all(r["size"] == [FH, FW] for r in rles)
    OUT[pre + "ref_rle_lens"] = np.array([len(r["counts"]) for r in rles], np.int64)
    OUT[pre + "ref_rle_flat"] = np.array([c for r in rles for c in r["counts"]], np.int32)
    print(f"{name}: gap {gap:.3g} = {gap / 2.0 ** -24 / max(np.abs(low_res).max(), 1e-30):.1f} x 2^-24 max|logit|, delta {delta:.3g}, "
          f"open {int(nopen.sum())} of {d64.size}")
    return True


def seeded(name, seed, make, **kw):
    first = seed
    while not record(name, *make(np.random.default_rng(seed)), **kw):
        seed += 1
        assert seed < first + 40, f"{name}: no seed found"
    print(f"{name}: seed {seed}")


def main():
    def ints(M, h=16):
        return lambda rng: rng.integers(-8, 9, size=(M, h, h)).astype(np.float32)

    # ---- exact ----
    for H in (64, 32, 128):
        seeded(f"exact_{H}", 100 + H, lambda rng: (ints(5)(rng), 64, (64, 64), (H, H)), exact=True, min_on=100 if H >= 64 else 0)

    # ---- general: smooth random logits, the bilinear interpolant of a small random grid ----
    def smooth(h, g, S, input_size, original_size):
        def make(rng):
            grid = (4 * rng.standard_normal(size=(12, g + 1, g + 1))).astype(np.float32)
            make.grid = grid
            return oracle.expand_logits(grid, h), S, input_size, original_size
        return make

    for name, h, g, S, inp, orig in (("general_27x48", 16, 4, 64, (36, 64), (27, 48)), ("general_135x240", 16, 4, 64, (36, 64), (135, 240)),
                                     ("general_121x70", 16, 4, 64, (64, 37), (121, 70)), ("general_270x480", 256, 8, 1024, (576, 1024), (270, 480))):
        seed = 500
        while True:
            mk = smooth(h, g, S, inp, orig)
            args = mk(np.random.default_rng(seed))
            if record(name, *args, grid=mk.grid):
                break
            seed += 1
            assert seed < 540, f"{name}: no seed found"
        print(f"{name}: seed {seed}", flush=True)

    # ---- edges (random logits: integer ones would put pixels of these inexact scales onto the thresholds) ----
    def floats(M, h=16):
        return lambda rng: (4 * rng.standard_normal(size=(M, h, h))).astype(np.float32)

    for H, W in ((1, 1), (1, 40), (40, 1)):
        seeded(f"edge_{H}x{W}", 900 + H + W, lambda rng: (floats(3)(rng), 64, (64, 64), (H, W)))
    seeded("edge_m1", 41, lambda rng: (floats(1)(rng), 64, (64, 64), (20, 24)))
    seeded("edge_m67", 42, lambda rng: (floats(67)(rng), 64, (64, 64), (20, 24)))
    lr = np.full((7, 16, 16), -4.0, np.float32)
    lr[1] = 4.0                                                 # all positive
    lr[2, 0, 0], lr[3, 0, 15], lr[4, 7, 0], lr[5, 7, 15] = 4.0, 4.0, 4.0, 4.0      # one pixel in each corner of the kept part
    lr[6, 9:] = 4.0                                             # positive only where the crop to input_size removes it
    assert record("edge_special", lr, 64, (32, 64), (16, 32), exact=False, no_open=True)
    assert OUT["edge_special/gap"] == 0.0
    assert OUT["edge_special/ref_counts"][0].tolist() == [0, 0, 0] and OUT["edge_special/ref_counts"][6, 2] == 0
    assert np.isnan(OUT["edge_special/ref_stability"][0]) and OUT["edge_special/ref_boxes"][0].tolist() == [0, 0, 0, 0]

    # ---- crops: frame (120, 160), crop (40, 30, 140, 110) ----
    lr = np.full((4, 16, 16), -4.3171, np.float32)
    lr[0, 4:8, 0:3] = 3.7313          # at the crop's left edge, far from the frame's: dropped
    lr[1, 10:13, 6:10] = 3.7313       # at the crop's bottom edge, which is within 20 of the frame's: kept
    lr[2, 4:8, 6:10] = 3.7313         # in the middle: kept
    lr[3, 4:8, 13:16] = 3.7313        # at the crop's right edge, 21 from the frame's: dropped
    assert record("crop", lr, 64, (52, 64), (80, 100), crop_box=(40, 30, 140, 110), frame_size=(120, 160))
    assert OUT["crop/ref_near_edge"].tolist() == [True, False, False, True], OUT["crop/ref_near_edge"]
    assert OUT["crop/ref_boxes"][1, 3] == 79

    path = os.path.join(HERE, "reference_sam_masks.npz")
    np.savez_compressed(path, **OUT)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
