"""Generates tests/golden/reference_small_regions.npz by running the reference's own code on the CPU:
encoders/sam_encoder/segment_anything/utils/amg.py `remove_small_regions` and `batched_mask_to_box`, chained as
automatic_mask_generator.py:325-373 `postprocess_small_regions` chains them (holes, then islands on the result), and for the
pipeline case that function itself, taken from its file's syntax tree.

utils/amg.py is loaded from its file (make_reference_sam_mask_vectors.py says why).  remove_small_regions imports cv2, which does
not exist where this runs: a stand-in module is put into sys.modules["cv2"] whose connectedComponentsWithStats(img, 8) is
scipy.ndimage.label with a 3 x 3 structure of ones, plus np.bincount for the areas.  The reference function runs unmodified on it.
Labels therefore come in scipy's order - by a component's first pixel in row-major order - and np.argmax(sizes) resolves a tie for
the largest component to the first of them.  That is this project's rule and is NOT measured against OpenCV: every call asserts
that no tie decided anything, except in the case `tie_rule`, which exists to pin the rule.
batched_nms (torchvision, not installed) is tests/sam_masks_oracle.py:nms, the documented stand-in.

Per case `name`: `name/frame` (FH, FW), `name/input` the masks bit-packed (tests/sam_masks_oracle.py:pack), `name/thresholds`, and
per threshold j `name/j/holes`, `name/j/islands` (packed: the masks after holes, and after islands on that), `name/j/changed`
(K,2) bool, `name/j/area` (K,) int32, `name/j/box` (K,4) int32 of the final masks; `name/index` where the case selects rows.
`pipeline/...`: the settings, the further logits and the expected records of MaskPostprocessor on the `exact_64` logits of
reference_sam_masks.npz and a second batch (pipeline() says why).

Run it where the reference and scipy exist (the tests read only the npz):

    python tests/golden/make_reference_small_region_vectors.py
"""
import ast
import importlib.util
import json
import os
import sys
import types

import numpy as np
import scipy.ndimage
import torch

REF = "/root/reference/encoders/sam_encoder/segment_anything"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sam_masks_oracle as oracle  # noqa: E402  (pack / unpack, the run lengths and the stand-in NMS)

TIES = {"allowed": False, "seen": 0}


def connected_components_with_stats(img, connectivity):
    assert connectivity == 8
    labels, n = scipy.ndimage.label(img, structure=np.ones((3, 3), int))
    sizes = np.bincount(labels.reshape(-1), minlength=n + 1)
    if n and (img != 0).any():
        fg = sizes[1:]
        TIES["last"] = int((fg == fg.max()).sum()) > 1
    stats = np.zeros((n + 1, 5), np.int32)
    stats[:, -1] = sizes
    return n + 1, labels.astype(np.int32), stats, None


sys.modules["cv2"] = types.SimpleNamespace(connectedComponentsWithStats=connected_components_with_stats)


def load_amg():
    spec = importlib.util.spec_from_file_location("ref_amg", os.path.join(REF, "utils", "amg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


AMG = load_amg()
OUT = {}


def remove(mask, t, mode):
    """the reference's remove_small_regions; a tie for the largest that DECIDES (islands, every one small) is counted"""
    TIES["last"] = False
    out, changed = AMG.remove_small_regions(mask, t, mode)
    if mode == "islands" and changed and TIES["last"]:
        n, _, stats, _ = connected_components_with_stats(mask.astype(np.uint8), 8)
        if (stats[1:, -1] < t).all():
            TIES["seen"] += 1
            assert TIES["allowed"], "a tie for the largest component decides a case other than tie_rule"
    return np.asarray(out, bool), bool(changed)


def draw(rng, shape, density, thresholds):
    """a random mask in which no tie for the largest component decides anything at these thresholds (the next draw otherwise)"""
    for _ in range(200):
        m = rng.random(shape) < density
        seen, allowed = TIES["seen"], TIES["allowed"]
        TIES["allowed"] = True
        for t in thresholds:
            remove(remove(m, t, "holes")[0], t, "islands")
        tied = TIES["seen"] > seen
        TIES["seen"], TIES["allowed"] = seen, allowed
        if not tied:
            return m
    raise AssertionError(f"no tie-free mask of {shape} at density {density}")


def record(name, masks, thresholds, index=None):
    masks = np.asarray(masks, bool)
    FH, FW = masks.shape[1:]
    OUT[f"{name}/frame"] = np.array([FH, FW], np.int64)
    OUT[f"{name}/input"] = oracle.pack(masks)
    OUT[f"{name}/thresholds"] = np.asarray(thresholds, np.float64)
    if index is not None:
        OUT[f"{name}/index"] = np.asarray(index, np.int64)
        masks = masks[index]
    summary = []
    for j, t in enumerate(thresholds):
        t = float(t) if float(t) != int(t) else int(t)
        holes, final, changed = [], [], []
        for m in masks:
            h, ch = remove(m, t, "holes")
            f, ci = remove(h, t, "islands")
            holes.append(h)
            final.append(f)
            changed.append((ch, ci))
        holes, final = np.array(holes).reshape(masks.shape), np.array(final).reshape(masks.shape)
        OUT[f"{name}/{j}/holes"], OUT[f"{name}/{j}/islands"] = oracle.pack(holes), oracle.pack(final)
        OUT[f"{name}/{j}/changed"] = np.array(changed, bool).reshape(-1, 2)
        OUT[f"{name}/{j}/area"] = final.sum((1, 2)).astype(np.int32)
        OUT[f"{name}/{j}/box"] = AMG.batched_mask_to_box(torch.from_numpy(final)).numpy().astype(np.int32)
        summary.append(f"t={t}: {int(np.array(changed)[:, 0].sum())}h {int(np.array(changed)[:, 1].sum())}i of {len(masks)}")
    print(f"{name} {FH}x{FW}: " + "; ".join(summary))
    return OUT


def ring(m, y0, x0, y1, x1):
    m[y0:y1, x0:x1] = True
    m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = False


def depth_masks(N=96):
    out = []
    m = np.zeros((N, N), bool)                                   # a comb: every second column, joined along the bottom row
    m[:, ::2] = True
    m[-1, :] = True
    out.append(m)
    m = np.zeros((N, N), bool)                                   # a serpentine: one component, a chain of thousands of runs
    m[::2, :] = True
    m[1::4, -1] = True
    m[3::4, 0] = True
    out.append(m)
    out.append(m.T.copy())                                       # the same along the columns: long runs, a deep chain
    m = np.zeros((N, N), bool)                                   # a spiral, its arms one blank pixel apart
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True
    free = lambda yy, xx: 0 <= yy < N and 0 <= xx < N and not m[yy, xx]
    ahead = lambda: free(y + dy, x + dx) and (not (0 <= y + 2 * dy < N and 0 <= x + 2 * dx < N) or not m[y + 2 * dy, x + 2 * dx])
    for _ in range(N * N):
        if not ahead():
            dy, dx = dx, -dy
            if not ahead():
                break
        y, x = y + dy, x + dx
        m[y, x] = True
    out.append(m)
    m = np.zeros((N, N), bool)                                   # a U on its side: the arms meet only in the last column
    m[10:14, :] = True
    m[60:64, :] = True
    m[10:64, -1] = True
    out.append(m)
    out.append((np.add.outer(np.arange(N), np.arange(N)) % 2).astype(bool))      # checkerboard: one component of each polarity
    m = np.zeros((N, N), bool)                                   # nested rings: hole in island in hole in island
    for d in (4, 12, 20, 28, 36):
        ring(m, d, d, N - d, N - d)
    m[44:52, 44:52] = True
    out.append(m)
    m = np.zeros((N, N), bool)                                   # thick nested rings with small cores: areas that differ widely
    m[2:94, 2:94] = True
    m[8:88, 8:88] = False
    m[20:76, 20:76] = True
    m[40:56, 40:56] = False
    m[46:49, 46:49] = True
    out.append(m)
    return np.array(out)


def medium_masks(K=8, FH=270, FW=480):
    rng = np.random.default_rng(2024)
    out = []
    for k in range(K):
        g = rng.standard_normal((FH // 15 + 2, FW // 15 + 2))
        smooth = scipy.ndimage.zoom(g, 15, order=3)[:FH, :FW]
        m = smooth > 0.3
        m ^= rng.random((FH, FW)) < 0.02                         # salt and pepper
        out.append(m)
    return np.array(out)


def load_method(path, cls_name, fn_name, ns):
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name][0]
    fn = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == fn_name]
    assert len(fn) == 1
    fn[0].decorator_list = []
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    return ns[fn_name]


def pipeline():
    """MaskPostprocessor's records on two batches in one crop (the whole 64 x 64 frame): the `exact_64` logits of
    reference_sam_masks.npz, then four masks of integer logits made here (the same dyadic geometry: float32 == float64, asserted).
    With the exact_64 logits alone the case the tests need cannot arise - every one of those masks has the whole frame for its box,
    so the first NMS leaves a single mask - hence the second batch: A, a block with a far speck (its box shrinks onto B's when the
    speck goes); B, nearly the same block, nothing small; C, a block with a pinhole (changed by `holes`, kept); D, a block of its
    own, nothing small.  The first stage is chained from the reference's own postprocess_masks, stability score, boxes and the
    stand-in NMS as automatic_mask_generator.py:_process_batch / _process_crop chain them; then the reference's own
    postprocess_small_regions runs on the MaskData.  min_mask_region_area is the first value at which at least one mask is changed
    and kept, one is unchanged, and the second NMS removes one."""
    sys.path.insert(0, HERE)
    import make_reference_sam_mask_vectors as first_stage
    z = np.load(os.path.join(HERE, "reference_sam_masks.npz"))
    extra = np.full((4, 16, 16), -8.0, np.float32)
    extra[0, 2:7, 2:7] = 8.0                                     # A
    extra[0, 13, 13] = 8.0
    extra[1, 2:7, 2:8] = 8.0                                     # B
    extra[2, 9:15, 2:8] = 8.0                                    # C
    extra[2, 11, 4] = -8.0
    extra[3, 9:14, 10:15] = 8.0                                  # D
    low_res = np.concatenate([z["exact_64/low_res"], extra])
    M = low_res.shape[0]
    v = first_stage.reference_dense(low_res, 64, (64, 64), (64, 64), torch.float32)
    assert np.array_equal(v.astype(np.float64), first_stage.reference_dense(low_res, 64, (64, 64), (64, 64), torch.float64))
    assert np.array_equal(v[:5], z["exact_64/dense32"])
    dense = torch.from_numpy(v)
    stab = AMG.calculate_stability_score(dense, 0.0, 1.0)
    masks = dense > 0.0
    boxes = AMG.batched_mask_to_box(masks)
    iou = torch.from_numpy(np.linspace(0.99, 0.90, M).astype(np.float32))
    points = torch.from_numpy(np.stack([np.arange(M) * 2.0 + 0.5, np.arange(M) * 3.0 + 1.0], 1))
    thr = 0.7

    def batched_nms(boxes, scores, idxs, iou_threshold):
        return torch.as_tensor(oracle.nms(boxes.numpy(), scores.numpy(), iou_threshold, idxs.numpy()), dtype=torch.int64)

    ns = {"torch": torch, "np": np, "MaskData": AMG.MaskData, "rle_to_mask": AMG.rle_to_mask, "remove_small_regions": AMG.remove_small_regions,
          "batched_mask_to_box": AMG.batched_mask_to_box, "batched_nms": batched_nms, "mask_to_rle_pytorch": AMG.mask_to_rle_pytorch}
    post = load_method(os.path.join(REF, "automatic_mask_generator.py"), "SamAutomaticMaskGenerator", "postprocess_small_regions", ns)
    assert not AMG.is_box_near_crop_edge(boxes, [0, 0, 64, 64], [0, 0, 64, 64]).any()
    first = AMG.MaskData(rles=AMG.mask_to_rle_pytorch(masks), boxes=boxes, iou_preds=iou, points=points, stability_score=stab,
                         crop_boxes=torch.tensor([[0, 0, 64, 64]] * M))
    first.filter(batched_nms(first["boxes"].float(), first["iou_preds"], torch.zeros_like(first["boxes"][:, 0]), thr))
    n_in = len(first["rles"])
    for min_area in (4, 8, 16, 24, 32, 48, 64, 100):
        data = AMG.MaskData(**{k: (list(x) if isinstance(x, list) else x.clone()) for k, x in first.items()})
        old = [r["counts"] for r in data["rles"]]
        data = post(data, min_area, thr)
        n_changed = sum(r["counts"] not in old for r in data["rles"])
        print(f"pipeline: min_area {min_area}: {n_in} in, {len(data['rles'])} out, {n_changed} changed")
        if not (n_changed >= 1 and len(data["rles"]) - n_changed >= 1 and len(data["rles"]) < n_in):
            continue
        records = []
        for i in range(len(data["rles"])):
            records.append({"segmentation": {"size": [int(x) for x in data["rles"][i]["size"]], "counts": [int(x) for x in data["rles"][i]["counts"]]},
                            "area": int(AMG.area_from_rle(data["rles"][i])), "bbox": AMG.box_xyxy_to_xywh(data["boxes"][i]).tolist(),
                            "predicted_iou": data["iou_preds"][i].item(), "point_coords": [data["points"][i].tolist()],
                            "stability_score": data["stability_score"][i].item(),
                            "crop_box": AMG.box_xyxy_to_xywh(data["crop_boxes"][i]).tolist()})
        print("pipeline: records of points", [r["point_coords"][0][0] for r in records])
        OUT["pipeline/extra_low_res"], OUT["pipeline/iou"], OUT["pipeline/points"] = extra, iou.numpy(), points.numpy()
        OUT["pipeline/settings"] = np.array([thr, float(min_area)], np.float64)      # both NMS thresholds, min_mask_region_area
        OUT["pipeline/records"] = np.frombuffer(json.dumps(records).encode(), np.uint8)
        return
    raise AssertionError("pipeline: no setting changes one mask, leaves one and lets the second NMS remove one")


def main():
    rng = np.random.default_rng(11)
    # 1. frame edges
    for FH, FW in ((1, 1), (1, 40), (40, 1), (32, 7), (33, 5), (64, 3), (37, 45), (70, 9)):
        ts = [1, 2, 7.5, FH * FW + 1]
        record(f"edges_{FH}x{FW}", np.array([draw(rng, (FH, FW), d, ts) for d in (0.1, 0.5, 0.9) for _ in range(2)]), ts)
    # 2. word and column boundaries (a 10 x 10 block keeps "every island small" out of it)
    m = np.zeros((4, 100, 6), bool)
    m[:, 50:60, 0:4] = True
    m[0, 31, 1] = m[0, 32, 2] = True                             # touch at a corner across the words: one component of 2
    m[1, 31, 1] = m[1, 33, 2] = True                             # a row further apart: two components of 1
    m[2, 20:85, 5] = True                                        # one run over three words
    m[3, 31, 2] = m[3, 32, 1] = True                             # the other diagonal
    m[3, 63, 4] = m[3, 64, 5] = True
    record("boundaries", m, [1, 2, 3, 66])
    # 3. connectivity depth
    record("depth", depth_masks(), [1, 10, 100, 5000])
    # 4. threshold edges, both polarities: islands and holes of 7 and 8 pixels beside a large block
    m = np.zeros((1, 40, 40), bool)
    m[0, 4:30, 4:30] = True
    m[0, 8:10, 8:12] = False                                     # a hole of 8
    m[0, 20, 8:15] = False                                       # a hole of 7
    m[0, 34:36, 4:8] = True                                      # an island of 8
    m[0, 34, 20:27] = True                                       # an island of 7
    record("threshold_edges", m, [7, 7.5, 8, 9])
    # 5. quirks
    FH, FW = 20, 24
    q = np.zeros((10, FH, FW), bool)
    q[1] = True                                                  # 0 empty, 1 full
    q[2, 5:7, 5:8] = True                                        # one small island: the same bits, changed
    q[3, 1, 1] = True                                            # every island small, distinct sizes: the largest stays
    q[3, 5, 5:7] = True
    q[3, 10:12, 10:13] = True
    q[3, 15, 1:4] = True
    q[4] = True                                                  # a small outer background: filled
    q[4, 0, :5] = False
    q[5, 2:18, 2:20] = True                                      # only holes
    q[5, 8, 8] = False
    q[6, 2:18, 2:20] = True                                      # only islands
    q[6, 19, 23] = True
    q[7] = q[6]                                                  # both
    q[7, 8, 8] = False
    q[8, 2:18, 2:20] = True                                      # neither
    q[9] = True                                                  # a 1-pixel corner hole in a full mask
    q[9, 0, 0] = False
    record("quirks", q, [1, 2, 10, 30])
    # 6. selection
    M = 70
    masks = np.array([draw(rng, (33, 20), rng.choice([0.2, 0.5, 0.8]), [3, 6]) for _ in range(M)])
    index = np.concatenate([rng.permutation(M)[:40], [3, 3, 69, 0, 69]])
    record("selection", masks, [3, 6], index=index)
    # 7. medium
    record("medium", medium_masks(), [100])
    n_before = TIES["seen"]
    assert n_before == 0
    # 8. the tie rule (this project's; see the module text): the first in row-major order stays, although the other comes first by column
    TIES["allowed"] = True
    t = np.zeros((3, 16, 20), bool)
    t[0, 2:4, 15:17] = True                                      # first in row-major order
    t[0, 8:10, 3:5] = True                                       # first in column-major order
    t[1, 9, 2:5] = True                                          # an L whose first row-major pixel is not in its first column
    t[1, 7:9, 4] = True
    t[1, 7, 5] = True                                            # 6 pixels, first pixel (7, 4)
    t[1, 8, 10:16] = True                                        # 6 pixels, first pixel (8, 10): later
    t[2, 5, 5] = t[2, 5, 7] = t[2, 4, 9] = True                  # three single pixels: (4, 9) first
    record("tie_rule", t, [50])
    assert TIES["seen"] == 3, TIES
    TIES["allowed"] = False
    # 9. the pipeline
    pipeline()
    assert TIES["seen"] == 3

    path = os.path.join(HERE, "reference_small_regions.npz")
    np.savez_compressed(path, **OUT)
    ref = os.path.getsize(os.path.join(HERE, "reference_sam_masks.npz"))
    print(f"wrote {path} ({os.path.getsize(path)} bytes; reference_sam_masks.npz has {ref})")
    assert os.path.getsize(path) < ref // 2


if __name__ == "__main__":
    main()
