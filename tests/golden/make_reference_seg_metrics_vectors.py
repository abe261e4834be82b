"""Generates tests/golden/reference_seg_metrics.npz by running the reference's own scoring code on the CPU:
encoders/lseg_encoder/segmentation_metric.py `calculate_accuracy`, `calculate_accuracy_mask`, `calculate_iou` and
`calculate_iou_mask` (:58-108), called as the script calls them (:818-821): on (1,H,W) int64 label maps.

The module imports `encoding`, `clip` and lightning at the top, none of which exists where this runs: the four functions are taken
from the file's syntax tree and compiled alone, with `np` as their only global.

Per case the label maps (stored as uint8), the label count L and, per num_classes, the four results.  The cases:

  big        L = 150, 37 x 53, skewed (Dirichlet) label frequencies; student and gt are the teacher with a share of pixels redrawn
  seven      L = 7, scored with num_classes 7 and 3
  few        four labels present, fewer than num_classes = 7; labels 2 and 5 are equally frequent: a tie INSIDE the cut
  same       teacher == student everywhere
  nomatch    gt never equals the teacher: both masked results are NaN
  gtonly     a label that occurs in gt only (it takes part in the masked ranking and has no matching pixel)

`np.argsort(-counts)` in the reference is not a stable sort, so the reference does not define which label wins a tie at the
cut.  For every recorded (case, num_classes) this script therefore ASSERTS that the count at rank num_classes differs from the
count at rank num_classes + 1 under both rankings (teacher + student; gt + teacher + student); a random case whose seed fails
takes the next seed.  Ties inside the cut are harmless.

The pictures (segmentation.py:547-559), cases `color_a` (the maps of `big`) and `color_b` (5 x 7; palette rows 0 and 255; image
values 0, 1 and exact k / 255):
  mask    `utils.get_mask_pallete(predict - 1, 'detail')` lives in the external `encoding` package; its two lines -
          `out_img = Image.fromarray(npimg.astype('uint8')); out_img.putpalette(palette)` - are restated here with a palette of
          this project's own, and PIL's `convert("RGB")` makes the colours
  strip   the reference's statements of segmentation.py:552-559, read from its file through the syntax tree when this runs
          (nothing of them is restated here) and executed in torch on the CPU with the palette image and the loader's image

Run it where the reference exists (the tests read only the npz):

    python tests/golden/make_reference_seg_metrics_vectors.py
"""
import ast
import os
import warnings

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("calculate_accuracy", "calculate_accuracy_mask", "calculate_iou", "calculate_iou_mask")


def load_reference():
    path = os.path.join(REF, "encoders", "lseg_encoder", "segmentation_metric.py")
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in tree.body) == sorted(NAMES)
    ns = {"np": np}
    exec(compile(tree, path, "exec"), ns)
    return [ns[n] for n in NAMES]


STRIP_LINES = (552, 559)      # segmentation.py: the statements between the saved mask and the saved `_vis.png`


def load_strip_chain():
    """The reference's own statements that turn the palette image `mask` and the loader's image `img` into the strip, read from
    its file when this runs: the assignments of the line range are executed as they stand, and of the last statement, which
    saves the picture, the array handed to `Image.fromarray` is evaluated.  Returns f(mask, img) -> (uint8 strip, namespace)."""
    path = os.path.join(REF, "encoders", "lseg_encoder", "segmentation.py")
    tree = ast.parse(open(path).read(), path)
    nodes = sorted((n for n in ast.walk(tree) if isinstance(n, (ast.Assign, ast.Expr)) and STRIP_LINES[0] <= n.lineno <= STRIP_LINES[1]),
                   key=lambda n: n.lineno)
    assigns, last = [n for n in nodes if isinstance(n, ast.Assign)], nodes[-1]
    assert len(assigns) == 7 and isinstance(last, ast.Expr) and last.lineno == STRIP_LINES[1], "the reference's file is not the one expected"
    saved = last.value.func.value          # Image.fromarray(<array>) of `Image.fromarray(<array>).save(...)`
    assert isinstance(saved, ast.Call) and ast.unparse(saved.func) == "Image.fromarray"
    body = compile(ast.Module(body=assigns, type_ignores=[]), path, "exec")
    array = compile(ast.Expression(body=saved.args[0]), path, "eval")

    def run(mask, img):
        ns = {"mask": mask, "img": img, "torch": torch, "np": np}
        exec(body, ns)
        return eval(array, ns), ns

    return run


def tie_at_cut(maps, num_classes):
    counts = np.sort(np.bincount(np.concatenate([m.reshape(-1) for m in maps])))[::-1]
    counts = counts[counts > 0]
    return len(counts) > num_classes and counts[num_classes - 1] == counts[num_classes]


def tie_inside_cut(maps, num_classes):
    counts = np.sort(np.bincount(np.concatenate([m.reshape(-1) for m in maps])))[::-1]
    counts = counts[counts > 0][:num_classes]
    return len(set(counts.tolist())) < len(counts)


def redraw(rng, base, share, p):
    out = base.copy()
    where = rng.random(base.shape) < share
    out[where] = rng.choice(len(p), size=int(where.sum()), p=p)
    return out


def random_case(seed, L, shape, num_classes, alpha, derive=lambda t, s, g: (t, s, g)):
    """The first seed from `seed` on whose maps (after `derive`) have no tie at any of the cuts."""
    while True:
        rng = np.random.default_rng(seed)
        p = rng.dirichlet(np.full(L, alpha))
        teacher = rng.choice(L, size=shape, p=p)
        student = redraw(rng, teacher, 0.3, p)
        gt = redraw(rng, teacher, 0.25, p)
        teacher, student, gt = derive(teacher, student, gt)
        if not any(tie_at_cut(maps, nc) for nc in num_classes for maps in ((teacher, student), (gt, teacher, student))):
            return teacher, student, gt, seed
        seed += 1


def main():
    acc, acc_mask, iou, iou_mask = load_reference()
    out = {}
    inside = []

    def record(name, teacher, student, gt, L, num_classes):
        for m in (teacher, student, gt):
            assert m.min() >= 0 and m.max() < L
        t, s, g = (m.astype(np.int64)[None] for m in (teacher, student, gt))          # (1,H,W) int64, as the script holds them
        out[f"{name}/teacher"], out[f"{name}/student"], out[f"{name}/gt"] = (m.astype(np.uint8) for m in (teacher, student, gt))
        out[f"{name}/L"] = np.int64(L)
        out[f"{name}/num_classes"] = np.array(num_classes, np.int64)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            out[f"{name}/accuracy"] = np.float64(acc(t, s))
            out[f"{name}/accuracy_masked"] = np.float64(acc_mask(g, t, s, 0))
            for nc in num_classes:
                for maps in ((teacher, student), (gt, teacher, student)):
                    assert not tie_at_cut(maps, nc), (name, nc)
                    inside.append(tie_inside_cut(maps, nc))
                out[f"{name}/iou_{nc}"] = np.float64(iou(t, s, nc))
                out[f"{name}/iou_masked_{nc}"] = np.float64(iou_mask(g, t, s, nc))

    t, s, g, seed = random_case(20260, 150, (37, 53), (7,), 0.08)
    print("big: seed", seed)
    record("big", t, s, g, 150, (7,))
    big = (t, s, g)

    t, s, g, seed = random_case(411, 7, (19, 23), (7, 3), 0.9)
    print("seven: seed", seed)
    record("seven", t, s, g, 7, (7, 3))

    # four labels present of 150, in blocks; labels 2 and 5 cover 60 pixels each in the teacher and in the student
    rng = np.random.default_rng(5)
    t = np.zeros((12, 20), np.int64)
    t[:3], t[3:6], t[6:7], t[7:] = 2, 5, 140, 9
    s = t.copy()
    s[6:9, 4:15] = 9
    s[9, :7] = 140
    s[0, :5], s[3, :5] = 5, 2
    g = t.copy()
    g[rng.random(t.shape) < 0.2] = 9
    record("few", t, s, g, 150, (7,))
    assert tie_inside_cut((t, s), 7)

    t, s, g, seed = random_case(77, 20, (16, 17), (7,), 0.5, lambda t, s, g: (t, t.copy(), g))
    print("same: seed", seed)
    record("same", t, s, g, 20, (7,))

    t, s, g, seed = random_case(99, 12, (9, 31), (7,), 0.7, lambda t, s, g: (t, s, (t + 1) % 12))
    print("nomatch: seed", seed)
    record("nomatch", t, s, g, 12, (7,))
    assert np.isnan(out["nomatch/accuracy_masked"]) and np.isnan(out["nomatch/iou_masked_7"])

    # label 30 occurs in gt only, often enough to enter the masked ranking
    def gt_only(t, s, g):
        g = g.copy()
        g[:4] = 30
        return t, s, g

    t, s, g, seed = random_case(1234, 10, (15, 22), (7,), 1.5, gt_only)
    print("gtonly: seed", seed)
    record("gtonly", t, s, g, 31, (7,))
    assert any(inside), "no case has a tie inside the cut"

    # ---- pictures ----
    from PIL import Image
    rng = np.random.default_rng(31337)

    strip_of = load_strip_chain()

    def pictures(name, labels, palette, image):
        """labels (H,W) < len(palette); palette (L,3) uint8; image (3,H,W) float32 in [-1, 1] as the reference's loader gives it"""
        mask = Image.fromarray(labels.astype('uint8'))
        mask.putpalette(palette.reshape(-1).tolist())
        strip, ns = strip_of(mask, torch.from_numpy(image))
        out[f"{name}/strip"] = strip
        out[f"{name}/image"] = ns["vis1"].permute(2, 0, 1).contiguous().numpy()      # (3,H,W): the image in [0, 1] of the strip's first part
        out[f"{name}/mask"] = np.array(mask.convert("RGB"))
        out[f"{name}/labels"], out[f"{name}/palette"] = labels.astype(np.uint8), palette

    palette = rng.integers(0, 256, size=(150, 3)).astype(np.uint8)
    pictures("color_a", big[1], palette, rng.uniform(-1, 1, size=(3, 37, 53)).astype(np.float32))
    palette = rng.integers(0, 256, size=(256, 3)).astype(np.uint8)
    palette[0], palette[255], palette[7] = (0, 0, 0), (255, 255, 255), (255, 0, 128)
    labels = rng.integers(0, 256, size=(5, 7))
    labels.reshape(-1)[:4] = (0, 255, 7, 255)
    image = rng.uniform(-1, 1, size=(3, 5, 7)).astype(np.float32)
    image[0].reshape(-1)[:6] = (-1.0, 1.0, 1.0, -1.0, 0.0, 0.5)
    image[1] = (2.0 * rng.integers(0, 256, size=(5, 7)).astype(np.float32) / 255.0 - 1.0).astype(np.float32)
    pictures("color_b", labels, palette, image)

    path = os.path.join(HERE, "reference_seg_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for k in sorted(out):
        if out[k].size == 1:
            print(k, out[k])


if __name__ == "__main__":
    main()
