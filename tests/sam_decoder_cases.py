"""The fixture recipe of the SAM decoder tests, shared by the golden generator (tests/golden/make_reference_sam_decoder_vectors.py),
the oracle's CPU tests and the GPU tests.  The full weight set is 16 MB and is not committed: it is a pure function of a seed.

Weights.  rng = numpy.random.default_rng(seed); the tensors are drawn in the order of sam_decoder.parameter_table() (the order
of include/f3dgs.h), each as rng.standard_normal(shape) in float64, scaled, then rounded to float32:
    matrices (Linear (out, in), ConvTranspose2d (in, out, 2, 2))         n / sqrt(fan_in), fan_in = in
    LayerNorm weights (norm*, output_upscaling.1)                        1 + 0.1 n
    biases                                                               0.1 n
    embeddings (*_embed*, point_embeddings, iou_token, mask_tokens) and the Gaussian matrix     n
    every q_proj and k_proj weight                                       further x QK_SCALE = 0.25 (x 1 in the sharp case)
Unscaled q / k give near-one-hot softmaxes whose flips make the reference's own fp32 differ from its fp64 by up to 0.07 on logits
of size 4; at 0.25 the gap is 2e-5 .. 2e-4 and the prompts still give clearly different masks.

Features.  numpy.random.default_rng([seed, h, w]).standard_normal((256, h, w)) x feature_scale (0.5; 32 in the sharp case), float32.

Prompts.  numpy.random.default_rng([seed, 77, case index]): coordinates uniform in the input image, then the boxes, float32.
"""
import numpy as np

QK_SCALE = 0.25
SEED = 1


class Case:
    def __init__(self, name, grid, B, labels=None, box=False, multimask=True, input_size=None, sharp=False, sampled=False):
        self.name, self.grid, self.B, self.labels, self.box, self.multimask = name, grid, B, labels, box, multimask
        self.input_size = input_size if input_size is not None else (16 * grid[0], 16 * grid[1])
        self.sharp, self.sampled = sharp, sampled
        self.n_points = 0 if labels is None else len(labels)
        self.tokens = 5 + self.n_points + (2 if box else 1)
        self.n_masks = 3 if multimask else 1
        self.qk_scale = 1.0 if sharp else QK_SCALE
        self.feature_scale = 32.0 if sharp else 0.5


# every kernel path: less than one 32-row tile, a tile plus a remainder (non-square grid and input), many tiles; one point plus
# the pad with either label, all three labels, a box alone (7 tokens, no pad), a box plus 9 points (16 tokens, the limit); B = 1,
# 2, 3; both mask selections; the sharp case (full-scale q / k on features x 64: scores beyond 88)
CASES = [
    Case("g1x1", (1, 1), 1, labels=[1]),
    Case("g4x4_fg", (4, 4), 1, labels=[1]),
    Case("g4x4_bg_single", (4, 4), 3, labels=[0], multimask=False),
    Case("g8x5_three_labels", (8, 5), 3, labels=[1, 0, -1], input_size=(128, 80)),
    Case("g8x5_box", (8, 5), 1, box=True, multimask=False, input_size=(128, 80)),
    Case("g8x5_box_9pts", (8, 5), 3, labels=[1, 0, 1, 1, 0, -1, 1, 0, 1], box=True, input_size=(128, 80)),
    Case("g64x64", (64, 64), 2, labels=[1], input_size=(1024, 1024), sampled=True),
    Case("sharp", (8, 5), 2, labels=[1, 0], input_size=(128, 80), sharp=True),
]
BY_NAME = {c.name: c for c in CASES}


def _kind(name, shape):
    if "gaussian_matrix" in name or "_embed" in name or "point_embeddings" in name or "iou_token" in name or "mask_tokens" in name:
        return "embedding"
    if name.endswith(".bias"):
        return "bias"
    return "matrix" if len(shape) >= 2 else "norm"


def make_weights(seed=SEED, qk_scale=QK_SCALE, table=None):
    """{name: float32 array} of every parameter, in the table's order."""
    if table is None:
        from sam_decoder import parameter_table
        table = parameter_table()
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in table:
        n = rng.standard_normal(shape)
        kind = _kind(name, shape)
        if kind == "matrix":
            n = n / np.sqrt(shape[1] if len(shape) == 2 else shape[0])
            if ".q_proj." in name or ".k_proj." in name:
                n = n * qk_scale
        elif kind == "norm":
            n = 1 + 0.1 * n
        elif kind == "bias":
            n = 0.1 * n
        out[name] = n.astype(np.float32)
    return out


def make_features(case, seed=SEED):
    h, w = case.grid
    return (case.feature_scale * np.random.default_rng([seed, h, w]).standard_normal((256, h, w))).astype(np.float32)


def make_prompts(case, seed=SEED):
    """(coords (B, n, 2) float32 or None, labels (B, n) int32 or None, boxes (B, 4) float32 or None); prompt b's labels are the
    case's rolled by b, so that the prompts of a batch differ in more than their coordinates."""
    rng = np.random.default_rng([seed, 77, [c.name for c in CASES].index(case.name)])
    ih, iw = case.input_size
    coords = labels = boxes = None
    if case.n_points:
        coords = (rng.uniform(0, 1, (case.B, case.n_points, 2)) * np.array([iw, ih])).astype(np.float32)
        labels = np.stack([np.roll(np.array(case.labels, np.int32), b) for b in range(case.B)])
    if case.box:
        a, b = rng.uniform(0, 0.5, (case.B, 2)), rng.uniform(0.5, 1, (case.B, 2))
        boxes = (np.concatenate([a, b], 1) * np.array([iw, ih, iw, ih])).astype(np.float32)
    return coords, labels, boxes


def sample_index(size):
    """the 64 x 64 case records a fixed sample instead of its whole output: the first and last 256 logits and 8192 drawn"""
    rng = np.random.default_rng(7)
    return np.unique(np.concatenate([np.arange(256), size - 1 - np.arange(256), rng.integers(0, size, 8192)]))
