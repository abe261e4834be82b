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

Prompts.  numpy.random.default_rng([seed, 77, case index]): coordinates uniform in the input image, then the boxes, float32.  The
index is the case's place in CASES; the edge cases (EDGE_CASES) continue after it from N_CASES.
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

# the edges of the two partitions of the hw image tokens (csrc/sam_decoder.hip): 32-token tiles (rows past hw are zeros in LDS, masked
# in the token -> image softmax, guarded at the stores) and 256-token chunks of the token -> image attention (one running max / sum /
# accumulator each, joined by the combine kernel).  Each case is the smallest grid that reaches its edge:
#   e4x8          32: exactly one full tile, no masked row            e3x11      33: a tile plus one row
#   e15x17       255: a chunk less one, the last tile has 31 rows     e16x16    256: exactly one chunk; B T = 32, one full row tile of the linear
#   e1x257, e257x1    a second chunk of ONE token, h = 1 / w = 1 (4-float logit rows)
#   e16x17       272: the second chunk is half a tile (thread-half 1 fully masked there)
#   e18x16       288: the second chunk is one full tile, then the early break out of the tile loop
#   e17x31       527: three chunks, 15 tokens in the last             e16x17_sharp   scores beyond 88 across two chunks
#   e128x128   16384: the grid limit, 64 chunks
# They live in their own golden file (reference_sam_decoder_edges.npz), every one as a sample (edge_sample_index).
N_CASES = 8                       # len(CASES), frozen: the edge cases' prompt streams continue after it whatever either list becomes
EDGE_CASES = [
    Case("e4x8", (4, 8), 2, labels=[1], sampled=True),
    Case("e3x11", (3, 11), 1, box=True, multimask=False, sampled=True),
    Case("e15x17", (15, 17), 2, labels=[1, 0], sampled=True),
    Case("e16x16", (16, 16), 2, labels=[1, 0, 1, 1, 0, -1, 1, 0, 1], box=True, sampled=True),
    Case("e1x257", (1, 257), 2, labels=[0], multimask=False, sampled=True),
    Case("e257x1", (257, 1), 1, labels=[1], sampled=True),
    Case("e16x17", (16, 17), 3, labels=[1, 0, -1], sampled=True),
    Case("e18x16", (18, 16), 1, box=True, sampled=True),
    Case("e17x31", (17, 31), 2, labels=[1, 0], sampled=True),
    Case("e16x17_sharp", (16, 17), 2, labels=[1, 0], sharp=True, sampled=True),
    Case("e128x128", (128, 128), 1, labels=[1], sampled=True),
]
EDGE_BY_NAME = {c.name: c for c in EDGE_CASES}
_PROMPT_STREAM = {c.name: i for i, c in enumerate(CASES)}
_PROMPT_STREAM.update({c.name: N_CASES + i for i, c in enumerate(EDGE_CASES)})


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
    rng = np.random.default_rng([seed, 77, _PROMPT_STREAM[case.name]])
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


def edge_sample_index(size):
    """every edge case records a sample: all of an output of up to 4096 logits, otherwise the first and last 256 and 1024 drawn"""
    if size <= 4096:
        return np.arange(size)
    rng = np.random.default_rng(11)
    return np.unique(np.concatenate([np.arange(256), size - 1 - np.arange(256), rng.integers(0, size, 1024)]))
