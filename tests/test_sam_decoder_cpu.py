"""CPU checks of the SAM decoder's test apparatus and of sam_decoder.py's surface (no GPU): the independent oracle
(tests/sam_decoder_oracle.py) against the reference's recorded float64 results (tests/golden/reference_sam_decoder.npz and, for
the tile / chunk / grid-limit edge cases, reference_sam_decoder_edges.npz), its prompt encoding against the reference's recorded
sparse embeddings, that the edge list reaches the edges it names, and the errors the Python layer raises before any device work."""
import os

import numpy as np
import pytest
import torch

import sam_decoder_cases as cases
import sam_decoder_oracle as oracle
from util import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_sam_decoder.npz")
EDGES = os.path.join(ROOT, "tests", "golden", "reference_sam_decoder_edges.npz")
NAMES = [c.name for c in cases.CASES]
EDGE_NAMES = [c.name for c in cases.EDGE_CASES]
ALL = {**cases.BY_NAME, **cases.EDGE_BY_NAME}
_Z, _W = {}, {}


def golden():
    """both golden files under one dict (the case names are disjoint)"""
    if not _Z:
        _Z.update(np.load(GOLDEN))
        _Z.update(np.load(EDGES))
    return _Z


def weights_of(name):
    """the case's weights by its recorded seed (made once per (seed, scale), left unchanged)"""
    c = ALL[name]
    key = (int(golden()[f"{name}/params"][8]), c.qk_scale)
    if key not in _W:
        _W[key] = cases.make_weights(*key)
    return _W[key]


def prompts_of(name):
    z = golden()
    return tuple(z[f"{name}/{k}"] if f"{name}/{k}" in z else None for k in ("coords", "labels", "boxes"))


def sd():
    import sam_decoder
    return sam_decoder


def test_golden_file_matches_the_recipe():
    z = golden()
    for c in cases.CASES:
        h, w, B, n, box, multi, ih, iw, seed, sharp = z[f"{c.name}/params"].tolist()
        assert ((h, w), B, n, bool(box), bool(multi), (ih, iw), bool(sharp)) == (c.grid, c.B, c.n_points, c.box, c.multimask, c.input_size, c.sharp)
        coords, labels, boxes = cases.make_prompts(c, seed)
        for got, want in zip(prompts_of(c.name), (coords, labels, boxes)):
            assert (got is None) == (want is None) and (got is None or np.array_equal(got, want))
        assert z[f"{c.name}/sparse"].shape == (c.B, c.tokens - 5, 256)
        assert float(z[f"{c.name}/delta"]) == 4 * float(z[f"{c.name}/gap"]) > 0
        if not c.sharp:
            size = c.B * c.n_masks * 16 * h * w
            assert int(z[f"{c.name}/nopen"]) <= 0.001 * size
    assert max(c.tokens for c in cases.CASES) == 16 and min(c.tokens for c in cases.CASES) == 7


def test_edge_golden_file_matches_the_recipe():
    z = golden()
    assert len(cases.CASES) == cases.N_CASES and not set(cases.BY_NAME) & set(cases.EDGE_BY_NAME)
    assert sorted({k.split("/")[0] for k in np.load(EDGES).files}) == sorted(EDGE_NAMES)
    for c in cases.EDGE_CASES:
        h, w, B, n, box, multi, ih, iw, seed, sharp = z[f"{c.name}/params"].tolist()
        assert ((h, w), B, n, bool(box), bool(multi), (ih, iw), bool(sharp)) == (c.grid, c.B, c.n_points, c.box, c.multimask, c.input_size, c.sharp)
        assert c.input_size == (16 * h, 16 * w) and c.sampled
        coords, labels, boxes = cases.make_prompts(c, seed)
        for got, want in zip(prompts_of(c.name), (coords, labels, boxes)):
            assert (got is None) == (want is None) and (got is None or np.array_equal(got, want))
        assert z[f"{c.name}/sparse"].shape == (c.B, c.tokens - 5, 256)
        size = c.B * c.n_masks * 16 * h * w
        idx = z[f"{c.name}/sample_idx"]
        assert np.array_equal(idx, cases.edge_sample_index(size)) and (len(idx) == size if size <= 4096 else len(idx) <= 1536)
        assert z[f"{c.name}/ref64"].shape == z[f"{c.name}/ref32"].shape == idx.shape and z[f"{c.name}/iou64"].shape == (c.B, c.n_masks)
        assert float(z[f"{c.name}/delta"]) == 4 * float(z[f"{c.name}/gap"]) > 0
        assert float(z[f"{c.name}/delta_iou"]) == 4 * float(z[f"{c.name}/gap_iou"]) > 0
        if not c.sharp:
            assert int(z[f"{c.name}/nopen"]) <= 0.001 * size
    # the prompt streams continue after CASES': no edge case draws the prompts of another case
    streams = [cases._PROMPT_STREAM[n] for n in NAMES + EDGE_NAMES]
    assert streams == list(range(cases.N_CASES + len(EDGE_NAMES)))


def test_edge_cases_reach_the_edges_they_name():
    """computed from `grid` alone (csrc/sam_decoder.hip: 32-token tiles, CHUNK = 256 tokens per workgroup of the token -> image
    attention), so that an edit of the list cannot silently drop an edge"""
    TILE, CHUNK = 32, 256
    reach = {}
    for c in cases.EDGE_CASES:
        hw = c.grid[0] * c.grid[1]
        nch = -(-hw // CHUNK)
        reach[c.name] = (hw, hw % TILE, nch, hw - (nch - 1) * CHUNK)          # tokens, of the last tile (0: full), chunks, tokens of the last chunk
    assert reach == {"e4x8": (32, 0, 1, 32), "e3x11": (33, 1, 1, 33), "e15x17": (255, 31, 1, 255), "e16x16": (256, 0, 1, 256),
                     "e1x257": (257, 1, 2, 1), "e257x1": (257, 1, 2, 1), "e16x17": (272, 16, 2, 16), "e18x16": (288, 0, 2, 32),
                     "e17x31": (527, 15, 3, 15), "e16x17_sharp": (272, 16, 2, 16), "e128x128": (16384, 0, 64, 256)}
    assert {r[1] for r in reach.values()} >= {0, 1, 15, 16, 31}
    assert {r[2] for r in reach.values()} >= {1, 2, 3, 64}
    last = {r[3] for r in reach.values() if r[2] > 1}
    assert 1 in last and 32 in last and any(1 < n <= 16 for n in last)      # one token; one full tile then the break; thread-half 1 all masked
    assert any(r[2] == 1 and r[3] == CHUNK for r in reach.values()) and any(r[2] == 1 and r[3] == CHUNK - 1 for r in reach.values())
    multi = [c for c in cases.EDGE_CASES if -(-c.grid[0] * c.grid[1] // CHUNK) > 1]
    assert any(c.sharp for c in multi) and any(c.grid[0] == 1 for c in multi) and any(c.grid[1] == 1 for c in multi)
    import sam_decoder
    assert max(r[0] for r in reach.values()) == sam_decoder.MAX_GRID and max(c.tokens for c in cases.EDGE_CASES) == sam_decoder.MAX_TOKENS
    assert any(c.B * c.tokens == TILE for c in cases.EDGE_CASES)             # one full row tile of the token-side linear
    assert {c.multimask for c in cases.EDGE_CASES} == {True, False}


@pytest.mark.parametrize("name", NAMES + EDGE_NAMES)
def test_oracle_prompt_encoding_against_the_reference(name):
    c = ALL[name]
    coords, labels, boxes = prompts_of(name)
    got = oracle.sparse_tokens(oracle.as_torch(weights_of(name)), coords, labels, boxes, c.input_size).numpy()
    want = golden()[f"{name}/sparse"]
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.abs(got - want).max() <= 1e-6


@pytest.mark.parametrize("name", NAMES + EDGE_NAMES)
def test_oracle_float64_against_the_reference(name):
    """fed the reference's recorded float32 prompt tokens, the oracle's float64 chain is the reference's float64 chain (at the
    sample where a case records one: that is what entitles the GPU tests to judge whole tensors against the oracle)"""
    z, c = golden(), ALL[name]
    seed = int(z[f"{name}/params"][8])
    low, iou, _ = oracle.decode(weights_of(name), cases.make_features(c, seed), z[f"{name}/sparse"], c.multimask, torch.float64)
    low, iou = low.numpy(), iou.numpy()
    h, w = c.grid
    assert low.shape == (c.B, c.n_masks, 4 * h, 4 * w) and iou.shape == (c.B, c.n_masks)
    ref = z[f"{name}/ref64"]
    got = low.reshape(-1)[z[f"{name}/sample_idx"]] if c.sampled else low
    err, err_iou = np.abs(got - ref).max(), np.abs(iou - z[f"{name}/iou64"]).max()
    print(f"{name}: oracle float64 vs reference float64: logits {err:.3g}, iou {err_iou:.3g}")
    assert err <= 1e-9 * np.abs(ref).max()
    assert err_iou <= 1e-9 * max(np.abs(z[f"{name}/iou64"]).max(), 1.0)


def test_point_grid_closed_form():
    for n in (1, 4, 32):
        g = sd().point_grid(n)
        assert g.shape == (n * n, 2) and g.dtype == np.float64
        k = np.arange(n * n)
        want = np.stack([(k % n + 0.5) / n, (k // n + 0.5) / n], 1)          # x fastest
        assert np.abs(g - want).max() <= 1e-15
    with pytest.raises(ValueError, match="points_per_side"):
        sd().point_grid(0)


def test_parameter_table():
    t = sd().parameter_table()
    assert len(t) == 127 and len({n for n, _ in t}) == 127
    assert sum(int(np.prod(s)) for n, s in t if n.startswith("mask_decoder.")) == 4058340      # the decoder's 4.06 M parameters
    assert sum(int(np.prod(s)) for n, s in t if n.startswith("prompt_encoder.")) == 2 * 128 + 6 * 256
    assert t[0] == ("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", (2, 128))
    assert t[-1] == ("mask_decoder.iou_prediction_head.layers.2.bias", (4,))


def test_from_state_dict_errors():
    w = {k: torch.from_numpy(v) for k, v in weights_of("g4x4_fg").items()}
    SW = sd().SamDecoderWeights
    missing = dict(w)
    del missing["mask_decoder.transformer.layers.1.norm3.bias"]
    with pytest.raises(KeyError, match="mask_decoder.transformer.layers.1.norm3.bias"):
        SW.from_state_dict(missing)
    with pytest.raises(KeyError, match="sam.prompt_encoder.pe_layer"):
        SW.from_state_dict(w, prefix="sam.")
    bad = dict(w)
    bad["mask_decoder.iou_token.weight"] = torch.zeros(256)
    with pytest.raises(ValueError, match="mask_decoder.iou_token.weight"):
        SW.from_state_dict(bad)
    wide = dict(w)
    wide["mask_decoder.transformer.layers.0.mlp.lin1.weight"] = torch.zeros(1024, 256)
    with pytest.raises(NotImplementedError, match="mlp.lin1.weight"):
        SW.from_state_dict(wide)
    deep = dict(w)
    deep["mask_decoder.transformer.layers.2.norm1.weight"] = torch.zeros(256)
    with pytest.raises(NotImplementedError, match="depth 2"):
        SW.from_state_dict(deep)
    ints = dict(w)
    ints["mask_decoder.mask_tokens.weight"] = torch.zeros((4, 256), dtype=torch.int32)
    with pytest.raises(ValueError, match="mask_tokens"):
        SW.from_state_dict(ints)
    # a complete dict under a prefix, with the checkpoint's other entries beside it, passes every check: then the device is asked for
    full = {"sam." + k: v for k, v in w.items()}
    full["sam.image_encoder.pos_embed"] = torch.zeros(3)
    full["sam.prompt_encoder.mask_downscaling.0.weight"] = torch.zeros(4, 1, 2, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        SW.from_state_dict(full, prefix="sam.", device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            SW.from_state_dict(full, prefix="sam.")


def test_not_implemented_and_argument_errors():
    m = sd()
    plan = m.SamImagePlan(None, torch.zeros(1), (4, 4))
    pts, lab = torch.zeros((2, 1, 2)), torch.ones((2, 1), dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="mask_input"):
        m.predict(plan, pts, lab, mask_input=torch.zeros((2, 1, 16, 16)))
    with pytest.raises(NotImplementedError, match="17 tokens"):
        m.predict(plan, torch.zeros((2, 11, 2)), torch.ones((2, 11), dtype=torch.int32))          # 5 + 11 + the pad
    with pytest.raises(NotImplementedError, match="17 tokens"):
        m.predict(plan, torch.zeros((2, 10, 2)), torch.ones((2, 10), dtype=torch.int32), boxes=torch.zeros((2, 4)))
    with pytest.raises(ValueError, match="neither points nor boxes"):
        m.predict(plan, None, None)
    with pytest.raises(ValueError, match="point_labels"):
        m.predict(plan, pts, torch.ones((2, 2)))
    with pytest.raises(ValueError, match="boxes"):
        m.predict(plan, pts, lab, boxes=torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="SamImagePlan"):
        m.predict(object(), pts, lab)
    weights = m.SamDecoderWeights(torch.zeros(1))
    with pytest.raises(NotImplementedError, match="128 channels"):
        m.plan(weights, torch.zeros((128, 4, 4)))                                               # a wrong width
    with pytest.raises(NotImplementedError, match="16384"):
        m.plan(weights, torch.zeros((256, 129, 128)))
    with pytest.raises(ValueError, match="float32"):
        m.plan(weights, torch.zeros((256, 4, 4), dtype=torch.float64))
    predictor = m.SamFeaturePredictor(weights)
    with pytest.raises(NotImplementedError, match="image encoder"):
        predictor.set_image(np.zeros((32, 48, 3), np.uint8))
    with pytest.raises(RuntimeError, match="set_image"):
        predictor.predict_torch(pts, lab)
    with pytest.raises(RuntimeError, match="set_image"):
        predictor.get_image_embedding()
    with pytest.raises(NotImplementedError, match="crop"):
        m.generate(weights, torch.zeros((256, 4, 4)), (32, 48), crop_n_layers=1)


def test_install():
    import types
    m = sd()
    mod = types.ModuleType("segment_anything")
    with pytest.raises(AttributeError, match="SamPredictor"):
        m.install(mod)
    mod.SamPredictor = object
    assert m.install(mod) is mod and mod.SamPredictor is m.SamFeaturePredictor


def test_c_abi_argument_checks_without_gpu():
    """include/f3dgs.h: every refusal comes before any device work, so the addresses here are never dereferenced"""
    import ctypes
    from test_abi_and_surface import _ensure_built
    lib = ctypes.CDLL(_ensure_built())
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    lib.f3dgs_version.restype = ctypes.c_int
    assert lib.f3dgs_version() >= 32600
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    for fn in (lib.f3dgs_sam_decoder_weights_bytes, lib.f3dgs_sam_decoder_plan_bytes, lib.f3dgs_sam_decoder_scratch_bytes):
        fn.restype = sz
    lib.f3dgs_sam_decoder_plan_bytes.argtypes = [ci, ci]
    lib.f3dgs_sam_decoder_scratch_bytes.argtypes = [ci] * 4
    assert lib.f3dgs_sam_decoder_weights_bytes() >= 4060132 * 4 and lib.f3dgs_sam_decoder_weights_bytes() % 256 == 0
    assert lib.f3dgs_sam_decoder_plan_bytes(64, 64) == 4096 * 3584 and lib.f3dgs_sam_decoder_plan_bytes(129, 128) == 0
    assert lib.f3dgs_sam_decoder_plan_bytes(0, 4) == 0
    assert lib.f3dgs_sam_decoder_scratch_bytes(64, 64, 64, 7) >= 64 * 4096 * 1024
    assert lib.f3dgs_sam_decoder_scratch_bytes(1, 4, 4, 17) == 0 and lib.f3dgs_sam_decoder_scratch_bytes(1, 4, 4, 4) == 0
    A = 0x10000                                    # a 16-byte aligned, never dereferenced address
    lib.f3dgs_sam_decoder_pack_weights.argtypes = [vp, ci, vp, vp]
    table = (vp * 127)(*([A] * 127))
    assert lib.f3dgs_sam_decoder_pack_weights(table, 126, A, None) == -1 and b"127" in lib.f3dgs_last_error()
    assert lib.f3dgs_sam_decoder_pack_weights(table, 127, A + 4, None) == -1 and b"16-byte" in lib.f3dgs_last_error()
    table[5] = None
    assert lib.f3dgs_sam_decoder_pack_weights(table, 127, A, None) == -1 and b"parameter 5" in lib.f3dgs_last_error()
    lib.f3dgs_sam_decoder_plan.argtypes = [ci, ci, ci, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, vp, vp, vp]
    assert lib.f3dgs_sam_decoder_plan(128, 4, 4, A, 16, 4, 1, A, A, None) == -4                  # F3DGS_ERR_UNSUPPORTED: another width
    assert lib.f3dgs_sam_decoder_plan(256, 129, 128, A, 16, 4, 1, A, A, None) == -4
    assert lib.f3dgs_sam_decoder_plan(256, 0, 4, A, 16, 4, 1, A, A, None) == -1
    assert lib.f3dgs_sam_decoder_plan(256, 4, 4, A, 16, -4, 1, A, A, None) == -1 and b"stride" in lib.f3dgs_last_error()
    assert lib.f3dgs_sam_decoder_plan(256, 4, 4, A, 16, 4, 1, A, A + 8, None) == -1 and b"16-byte" in lib.f3dgs_last_error()
    assert lib.f3dgs_sam_decoder_plan(256, 4, 4, None, 16, 4, 1, A, A, None) == -1 and b"null" in lib.f3dgs_last_error()
    lib.f3dgs_sam_decoder_predict.argtypes = [ci] * 4 + [vp] * 3 + [ci] * 3 + [vp] * 5 + [sz, vp]
    predict = lambda B, n, boxes, scratch=A, bytes_=1 << 40, low=A: lib.f3dgs_sam_decoder_predict(
        B, 4, 4, n, A, A, boxes, 64, 64, 1, A, A, low, A, scratch, bytes_, None)
    assert predict(2, 11, None) == -4 and b"17 tokens" in lib.f3dgs_last_error()                  # 5 + 11 + the pad
    assert predict(2, 10, A) == -4 and predict(2, 9, A, bytes_=16) == -1 and b"scratch" in lib.f3dgs_last_error()
    assert predict(70000, 1, None) == -4
    assert predict(-1, 1, None) == -1 and predict(2, 0, None) == -1 and b"neither" in lib.f3dgs_last_error()
    assert predict(2, 1, None, low=A + 4) == -1 and b"16-byte" in lib.f3dgs_last_error()
    assert predict(2, 1, None, scratch=None) == -1
    assert predict(0, 1, None, scratch=None, low=None) == 0                                         # B == 0: a no-op
