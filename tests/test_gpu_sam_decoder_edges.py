"""The SAM decoder on the GPU at the edges of its two partitions of the hw image tokens (csrc/sam_decoder.hip): the 32-token tiles
of sd_src / sd_lin / sd_i2t / sd_upscale and of each round of sd_t2i, and the 256-token chunks of sd_t2i that sd_t2i_combine
joins.  The cases are EDGE_CASES of tests/sam_decoder_cases.py (one full tile, a tile plus a row, a chunk less one token, one full
chunk, a second chunk of one token with h = 1 and with w = 1, of half a tile, of one full tile, three chunks, scores beyond 88
across two chunks, and the grid limit of 16384 tokens = 64 chunks); test_sam_decoder_cpu.py asserts that they reach those edges.

Bars, as in test_gpu_sam_decoder.py: per case delta = 4 x max |reference float32 - reference float64| over the case's whole output,
recorded by the generator (tests/golden/reference_sam_decoder_edges.npz), for the logits and the IoU predictions separately.  The
file holds a sample of each case's logits; every logit of the sample lies within delta of the reference's float64, and every logit
of the WHOLE tensor within delta of the float64 oracle (tests/sam_decoder_oracle.py), which test_sam_decoder_cpu.py pins to the
reference's float64 at the sample to 1e-9 relative.  The oracle runs once per case in float64 on the host - for e128x128 on the
device (786,432 logits: seconds on a host of few cores) - and is shared.  A logit whose float64 value lies within delta of 0 is
OPEN (at most 0.1 % of a case), every other has the float64 sign.  The sharp case is held to finiteness and its own delta.
Batch invariance, repeatability, graph replay, plan reuse and the strided features are bit equalities at more than one chunk, so
that the combine and the `part` scratch are inside them; the C entry's writes are held inside its buffers by guard bands."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sam_decoder_cases as cases
import sam_decoder_oracle as oracle
from test_gpu_sam_decoder import DEV, _DEV_W, _HOST_W, sd          # the packed weights of a (seed, scale) are shared with that file
from util import ROOT

pytestmark = pytest.mark.gpu

EDGES = os.path.join(ROOT, "tests", "golden", "reference_sam_decoder_edges.npz")
NAMES = [c.name for c in cases.EDGE_CASES]
ON_DEVICE = {"e128x128"}                            # where the float64 oracle runs on the device
_Z, _RUN, _ORACLE = {}, {}, {}


def golden():
    if not _Z:
        _Z.update(np.load(EDGES))
    return _Z


def seed_of(name):
    return int(golden()[f"{name}/params"][8])


def host_weights(name):
    key = (seed_of(name), cases.EDGE_BY_NAME[name].qk_scale)
    if key not in _HOST_W:
        _HOST_W[key] = cases.make_weights(*key)
    return _HOST_W[key]


def weights(name):
    """the packed weights of a case on the device, made once and left unchanged"""
    key = (seed_of(name), cases.EDGE_BY_NAME[name].qk_scale)
    if key not in _DEV_W:
        _DEV_W[key] = sd().SamDecoderWeights.from_state_dict({k: torch.from_numpy(v) for k, v in host_weights(name).items()}, device=DEV)
    return _DEV_W[key]


def features(name, seed=None):
    return torch.from_numpy(cases.make_features(cases.EDGE_BY_NAME[name], seed_of(name) if seed is None else seed)).to(DEV)


def prompts(name):
    z = golden()
    return tuple(torch.from_numpy(z[f"{name}/{k}"]).to(DEV) if f"{name}/{k}" in z else None for k in ("coords", "labels", "boxes"))


def run(name):
    """(low_res, iou) of an edge case as numpy, computed once and shared"""
    if name not in _RUN:
        c = cases.EDGE_BY_NAME[name]
        plan = sd().plan(weights(name), features(name))
        low, iou = sd().predict(plan, *prompts(name), multimask_output=c.multimask, input_size=c.input_size)
        h, w = c.grid
        assert low.shape == (c.B, c.n_masks, 4 * h, 4 * w) and iou.shape == (c.B, c.n_masks)
        assert low.dtype == torch.float32 and iou.dtype == torch.float32 and low.is_contiguous()
        _RUN[name] = (low.cpu().numpy(), iou.cpu().numpy())
    return _RUN[name]


def oracle64(name):
    """(low_res, iou) of the float64 oracle over the whole output, computed once and shared, left unchanged"""
    if name not in _ORACLE:
        z, c = golden(), cases.EDGE_BY_NAME[name]
        W = host_weights(name)
        get = lambda k: z[f"{name}/{k}"] if f"{name}/{k}" in z else None
        sparse = oracle.sparse_tokens(oracle.as_torch(W), get("coords"), get("labels"), get("boxes"), c.input_size)
        with torch.no_grad():
            low, iou, _ = oracle.decode(W, cases.make_features(c, seed_of(name)), sparse, c.multimask, torch.float64,
                                        device=DEV if name in ON_DEVICE else None, want_info=False)
        assert low.dtype == torch.float64
        _ORACLE[name] = (low.cpu().numpy(), iou.cpu().numpy())
    return _ORACLE[name]


# ---- 1. parity: the recorded reference at the sample, the float64 oracle over the whole tensor ------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_edge_parity(name):
    z = golden()
    low, iou = run(name)
    want, want_iou = oracle64(name)
    assert np.isfinite(low).all() and np.isfinite(iou).all() and np.isfinite(want).all()
    idx, ref = z[f"{name}/sample_idx"], z[f"{name}/ref64"]
    gap, gap_iou = float(z[f"{name}/gap"]), float(z[f"{name}/gap_iou"])
    err, err_all = np.abs(low.reshape(-1)[idx] - ref).max(), np.abs(low - want).max()
    err_iou, err_iou_o = np.abs(iou - z[f"{name}/iou64"]).max(), np.abs(iou - want_iou).max()
    print(f"{name}: max|out - ref64| = {err:.3g} = {err / gap:.2f} gap at the {len(idx)} sampled logits, max|out - oracle64| = {err_all:.3g} = "
          f"{err_all / gap:.2f} gap over all {low.size}; iou {err_iou:.3g} = {err_iou / gap_iou:.2f} gap (oracle: {err_iou_o / gap_iou:.2f}); "
          f"the reference's own float32: gap {gap:.3g}, {gap_iou:.3g}")
    assert err <= float(z[f"{name}/delta"])
    assert err_all <= float(z[f"{name}/delta"])
    assert err_iou <= float(z[f"{name}/delta_iou"]) and err_iou_o <= float(z[f"{name}/delta_iou"])


# ---- 2. binary masks over the whole tensor -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in cases.EDGE_CASES if not c.sharp])
def test_edge_binary_masks(name):
    low, _ = run(name)
    want, _ = oracle64(name)
    decided = np.abs(want) > float(golden()[f"{name}/delta"])
    assert decided.mean() >= 0.999
    assert np.array_equal((low > 0)[decided], (want > 0)[decided])


# ---- 3. the C entry writes inside its buffers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e257x1", "e1x257", "e16x17"])
def test_writes_stay_inside_the_buffers(name):
    """f3dgs_sam_decoder_predict on device pointers: low_res, iou and the scratch each lie between two guard bands of a larger
    buffer.  The bands are intact afterwards and the outputs are the bits of the Python call (so every element was written)."""
    c = cases.EDGE_BY_NAME[name]
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.f3dgs_sam_decoder_scratch_bytes.restype = sz
    lib.f3dgs_sam_decoder_scratch_bytes.argtypes = [ci] * 4
    lib.f3dgs_sam_decoder_predict.argtypes = [ci] * 4 + [vp] * 3 + [ci] * 3 + [vp] * 5 + [sz, vp]
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    h, w = c.grid
    plan = sd().plan(weights(name), features(name))
    coords, labels, boxes = prompts(name)
    want = sd().predict(plan, coords, labels, boxes, multimask_output=c.multimask, input_size=c.input_size)
    n_low, n_iou, G = c.B * c.n_masks * 16 * h * w, c.B * c.n_masks, 4096          # G floats: more than a 32-token tile's 4 x 4 blocks of a row
    nbytes = lib.f3dgs_sam_decoder_scratch_bytes(c.B, h, w, c.tokens)
    assert nbytes > 0 and nbytes % 16 == 0
    SENT = -7777.25
    low_store = torch.full((G + n_low + G,), SENT, device=DEV)
    iou_store = torch.full((G + n_iou + G,), SENT, device=DEV)
    scr_store = torch.full((4 * G + nbytes + 4 * G,), 0x5A, dtype=torch.uint8, device=DEV)
    low, iou, scr = low_store[G:G + n_low], iou_store[G:G + n_iou], scr_store[4 * G:4 * G + nbytes]
    assert low.data_ptr() % 16 == 0 and scr.data_ptr() % 16 == 0
    rc = lib.f3dgs_sam_decoder_predict(c.B, h, w, c.n_points, None if coords is None else coords.data_ptr(), None if labels is None else labels.data_ptr(),
                                       None if boxes is None else boxes.data_ptr(), c.input_size[0], c.input_size[1], int(c.multimask),
                                       plan.data.data_ptr(), plan.weights.packed.data_ptr(), low.data_ptr(), iou.data_ptr(), scr.data_ptr(), nbytes,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.f3dgs_last_error()
    torch.cuda.synchronize()
    for store, n, fill in ((low_store, n_low, SENT), (iou_store, n_iou, SENT), (scr_store, nbytes, 0x5A)):
        g = len(store) - n >> 1
        assert bool((store[:g] == fill).all()) and bool((store[g + n:] == fill).all())
    assert torch.equal(low.reshape(want[0].shape), want[0]) and torch.equal(iou.reshape(want[1].shape), want[1])


# ---- 4. batch invariance at two chunks ---------------------------------------------------------------------------------------------------
def test_batch_invariance_bitwise_two_chunks():
    """a prompt alone, first of 3, last of 3 and at position 67 of 70, on a 16 x 17 grid: two chunks, the second half a tile"""
    name = "e16x17"
    c = cases.EDGE_BY_NAME[name]
    plan = sd().plan(weights(name), features(name))
    coords, labels, _ = prompts(name)
    rng = np.random.default_rng(5)
    ih, iw = c.input_size
    fill_c = torch.from_numpy((rng.uniform(0, 1, (70, 3, 2)) * np.array([iw, ih])).astype(np.float32)).to(DEV)
    fill_l = torch.from_numpy(rng.integers(-1, 2, (70, 3)).astype(np.int32)).to(DEV)
    one = lambda cc, ll: sd().predict(plan, cc, ll, multimask_output=True, input_size=c.input_size)
    alone = one(coords[:1], labels[:1])
    first = one(torch.cat([coords[:1], fill_c[:2]]), torch.cat([labels[:1], fill_l[:2]]))
    last = one(torch.cat([fill_c[:2], coords[:1]]), torch.cat([fill_l[:2], labels[:1]]))
    big_c, big_l = fill_c.clone(), fill_l.clone()
    big_c[67], big_l[67] = coords[0], labels[0]
    big = one(big_c, big_l)
    assert not torch.equal(big[0][66], big[0][67])
    for got, at in ((first, 0), (last, 2), (big, 67)):
        assert torch.equal(got[0][at], alone[0][0]) and torch.equal(got[1][at], alone[1][0]), at
    assert torch.equal(big[0][:2], last[0][:2]) and torch.equal(big[1][:2], last[1][:2])
    assert torch.equal(alone[0][0], torch.from_numpy(run(name)[0][0]).to(DEV))          # and the bits of the golden run's first prompt


# ---- 5. repeatability and graph replay at three chunks -----------------------------------------------------------------------------------
def test_repeatable_and_capturable_three_chunks():
    name = "e17x31"
    c = cases.EDGE_BY_NAME[name]
    plan = sd().plan(weights(name), features(name))
    p = prompts(name)
    call = lambda: sd().predict(plan, *p, multimask_output=c.multimask, input_size=c.input_size)
    a, b = call(), call()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no parallel branches
        captured = call()
    for _ in range(2):
        for t in captured:
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured[0], a[0]) and torch.equal(captured[1], a[1])


# ---- 6. plan reuse at two chunks -------------------------------------------------------------------------------------------------------------
def test_plan_reuse_leaves_nothing_behind_two_chunks():
    """two feature maps and two prompt sets interleaved, each the bits of a fresh plan's result: the `part` and `keys` scratch of
    two chunks carries nothing from one call to the next"""
    name = "e16x17"
    c = cases.EDGE_BY_NAME[name]
    W = weights(name)
    f0, f1 = features(name), features(name, seed=seed_of(name) + 100)
    coords, labels, _ = prompts(name)
    other_c = torch.flip(coords, dims=(0, 1)) * 0.5
    kw = dict(multimask_output=True, input_size=c.input_size)
    fresh = lambda f, cc: sd().predict(sd().plan(W, f), cc, labels, **kw)
    want00, want01, want10 = fresh(f0, coords), fresh(f0, other_c), fresh(f1, coords)
    assert not torch.equal(want00[0], want01[0]) and not torch.equal(want00[0], want10[0])
    plan0 = sd().plan(W, f0)
    got00, got01 = sd().predict(plan0, coords, labels, **kw), sd().predict(plan0, other_c, labels, **kw)
    plan1 = sd().plan(W, f1)
    got10 = sd().predict(plan1, coords, labels, **kw)
    again00 = sd().predict(plan0, coords, labels, **kw)
    for got, want in ((got00, want00), (got01, want01), (got10, want10), (again00, want00)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- 7. strided features at two chunks -----------------------------------------------------------------------------------------------------
def test_strided_features_are_read_in_place_two_chunks():
    name = "e16x17"
    c = cases.EDGE_BY_NAME[name]
    W = weights(name)
    f = features(name)
    big = torch.full((300, 19, 22), 7.5, device=DEV)                  # a larger render: the map is channels 20.., rows 2.., columns 3..
    view = big[20:276, 2:18, 3:20]
    view.copy_(f)
    assert not view.is_contiguous() and view.data_ptr() != f.data_ptr()
    hwc = f.permute(1, 2, 0).contiguous().permute(2, 0, 1)            # channel-last memory under the same shape
    assert hwc.stride(0) == 1
    coords, labels, _ = prompts(name)
    kw = dict(multimask_output=True, input_size=c.input_size)
    want = sd().predict(sd().plan(W, f), coords, labels, **kw)
    for v in (view, hwc, f[None]):
        got = sd().predict(sd().plan(W, v), coords, labels, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(view, f)
    outside = big.clone()
    outside[20:276, 2:18, 3:20] = 7.5
    assert bool((outside == 7.5).all())                               # the surrounding tensor is untouched
