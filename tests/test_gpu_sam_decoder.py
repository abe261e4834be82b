"""The SAM prompt encoder and mask decoder on the GPU (feature-3dgs_amd/sam_decoder.py, csrc/sam_decoder.hip) against the
reference's recorded results (tests/golden/reference_sam_decoder.npz) and the independent oracle (tests/sam_decoder_oracle.py).

Bars.  Per case delta = 4 x max |reference float32 - reference float64| of that case, for the logits and for the IoU predictions
separately (recorded by the generator over the case's whole output): both are fp32 chains of the same length that differ only in
their summation order.  Every logit and IoU prediction lies within its delta of the reference's float64 value; a logit whose
float64 value lies within delta of 0 is OPEN (at most 0.1 % of a case), every other has the float64 sign.  The `sharp` case
(token -> image scores beyond 88) is held to finiteness and its own delta.  Batch invariance, repeatability, graph replay, plan
reuse and the strided features are bit equalities.  Strided features are READ IN PLACE (any non-negative strides) and give the
bits of their contiguous copy."""
import os

import numpy as np
import pytest
import torch

import sam_decoder_cases as cases
import sam_decoder_oracle as oracle
from util import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_sam_decoder.npz")
DEV = "cuda:0"
NAMES = [c.name for c in cases.CASES]
_Z, _HOST_W, _DEV_W, _RUN = {}, {}, {}, {}


def sd():
    import sam_decoder
    return sam_decoder


def golden():
    if not _Z:
        _Z.update(np.load(GOLDEN))
    return _Z


def seed_of(name):
    return int(golden()[f"{name}/params"][8])


def host_weights(name):
    key = (seed_of(name), cases.BY_NAME[name].qk_scale)
    if key not in _HOST_W:
        _HOST_W[key] = cases.make_weights(*key)
    return _HOST_W[key]


def weights(name="g8x5_three_labels"):
    """the packed weights of a case on the device, made once and left unchanged"""
    key = (seed_of(name), cases.BY_NAME[name].qk_scale)
    if key not in _DEV_W:
        _DEV_W[key] = sd().SamDecoderWeights.from_state_dict({k: torch.from_numpy(v) for k, v in host_weights(name).items()}, device=DEV)
    return _DEV_W[key]


def features(name, seed=None):
    return torch.from_numpy(cases.make_features(cases.BY_NAME[name], seed_of(name) if seed is None else seed)).to(DEV)


def prompts(name):
    z = golden()
    return tuple(torch.from_numpy(z[f"{name}/{k}"]).to(DEV) if f"{name}/{k}" in z else None for k in ("coords", "labels", "boxes"))


def run(name):
    """(low_res, iou) of a golden case as numpy, computed once and shared"""
    if name not in _RUN:
        c = cases.BY_NAME[name]
        plan = sd().plan(weights(name), features(name))
        low, iou = sd().predict(plan, *prompts(name), multimask_output=c.multimask, input_size=c.input_size)
        h, w = c.grid
        assert low.shape == (c.B, c.n_masks, 4 * h, 4 * w) and iou.shape == (c.B, c.n_masks)
        assert low.dtype == torch.float32 and iou.dtype == torch.float32 and low.is_contiguous()
        _RUN[name] = (low.cpu().numpy(), iou.cpu().numpy())
    return _RUN[name]


def compared(name):
    """(got, ref64) of the logits the golden file holds for the case"""
    z, c = golden(), cases.BY_NAME[name]
    low, _ = run(name)
    return (low.reshape(-1)[z[f"{name}/sample_idx"]] if c.sampled else low), z[f"{name}/ref64"]


# ---- 1. golden parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_golden_parity(name):
    z = golden()
    got, ref = compared(name)
    _, iou = run(name)
    assert np.isfinite(got).all() and np.isfinite(iou).all() and np.isfinite(run(name)[0]).all()
    err, err_iou = np.abs(got - ref).max(), np.abs(iou - z[f"{name}/iou64"]).max()
    gap, gap_iou = float(z[f"{name}/gap"]), float(z[f"{name}/gap_iou"])
    print(f"{name}: max|out - ref64| = {err:.3g} = {err / gap:.2f} gap (logits), {err_iou:.3g} = {err_iou / gap_iou:.2f} gap (iou); "
          f"the reference's own float32: gap {gap:.3g}, {gap_iou:.3g}")
    assert err <= float(z[f"{name}/delta"])
    assert err_iou <= float(z[f"{name}/delta_iou"])


# ---- 2. binary masks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in NAMES if n != "sharp"])
def test_binary_masks(name):
    got, ref = compared(name)
    decided = np.abs(ref) > float(golden()[f"{name}/delta"])
    assert decided.mean() >= 0.999
    assert np.array_equal((got > 0)[decided], (ref > 0)[decided])


# ---- 3. full-size parity against the float64 oracle -------------------------------------------------------------------------------
def test_full_size_parity_against_the_oracle():
    name = "g64x64"
    z, c = golden(), cases.BY_NAME[name]
    coords, labels, boxes = (None if t is None else t.cpu() for t in prompts(name))
    W = host_weights(name)
    sparse = oracle.sparse_tokens(oracle.as_torch(W), coords, labels, boxes, c.input_size)
    want, want_iou, _ = oracle.decode(W, cases.make_features(c, seed_of(name)), sparse, c.multimask, torch.float64)
    low, iou = run(name)
    err, err_iou = np.abs(low - want.numpy()).max(), np.abs(iou - want_iou.numpy()).max()
    print(f"{name}, all {low.size} logits: max|out - oracle64| = {err:.3g} = {err / float(z[f'{name}/gap']):.2f} gap, iou {err_iou:.3g}")
    assert err <= float(z[f"{name}/delta"]) and err_iou <= float(z[f"{name}/delta_iou"])


# ---- 4. batch invariance ---------------------------------------------------------------------------------------------------------
def test_batch_invariance_bitwise():
    """a prompt alone, first of 3, last of 3 and inside a batch of 70 (more than one token row tile, more than 64 prompts)"""
    name = "g8x5_three_labels"
    c = cases.BY_NAME[name]
    plan = sd().plan(weights(name), features(name))
    coords, labels, _ = prompts(name)
    rng = np.random.default_rng(5)
    fill_c = torch.from_numpy((rng.uniform(0, 1, (70, 3, 2)) * np.array([80, 128])).astype(np.float32)).to(DEV)
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


# ---- 5. repeatability --------------------------------------------------------------------------------------------------------------
def test_repeatable_and_capturable():
    name = "g8x5_box_9pts"
    c = cases.BY_NAME[name]
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


# ---- 6. plan reuse -----------------------------------------------------------------------------------------------------------------
def test_plan_reuse_leaves_nothing_behind():
    name = "g8x5_three_labels"
    c = cases.BY_NAME[name]
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


# ---- 7. strided features -----------------------------------------------------------------------------------------------------------
def test_strided_features_are_read_in_place():
    name = "g8x5_three_labels"
    c = cases.BY_NAME[name]
    W = weights(name)
    f = features(name)
    big = torch.full((300, 11, 9), 7.5, device=DEV)                   # a larger render: the map is channels 20.., rows 2.., columns 3..
    view = big[20:276, 2:10, 3:8]
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
    assert float(big[0, 0, 0]) == 7.5 and torch.equal(view, f)


# ---- 8. the surface chain ------------------------------------------------------------------------------------------------------------
def test_predictor_is_predict_then_upscale():
    import sam_masks
    name = "g8x5_three_labels"
    W, f = weights(name), features(name)
    coords, labels, _ = prompts(name)
    predictor = sd().SamFeaturePredictor(W, img_size=128)
    predictor.set_image((50, 31), features=f)                       # the longest side to 128: input (128, 79)
    assert predictor.original_size == (50, 31) and predictor.input_size == (128, 79) and predictor.is_image_set
    assert predictor.get_image_embedding().shape == (1, 256, 8, 5)
    low, iou = sd().predict(sd().plan(W, f), coords, labels, multimask_output=True, input_size=(128, 128))
    masks, iou_p, low_p = predictor.predict_torch(coords, labels, return_logits=True)
    assert torch.equal(low_p, low) and torch.equal(iou_p, iou)
    want = sam_masks.upscale_masks(low, 128, (128, 79), (50, 31))
    assert masks.shape == (3, 3, 50, 31) and torch.equal(masks, want)
    binary, _, _ = predictor.predict_torch(coords, labels)
    assert binary.dtype == torch.bool and torch.equal(binary, want > predictor.mask_threshold)
    single, iou_s, low_s = predictor.predict_torch(coords, labels, multimask_output=False)
    assert single.shape == (3, 1, 50, 31) and iou_s.shape == (3, 1) and low_s.shape == (3, 1, 32, 20)
    predictor.reset_image()
    assert not predictor.is_image_set
    with pytest.raises(RuntimeError, match="set_image"):
        predictor.predict_torch(coords, labels)


def test_generate_is_the_hand_written_chain():
    """points_per_side 4, points_per_batch 5: batches of 5, 5, 5 and 1"""
    import sam_masks
    name = "g8x5_three_labels"
    W, f = weights(name), features(name)
    H, Wd, S = 50, 31, 128
    kw = dict(pred_iou_thresh=-10.0, stability_score_thresh=0.0, box_nms_thresh=0.9)          # keep (nearly) everything: the chain is what is compared
    got = sd().generate(W, f, (H, Wd), points_per_side=4, points_per_batch=5, img_size=S, **kw)
    plan = sd().plan(W, f)
    pp = sam_masks.MaskPostprocessor((H, Wd), **kw)
    k = np.arange(16)
    pts = np.stack([(k % 4 + 0.5) / 4 * Wd, (k // 4 + 0.5) / 4 * H], 1)
    inp = (128, 79)
    for at in (0, 5, 10, 15):
        batch = pts[at:at + 5]
        scaled = batch * np.array([[inp[1] / Wd, inp[0] / H]])
        coords = torch.as_tensor(scaled, dtype=torch.float32, device=DEV)[:, None, :]
        labels = torch.ones((len(batch), 1), dtype=torch.int32, device=DEV)
        low, iou = sd().predict(plan, coords, labels, multimask_output=True, input_size=(S, S))
        assert low.shape == (len(batch), 3, 32, 20)
        pp.add_batch(low, iou, batch, (0, 0, Wd, H), inp, (H, Wd), S)
    want = pp.finish()
    assert len(got) == len(want) > 0
    assert got == want


# ---- 9. B = 0 ------------------------------------------------------------------------------------------------------------------------
def test_empty_batch():
    name = "g8x5_three_labels"
    plan = sd().plan(weights(name), features(name))
    for multi, m in ((True, 3), (False, 1)):
        low, iou = sd().predict(plan, torch.zeros((0, 2, 2), device=DEV), torch.zeros((0, 2), dtype=torch.int32, device=DEV), multimask_output=multi)
        assert low.shape == (0, m, 32, 20) and iou.shape == (0, m) and low.dtype == torch.float32
    low, iou = sd().predict(plan, None, None, boxes=torch.zeros((0, 4), device=DEV))
    assert low.shape == (0, 3, 32, 20)
    torch.cuda.synchronize()
