"""LPIPS (VGG16) on the GPU (feature-3dgs_amd/lpips_vgg.py, csrc/lpips.hip) against the reference's recorded results
(tests/golden/reference_lpips.npz) and the independent oracle (tests/lpips_oracle.py).

Bars (the project's convention: 4 x the reference's own float32-to-float64 gap, recorded by the generator).  Every tap element
lies within 4 gap_tap[l] of float64 - at the recorded sample against the reference's float64, and over the WHOLE tensor against
the float64 oracle, which tests/test_lpips_cpu.py pins to the reference at the same sample (the whole taps do not fit a committed
file); every layer term and total lies within 4 gap_rel relative of the reference's float64.  Exact zeros, symmetry,
repeatability, batch invariance, graph replay and the input forms are bit equalities; strided inputs are READ IN PLACE."""
import os
import types

import numpy as np
import pytest
import torch

import lpips_cases as cases
import lpips_oracle as oracle
from util import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_lpips.npz")
DEV = "cuda:0"
NAMES = [c.name for c in cases.CASES]
_Z, _HOST_W, _DEV_W, _PAIRS = {}, {}, {}, {}


def lv():
    import lpips_vgg
    return lpips_vgg


def golden():
    if not _Z:
        _Z.update(np.load(GOLDEN))
    return _Z


def host_weights(dead=False):
    if dead not in _HOST_W:
        _HOST_W[dead] = cases.make_weights(cases.SEED, dead)
    return _HOST_W[dead]


def weights(dead=False):
    """the packed weights on the device, made once and left unchanged"""
    if dead not in _DEV_W:
        _DEV_W[dead] = lv().LpipsWeights.from_state_dicts({k: torch.from_numpy(v) for k, v in host_weights(dead).items()}, device=DEV)
    return _DEV_W[dead]


def pairs(name):
    """(x, y) of a case on the device (and on the host), made once and left unchanged"""
    if name not in _PAIRS:
        x, y = cases.make_pairs(cases.BY_NAME[name], cases.SEED)
        _PAIRS[name] = (torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), x, y)
    return _PAIRS[name]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", NAMES)
def test_taps_terms_and_totals_against_the_reference(name):
    z, c = golden(), cases.BY_NAME[name]
    x, y, hx, hy = pairs(name)
    w = weights(c.dead)
    gap_tap, gap_rel = z[f"{name}/gap_tap"], float(z[f"{name}/gap_rel"])
    taps = lv().vgg_taps(w, torch.cat([x, y]))
    full = None if name == "mid" else oracle.taps(host_weights(c.dead), np.concatenate([hx, hy]), torch.float64)
    for l, t in enumerate(taps):
        assert tuple(t.shape) == cases.tap_shapes(c)[l] and t.dtype == torch.float32
        got = t.cpu().double().reshape(-1).numpy()
        err = np.abs(got[cases.sample_index(got.size, c.samples, l)] - z[f"{name}/tap64_{l}"]).max()
        print(f"{name} tap {l}: max error at the sample {err:.3g}, bar {4 * gap_tap[l]:.3g}")
        assert err <= 4 * gap_tap[l], (name, l, err, gap_tap[l])
        if full is not None:
            err = np.abs(got - full[l].reshape(-1).numpy()).max()
            print(f"{name} tap {l}: max error over the tensor {err:.3g}")
            assert err <= 4 * gap_tap[l], (name, l, err, gap_tap[l])
    terms = lv().layer_terms(x, y, w).cpu().double().numpy()
    totals = lv().lpips_views(x, y, w).cpu().double().numpy()
    t64, tot64 = z[f"{name}/terms64"], z[f"{name}/total64"]
    live = t64 > 0
    print(f"{name}: terms {terms.tolist()}, relative error {(np.abs(terms - t64)[live] / t64[live]).max() if live.any() else 0:.3g}, "
          f"totals' {(np.abs(totals - tot64)[tot64 > 0] / tot64[tot64 > 0]).max():.3g}, bar {4 * gap_rel:.3g}")
    assert terms.shape == t64.shape and totals.shape == tot64.shape
    assert (np.abs(terms - t64) <= 4 * gap_rel * t64).all(), (name, terms, t64, gap_rel)
    assert (np.abs(totals - tot64) <= 4 * gap_rel * tot64).all(), (name, totals, tot64, gap_rel)


def test_exact_zero():
    x, y, _, _ = pairs("batch3")
    w = weights()
    assert cases.BY_NAME["batch3"].kinds[0] == "same"
    assert (bits(lv().layer_terms(x, y, w))[0] == 0).all() and bits(lv().lpips_views(x, y, w))[0] == 0
    assert (bits(lv().layer_terms(x, x, w)) == 0).all() and (bits(lv().lpips_views(y, y, w)) == 0).all()
    dx, dy, _, _ = pairs("dead")
    terms = lv().layer_terms(dx, dy, weights(True))
    assert (bits(terms)[:, 4] == 0).all() and (terms[:, :4] > 0).all()
    assert all((t == 0).all() for t in lv().vgg_taps(weights(True), dx)[4:])


def test_symmetry():
    for name in ("batch3", "odd"):
        x, y, _, _ = pairs(name)
        assert torch.equal(bits(lv().layer_terms(x, y, weights())), bits(lv().layer_terms(y, x, weights())))
        assert torch.equal(bits(lv().lpips_views(x, y, weights())), bits(lv().lpips_views(y, x, weights())))


def test_repeatability_and_batch_invariance():
    x, y, _, _ = pairs("batch3")
    w = weights()
    whole = bits(lv().layer_terms(x, y, w))
    assert torch.equal(whole, bits(lv().layer_terms(x, y, w)))                       # a second call
    totals = bits(lv().lpips_views(x, y, w))
    for k in range(3):
        assert torch.equal(bits(lv().layer_terms(x[k:k + 1], y[k:k + 1], w))[0], whole[k])      # alone
        assert torch.equal(bits(lv().lpips_views(x[k], y[k], w))[0], totals[k])                 # (3,H,W)
    for shift in (1, 2):                                                             # every pair at every position
        order = [(k + shift) % 3 for k in range(3)]
        assert torch.equal(bits(lv().layer_terms(x[order], y[order], w)), whole[order])
    five = [0, 1, 2, 1, 0]                                                           # another batch size
    assert torch.equal(bits(lv().layer_terms(x[five], y[five], w)), whole[five])


def test_graph_capture_replays_on_new_contents():
    x, y, _, _ = pairs("odd")
    x2, y2 = (torch.from_numpy(t).to(DEV) for t in cases.make_pairs(cases.BY_NAME["odd"], cases.SEED + 1))      # other images
    w = weights()
    sx, sy = x.clone(), y.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lv().lpips_views(sx, sy, w)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = lv().lpips_views(sx, sy, w)
    g.replay()
    assert torch.equal(bits(out), bits(lv().lpips_views(x, y, w)))
    sx.copy_(x2)
    sy.copy_(y2)
    g.replay()
    assert torch.equal(bits(out), bits(lv().lpips_views(x2, y2, w)))
    assert not torch.equal(bits(out), bits(lv().lpips_views(x, y, w)))


def test_uint8_and_quantize():
    x, y, _, _ = pairs("odd")
    w = weights()
    bx, by = (x * 255).round().to(torch.uint8), (y * 255).round().to(torch.uint8)
    # the quotients are formed on the host: on the device torch multiplies by the rounded reciprocal, which is not v / 255
    fx, fy = ((t.cpu().float() / 255).to(DEV) for t in (bx, by))
    ref = bits(lv().layer_terms(fx, fy, w))
    assert torch.equal(bits(lv().layer_terms(bx, by, w)), ref)
    assert torch.equal(bits(lv().layer_terms(bx, fy, w)), ref) and torch.equal(bits(lv().layer_terms(fx, by, w)), ref)
    qx, qy = ((torch.floor(torch.clamp(t.cpu() * 255 + 0.5, 0, 255)) / 255).to(DEV) for t in (x, y))      # image_metrics' rounding
    pre = bits(lv().layer_terms(qx, qy, w))
    assert torch.equal(bits(lv().layer_terms(x, y, w, quantize=True)), pre)
    assert torch.equal(bits(lv().layer_terms(x, qy, w, quantize=(True, False))), pre)
    assert not torch.equal(bits(lv().layer_terms(x, y, w)), pre)
    for a, b in zip(lv().vgg_taps(w, x, quantize=True), lv().vgg_taps(w, qx)):
        assert torch.equal(bits(a), bits(b))


def test_strided_inputs_are_read_in_place():
    x, y, _, _ = pairs("odd")
    w = weights()
    ref = bits(lv().layer_terms(x, y, w))
    N, _, H, W = x.shape
    last = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)                    # a channels-last view
    big = torch.rand(N, 3, H + 9, W + 14, device=DEV)
    big[:, :, 4:4 + H, 5:5 + W] = y
    crop = big[:, :, 4:4 + H, 5:5 + W]
    assert not last.is_contiguous() and not crop.is_contiguous()
    ws = lv()._C().lpips_workspace_bytes(N, H, W)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = lv().layer_terms(last, crop, w)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert torch.equal(bits(out), ref)
    assert peak < ws + 2048 + x[0].numel() * 4, (peak, ws)                            # workspace and two small outputs: no image copy
    u8 = (x * 255).round().to(torch.uint8)
    hwc = u8.permute(0, 2, 3, 1).contiguous()                                        # (N,H,W,3) as PIL hands an image over
    assert torch.equal(bits(lv().layer_terms(hwc.permute(0, 3, 1, 2), y, w)), bits(lv().layer_terms(u8, y, w)))


def test_dropin_and_install():
    z = golden()
    w = weights()
    for name in ("batch3", "odd"):
        x, y, _, _ = pairs(name)
        v = lv().lpips(x, y, net_type="vgg", weights=w)
        ref = z[f"{name}/dropin64"].item()
        assert tuple(v.shape) == (1, 1, 1, 1) and v.dtype == torch.float32
        assert abs(v.item() - ref) <= 4 * float(z[f"{name}/gap_rel"]) * ref, (name, v.item(), ref)
    stub = types.ModuleType("lpipsPyTorch")
    stub.lpips = lambda *a, **k: None
    try:
        assert lv().install(stub, w) is stub and stub.lpips is lv().lpips
        x, y, _, _ = pairs("odd")
        assert torch.equal(bits(stub.lpips(x, y, net_type="vgg")), bits(lv().lpips(x, y, weights=w)))
    finally:
        lv().set_default_weights(None)
    with pytest.raises(ValueError, match="LpipsWeights"):
        lv().lpips(x, y, net_type="vgg")


def test_evaluate_views():
    import image_metrics
    w = weights()
    xa, ya, _, _ = pairs("batch3")
    xb, yb, _, _ = pairs("min16")
    renders = [xa[0], xb[0], xa[1], xa[2], xb[0][None]]
    gts = [ya[0], yb[0], ya[1], ya[2], yb[0][None]]
    each = [lv().lpips_views(r, g, w, quantize=True).item() for r, g in zip(renders, gts)]
    rep = lv().evaluate_views(renders, gts, w)
    assert sorted(rep) == ["LPIPS", "per_view"] and list(rep["per_view"]) == ["LPIPS"]
    assert rep["per_view"]["LPIPS"] == each and rep["LPIPS"] == torch.tensor(each).mean().item()
    same_size = [xa[0], xa[1], xa[2]], [ya[0], ya[1], ya[2]]
    one = lv()._C().lpips_workspace_bytes(1, 40, 48)
    split = lv().evaluate_views(*same_size, w, max_workspace_bytes=2 * one)          # a run of three in calls of two and one
    assert split["per_view"]["LPIPS"] == [each[0], each[2], each[3]]
    raw = lv().evaluate_views(renders, gts, w, quantize=False)
    assert raw["per_view"]["LPIPS"] == [lv().lpips_views(r, g, w).item() for r, g in zip(renders, gts)]
    today = image_metrics.evaluate_views(renders, gts)
    assert sorted(today) == ["L1", "PSNR", "SSIM", "per_view"] and sorted(today["per_view"]) == ["L1", "PSNR", "SSIM"]
    both = image_metrics.evaluate_views(renders, gts, lpips_weights=w)
    assert sorted(both) == ["L1", "LPIPS", "PSNR", "SSIM", "per_view"] and sorted(both["per_view"]) == ["L1", "LPIPS", "PSNR", "SSIM"]
    assert both["per_view"]["LPIPS"] == each and both["LPIPS"] == rep["LPIPS"]
    assert all(both[k] == today[k] and both["per_view"][k] == today["per_view"][k] for k in ("L1", "PSNR", "SSIM"))


def test_workspace_is_all_the_call_allocates():
    x, y, _, _ = pairs("mid")
    w = weights()
    N, _, H, W = x.shape
    ws = lv()._C().lpips_workspace_bytes(N, H, W)
    assert ws >= 2 * 2 * N * 64 * H * W * 4 and ws <= 2 * 2 * N * 64 * H * W * 4 + (1 << 20)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()                                           # the inputs and the weights
    out = lv().lpips_views(x, y, w)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= ws + out.numel() * 4 + N * 5 * 4 + (1 << 20)


# (id, the two sides, keyword arguments, whether evaluate_views refuses the pair as a view too)
REFUSALS = [
    ("below16", lambda t: (t(1, 3, 15, 40), t(1, 3, 15, 40)), {}, True),
    ("channels", lambda t: (t(1, 4, 32, 32), t(1, 4, 32, 32)), {}, True),
    ("shapes", lambda t: (t(1, 3, 32, 32), t(1, 3, 32, 40)), {}, True),
    ("batch_sizes", lambda t: (t(2, 3, 32, 32), t(1, 3, 32, 32)), {}, False),
    ("dtype", lambda t: (t(1, 3, 32, 32).half(), t(1, 3, 32, 32).half()), {}, True),
    ("quantize_u8", lambda t: (t(1, 3, 32, 32).to(torch.uint8), t(1, 3, 32, 32)), {"quantize": True}, False),
    ("cpu_side", lambda t: (t(1, 3, 32, 32), t(1, 3, 32, 32).cpu()), {}, True),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_before_any_device_work(case):
    _, make, kwargs, as_views = case
    exc = ValueError
    w = weights()
    x, y = make(lambda *s: torch.zeros(s, device=DEV))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    for call in (lv().lpips_views, lv().layer_terms):
        with pytest.raises(exc):
            call(x, y, w, **kwargs)
    with pytest.raises(NotImplementedError):
        lv().lpips(x, y, net_type="alex", weights=w)
    if as_views:
        with pytest.raises(exc):
            lv().evaluate_views([x[0]], [y[0]], w, **kwargs)
    assert torch.cuda.max_memory_allocated() == before
