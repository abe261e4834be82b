"""The image metrics on the GPU (feature-3dgs_amd/image_metrics.py, csrc/image_metrics.hip) against the fp64 oracle
(tests/image_metrics_oracle.py, itself held to the reference's own code on the CPU), the training forward's `fused_ssim`, and
the reference's fixture values; every input form on each side; determinism, graph capture and uninitialised scratch.

Bars.  l1, mse, ssim: 1e-6 + 1e-5 |want|, the bar tests/test_gpu_image_loss.py holds the training forward to.
psnr: 1e-4 dB wherever the oracle's mse is at least 1e-10, from
  - the kernel's mse: fp32 sums along a tree at most 14 additions deep (4 per thread, 6 shuffle steps, 2 across the waves; the
    rest is fp64), 14 x 2^-24 = 8.4e-7 relative, and 10 log10(1 + d) = 4.34 d dB: 3.6e-6 dB (a 1e-5 relative error of the mse, the
    most the mse bar admits for a large mse, would be 4.3e-5 dB);
  - the rounding of the mse to fp32, the fp32 sqrt and the fp32 division, each correctly rounded: 3 x 2^-24 relative in the
    argument of 20 log10, 8.69 dB per unit: 1.6e-6 dB;
  - the fp32 log10, taken as 2 ulp of a result below 5 (mse >= 1e-10), times 20: 1.9e-5 dB, and the rounding of the product,
    half an ulp of a value below 128: 3.8e-6 dB;
2.8e-5 dB in all.  Below an mse of 1e-10 psnr exceeds 100 dB and only l1, mse and ssim are judged."""
import ctypes
import itertools
import math
import os
import types

import numpy as np
import pytest
import torch

import image_loss_oracle as LO
import image_metrics_oracle as O
from util import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_image_metrics.npz")
DEV = "cuda:0"
FORMS = ("f32", "f32q", "u8p", "u8i")

# (H, W): smaller than the halo; below and exactly the window; one tile; one pixel past and one short of a tile on each axis;
# several tiles with ragged edges.  Each with two of the six (N, C) pairs of N in {1, 3}, C in {1, 3, 4}.
SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 4)), ((5, 5), (3, 3)), ((5, 5), (1, 4)), ((11, 11), (1, 3)), ((11, 11), (3, 1)),
          ((16, 64), (3, 3)), ((16, 64), (1, 1)), ((17, 65), (3, 4)), ((17, 65), (1, 3)), ((15, 63), (3, 1)), ((15, 63), (1, 4)),
          ((37, 53), (3, 3)), ((37, 53), (1, 1)), ((33, 129), (3, 4)), ((33, 129), (1, 3))]


def _views(N, C, H, W, seed):
    """fp32 views on the CPU whose images differ in content and in error level; a few values leave [0, 1]"""
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(N, C, H, W, generator=g)
    noise = torch.randn(N, C, H, W, generator=g) * (0.05 + 0.1 * torch.arange(N, dtype=torch.float32)).view(N, 1, 1, 1)
    return gt + noise, gt * 1.02 - 0.01


def _torch_bytes(t):
    """the uint8 tensor torch's own chain (torchvision's save_image) makes of a float tensor"""
    return t.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def _form(t, form):
    """(device tensor, quantize, channels_last) of a CPU fp32 (N,C,H,W) tensor in one input form"""
    if form == "f32":
        return t.to(DEV), False, False
    if form == "f32q":
        return t.to(DEV), True, False
    if form == "u8p":
        return _torch_bytes(t).to(DEV), False, False
    return _torch_bytes(t).permute(0, 2, 3, 1).contiguous().to(DEV), False, True


def _call(img, fi, gt, fg):
    from image_metrics import image_metrics
    x, qx, cx = _form(img, fi)
    y, qy, cy = _form(gt, fg)
    return image_metrics(x, y, quantize=(qx, qy), channels_last=(cx, cy))


def _check(got, want, what):
    """got: ImageMetrics on the device; want: the oracle's dict of fp64 (N,) tensors"""
    for k in ("l1", "mse", "ssim"):
        g, w = getattr(got, k).double().cpu(), want[k]
        assert g.shape == w.shape, (what, k, g.shape)
        err, bar = (g - w).abs(), 1e-6 + 1e-5 * w.abs()
        assert bool((err <= bar).all()), (what, k, g.tolist(), w.tolist())
    g, w = got.psnr.double().cpu(), want["psnr"]
    judged = want["mse"] >= 1e-10
    assert bool(((g - w).abs()[judged] <= 1e-4).all()), (what, "psnr", g.tolist(), w.tolist())
    assert bool((g[want["mse"] == 0] == math.inf).all())


def _same_bits(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("l1", "mse", "psnr", "ssim"))


@pytest.mark.parametrize("hw,nc", SHAPES, ids=[f"{h}x{w}_n{n}c{c}" for (h, w), (n, c) in SHAPES])
def test_every_input_form_against_the_oracle(hw, nc):
    """All sixteen pairs of input forms.  A side holds one of two sets of values - the floats as they are, or the 8-bit image
    torch's chain makes of them (quantised float, uint8 planar, uint8 interleaved) -, so four oracle results judge the sixteen
    calls, and the calls that share their values must agree bit for bit: in particular a quantised float input and the uint8
    tensor torch makes of it."""
    from image_loss import fused_ssim
    (H, W), (N, C) = hw, nc
    img, gt = _views(N, C, H, W, seed=1000 * H + W + 7 * N + C)
    first = {}
    for fi, fg in itertools.product(FORMS, FORMS):
        key = (fi != "f32", fg != "f32")
        got = _call(img, fi, gt, fg)
        assert all(getattr(got, k).shape == (N,) and getattr(got, k).dtype == torch.float32 for k in got._fields)
        if key not in first:
            want = O.metrics(img if fi == "f32" else _torch_bytes(img), gt if fg == "f32" else _torch_bytes(gt))
            _check(got, want, (fi, fg))
            first[key] = got
        else:
            assert _same_bits(got, first[key]), (fi, fg)
    # the training forward on the same floats
    s = fused_ssim(img.to(DEV), gt.to(DEV), size_average=False).double()
    mine = first[(False, False)].ssim.double()
    assert bool(((mine - s).abs() <= 1e-6 + 1e-5 * s.abs()).all()), (mine.tolist(), s.tolist())
    if N == 3:          # different images, different results: a per-image mix-up would show
        v = first[(False, False)].mse.tolist()
        assert len({round(a, 6) for a in v}) == 3


def test_equal_values_give_equal_bits_across_forms():
    """Every byte 0 .. 255 on both sides: the uint8 tensor, its quantised float image and the UNquantised float tensor that
    holds exactly torch's v / 255 are the same values, so all forms agree bit for bit - the kernel's division-free v / 255 is the
    fp32 quotient for every byte."""
    from image_metrics import image_metrics
    g = torch.Generator().manual_seed(3)
    a8 = torch.arange(256, dtype=torch.uint8)[torch.randperm(256, generator=g)].view(1, 1, 16, 16).repeat(1, 2, 1, 1)
    b8 = torch.arange(256, dtype=torch.uint8)[torch.randperm(256, generator=g)].view(1, 1, 16, 16).repeat(1, 2, 1, 1)
    b8[0, 1] = b8[0, 1].flip(0)
    af, bf = a8.float().div(255), b8.float().div(255)
    ref = image_metrics(a8.to(DEV), b8.to(DEV))
    _check(ref, O.metrics(a8, b8), "bytes")
    sides_a = [(a8.to(DEV), False, False), (a8.permute(0, 2, 3, 1).contiguous().to(DEV), False, True), (af.to(DEV), False, False),
               (af.to(DEV), True, False)]
    sides_b = [(b8.to(DEV), False, False), (b8.permute(0, 2, 3, 1).contiguous().to(DEV), False, True), (bf.to(DEV), False, False),
               (bf.to(DEV), True, False)]
    for (x, qx, cx), (y, qy, cy) in itertools.product(sides_a, sides_b):
        assert _same_bits(image_metrics(x, y, quantize=(qx, qy), channels_last=(cx, cy)), ref), (x.dtype, qx, cx, y.dtype, qy, cy)


def test_unaligned_planes_take_the_element_path():
    """W % 4 == 0 but planes that start off a 16-byte (float) or 4-byte (uint8) boundary: the same bits as the aligned call."""
    from image_metrics import image_metrics
    img, gt = _views(2, 3, 20, 68, seed=5)
    want = image_metrics(img.to(DEV), gt.to(DEV), quantize=(False, True))
    flat = torch.empty(img.numel() + 1, device=DEV)
    flat[1:] = img.to(DEV).reshape(-1)
    shifted = flat[1:].view(img.shape)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert _same_bits(image_metrics(shifted, gt.to(DEV), quantize=(False, True)), want)
    i8 = _torch_bytes(img)
    want8 = image_metrics(i8.to(DEV), gt.to(DEV))
    flat8 = torch.empty(i8.numel() + 1, dtype=torch.uint8, device=DEV)
    flat8[1:] = i8.to(DEV).reshape(-1)
    shifted8 = flat8[1:].view(i8.shape)
    assert shifted8.data_ptr() % 4 == 1
    assert _same_bits(image_metrics(shifted8, gt.to(DEV)), want8)
    _check(want8, O.metrics(i8, gt), "u8 planar")


def test_identical_images():
    from image_metrics import image_metrics
    img, _ = _views(2, 3, 21, 70, seed=6)
    for form in FORMS:
        got = _call(img, form, img, form)
        assert got.l1.tolist() == [0.0, 0.0] and got.mse.tolist() == [0.0, 0.0], form
        assert got.psnr.tolist() == [math.inf, math.inf], form
        assert bool(((got.ssim - 1).abs() <= 1e-6).all()), (form, got.ssim.tolist())


def test_constant_images_have_a_closed_form():
    """x = a, y = b everywhere: with m the window's mass inside the image at a pixel (zero padding), mu1 = a m, mu2 = b m and
    every (co)variance is the product of the constants times m (1 - m), so
    S = (2 a b m^2 + C1)(2 a b m (1 - m) + C2) / (((a^2 + b^2) m^2 + C1)((a^2 + b^2) m (1 - m) + C2));
    l1 = |a - b|, mse = (a - b)^2, psnr = -20 log10 |a - b|.
    a and b are powers of two: every product with a window weight is then exact and the kernel's moments are the constants times
    its fp32 window mass, which the bars allow for ((a - b)^2 / C2 = 4.3 times the 1e-7 by which two fp32 sums of the weights may
    differ).  Other constants would measure the conditioning of ANY fp32 SSIM on an image without variance - (co)variances that
    are pure rounding, 1e-8, beside C2 = 9e-4 - and not this kernel."""
    from image_metrics import image_metrics
    a, b, shape = 0.125, 0.0625, (1, 3, 20, 70)
    m = LO.stencil(torch.ones(shape, dtype=torch.float64), LO.window2d())
    p, s = a * b, a * a + b * b
    S = (2 * p * m * m + LO.C1) * (2 * p * m * (1 - m) + LO.C2) / ((s * m * m + LO.C1) * (s * m * (1 - m) + LO.C2))
    want = dict(l1=torch.tensor([abs(a - b)], dtype=torch.float64), mse=torch.tensor([(a - b) ** 2], dtype=torch.float64),
                psnr=torch.tensor([-20 * math.log10(abs(a - b))], dtype=torch.float64), ssim=S.mean(dim=(1, 2, 3)))
    _check(image_metrics(torch.full(shape, a, device=DEV), torch.full(shape, b, device=DEV)), want, "constants")


def _z():
    return np.load(GOLDEN)


def _fixture_want(z, name):
    want = {k: torch.from_numpy(z[f"{name}/{k}"]).double() for k in ("l1", "mse", "ssim")}
    want["psnr"] = torch.from_numpy(z[f"{name}/psnr_fp32"]).double()
    return want


def test_nan_and_the_other_edge_values_as_the_fixture_pins_them():
    """The render of this case holds NaN, infinities, negatives, values above 1 and exact halves; the fixture pins what torch's
    chain makes of them on the CPU and what the reference then reports."""
    from image_metrics import image_metrics
    z = _z()
    img, gt = torch.from_numpy(z["special/image"]), torch.from_numpy(z["special/gt"])
    assert torch.isnan(img).any()
    got = image_metrics(img.to(DEV), gt.to(DEV), quantize=(True, False))
    _check(got, _fixture_want(z, "special"), "special")
    pinned = torch.from_numpy(z["special/image_u8"]).to(DEV)                 # (1,H,W,1), NaN -> z["nan_byte"]
    assert _same_bits(image_metrics(pinned, gt.to(DEV), channels_last=(True, False)), got)


def test_fixture_values_through_psnr_ssim_and_evaluate_views():
    import image_metrics as M
    z = _z()
    # psnr, the drop-in: (N, 1), and one value per channel of an unbatched image
    img, gt = torch.from_numpy(z["float/image"]).to(DEV), torch.from_numpy(z["float/gt"]).to(DEV)
    image_utils, loss_utils = types.ModuleType("utils.image_utils"), types.ModuleType("utils.loss_utils")
    image_utils.psnr, loss_utils.ssim = None, None
    M.install(image_utils)
    M.install(loss_utils)
    p = image_utils.psnr(img, gt)
    assert p.shape == (3, 1) and bool(((p[:, 0].double().cpu() - torch.from_numpy(z["float/psnr_fp32"]).double()).abs() <= 1e-4).all())
    p = image_utils.psnr(img[0], gt[0])
    assert p.shape == (3, 1) and bool(((p[:, 0].double().cpu() - torch.from_numpy(z["float/psnr_chw_fp32"]).double()).abs() <= 1e-4).all())
    # ssim, installed: the mean, and one value per image
    want = torch.from_numpy(z["float/ssim"])
    s = loss_utils.ssim(img, gt, size_average=False).double().cpu()
    assert s.shape == (3,) and bool(((s - want).abs() <= 1e-6 + 1e-5 * want.abs()).all())
    for i in range(3):
        s = loss_utils.ssim(img[i:i + 1], gt[i:i + 1])
        assert s.dim() == 0 and abs(float(s) - float(want[i])) <= 1e-6 + 1e-5 * abs(float(want[i]))
    s = loss_utils.ssim(img[0], gt[0])                      # unbatched, as training_report has it
    assert abs(float(s) - float(want[0])) <= 1e-6 + 1e-5 * abs(float(want[0]))
    _check(M.image_metrics(img, gt), _fixture_want(z, "float"), "float")
    # evaluate_views: metrics.py's views - float renders that went through a PNG - beside views of another size and uint8 ones
    pi, pg = torch.from_numpy(z["png/image"]), torch.from_numpy(z["png/gt"])
    fi, fg = torch.from_numpy(z["float/image"]), torch.from_numpy(z["float/gt"])
    renders = [pi[0].to(DEV), pi[1].to(DEV), fi[0].to(DEV), fi[1].to(DEV), pi[0].to(DEV)]
    gts = [pg[0].to(DEV), pg[1].to(DEV), fg[0].to(DEV), fg[1].to(DEV), pg[0].to(DEV)]
    rep = M.evaluate_views(renders, gts)                    # quantize=True
    png, flt = _fixture_want(z, "png"), O.metrics(fi[:2], fg[:2], quantize=(True, True))
    order = [(png, 0), (png, 1), (flt, 0), (flt, 1), (png, 0)]
    for name, k in (("SSIM", "ssim"), ("PSNR", "psnr"), ("L1", "l1")):
        want = [float(src[k][i]) for src, i in order]
        bar = (lambda w: 1e-4) if k == "psnr" else (lambda w: 1e-6 + 1e-5 * abs(w))
        assert len(rep["per_view"][name]) == 5
        for g, w in zip(rep["per_view"][name], want):
            assert abs(g - w) <= bar(w), (name, g, w)
        assert rep[name] == torch.tensor(rep["per_view"][name]).mean().item()           # metrics.py:81-83
        assert abs(rep[name] - sum(want) / 5) <= bar(sum(want) / 5) + 1e-6
    # the decoded PNG bytes as PIL hands them over
    i8, g8 = torch.from_numpy(z["png/image_u8"]).to(DEV), torch.from_numpy(z["png/gt_u8"]).to(DEV)
    rep8 = M.evaluate_views([i8[0], i8[1]], [g8[0], g8[1]], channels_last=True)
    assert rep8["per_view"]["SSIM"] == rep["per_view"]["SSIM"][:2] and rep8["per_view"]["PSNR"] == rep["per_view"]["PSNR"][:2]
    assert rep8["per_view"]["L1"] == rep["per_view"]["L1"][:2]


def test_argument_errors_on_device_tensors():
    from image_metrics import image_metrics
    a, b = torch.rand(2, 3, 8, 9, device=DEV), torch.rand(2, 3, 8, 9, device=DEV)
    with pytest.raises(ValueError, match="shapes differ"):
        image_metrics(a, b[:, :2])
    with pytest.raises(ValueError, match="float32 or uint8"):
        image_metrics(a.half(), b.half())
    with pytest.raises(ValueError, match="quantize applies"):
        image_metrics((a * 255).to(torch.uint8), b, quantize=True)
    with pytest.raises(ValueError, match="HIP device"):
        image_metrics(a, b.cpu())
    empty = image_metrics(a[:0], b[:0])                     # N = 0: a no-op
    assert all(t.shape == (0,) for t in empty)
    # a strided view is read through a contiguous copy
    wide = torch.zeros(2, 3, 8, 18, device=DEV)
    wide[..., ::2] = a
    assert _same_bits(image_metrics(wide[..., ::2], b), image_metrics(a, b))


def test_two_calls_and_a_graph_replay_give_the_same_bits():
    from image_metrics import image_metrics
    img, gt = _views(3, 3, 37, 131, seed=8)
    x, y = img.to(DEV), _torch_bytes(gt).to(DEV)
    a = image_metrics(x, y, quantize=(True, False))
    b = image_metrics(x, y, quantize=(True, False))
    assert _same_bits(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream, no parallel branches
        c = image_metrics(x, y, quantize=(True, False))
    for t in c:
        t.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(c, a)
    x.copy_(torch.flip(x, dims=(0,)))                       # new content behind the same pointers
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(c, image_metrics(x, y, quantize=(True, False))) and not torch.equal(c.mse, a.mse)


def test_scratch_needs_no_clearing_and_outputs_are_optional():
    """The C ABI on device pointers: a scratch buffer pre-filled with 0xFF gives the bits of one pre-filled with zeros and of the
    Python call (no partial sum is accumulated into what the buffer held); NULL outputs are left out."""
    from image_metrics import image_metrics
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_image_metrics_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_image_metrics_scratch_bytes.argtypes = [ctypes.c_int] * 4
    lib.f3dgs_image_metrics.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + \
        [ctypes.c_void_p] * 6
    N, C, H, W = 3, 3, 33, 129
    img, gt = _views(N, C, H, W, seed=9)
    x, y = img.to(DEV), _torch_bytes(gt).permute(0, 2, 3, 1).contiguous().to(DEV)
    want = image_metrics(x, y, quantize=(True, False), channels_last=(False, True))
    nbytes = lib.f3dgs_image_metrics_scratch_bytes(N, C, H, W)
    assert nbytes >= 3 * 4 * N * C * 3 * 3
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for fill in (0xFF, 0x00):
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        out = torch.full((4, N), -1.0, device=DEV)
        rc = lib.f3dgs_image_metrics(N, C, H, W, x.data_ptr(), 0, y.data_ptr(), 2, 1, out[0].data_ptr(), out[1].data_ptr(),
                                     out[2].data_ptr(), out[3].data_ptr(), scratch.data_ptr(), stream)
        assert rc == 0
        torch.cuda.synchronize()
        results.append(out)
    assert torch.equal(results[0], results[1])
    for row, k in enumerate(("l1", "mse", "psnr", "ssim")):
        assert torch.equal(results[0][row], getattr(want, k)), k
    # psnr alone: the other outputs NULL, the windowed moments skipped
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((N,), -1.0, device=DEV)
    assert lib.f3dgs_image_metrics(N, C, H, W, x.data_ptr(), 0, y.data_ptr(), 2, 1, None, None, out.data_ptr(), None, scratch.data_ptr(),
                                   stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want.psnr)
