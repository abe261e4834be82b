"""The fused L1 + D-SSIM image loss on the GPU (feature-3dgs_amd/image_loss.py, csrc/image_loss.hip) against the fp64
oracle (tests/image_loss_oracle.py, itself checked against the reference's own code on CPU), the reference's fp32 torch ops,
and inside a rasterizer step, eager and replayed from a graph."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_loss_oracle as O
from util import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_ssim.npz")
DEV = "cuda:0"
LAM = 0.2


def _fixture_cases():
    z = np.load(GOLDEN)
    return sorted({k.split("/")[0] for k in z.files if "/" in k})


def _random(shape, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    img = (gt + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    return img.to(DEV), gt.to(DEV)


def _torch_ops(img, gt, lam=LAM):
    """The reference's loss (utils/loss_utils.py) restated in fp32 torch ops, with its fp32 window."""
    C = img.shape[-3]
    w = O.window2d(img.device).to(torch.float32).expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=C)
    mu1, mu2 = conv(img), conv(gt)
    s1, s2, s12 = conv(img * img) - mu1 ** 2, conv(gt * gt) - mu2 ** 2, conv(img * gt) - mu1 * mu2
    S = ((2 * mu1 * mu2 + O.C1) * (2 * s12 + O.C2)) / ((mu1 ** 2 + mu2 ** 2 + O.C1) * (s1 + s2 + O.C2))
    return (1 - lam) * (img - gt).abs().mean() + lam * (1 - S.mean())


def _fused(img, gt, upstream=1.0):
    from image_loss import fused_l1_dssim
    x = img.clone().requires_grad_(True)
    loss, l1, ssim = fused_l1_dssim(x, gt, LAM, return_parts=True)
    (upstream * loss).backward()
    return loss.detach(), l1, ssim, x.grad


def _close_scalar(got, want, what):
    got = float(got.detach()) if torch.is_tensor(got) else float(got)
    want = float(want)
    assert abs(got - want) <= 1e-6 + 1e-5 * abs(want), (what, got, want)


def _grad_bar(got, want, what, floor=0.0):
    """every element within 1e-3 |g| + 1e-5 max|g| of the oracle (floor: a lower bound of max|g| where the gradient vanishes)"""
    got, want = got.double(), want.double()
    scale = max(float(want.abs().max()), floor)
    bound = 1e-3 * want.abs() + 1e-5 * scale
    worst = float(((got - want).abs() / bound).max())
    assert worst <= 1.0, (what, worst)


@pytest.mark.parametrize("name", _fixture_cases())
def test_fixture_cases_against_the_oracle(name):
    z = np.load(GOLDEN)
    img, gt = torch.from_numpy(z[f"{name}/image"]).to(DEV), torch.from_numpy(z[f"{name}/gt"]).to(DEV)
    n = img.numel()
    loss, l1, ssim, grad = _fused(img, gt)
    _close_scalar(loss, z[f"{name}/loss"], "loss")
    _close_scalar(l1, z[f"{name}/l1"], "l1")
    _close_scalar(ssim, z[f"{name}/ssim"], "ssim")
    _grad_bar(grad, torch.from_numpy(z[f"{name}/grad_loss"]).to(DEV), "grad_loss", floor=1.0 / n)
    from image_loss import fused_ssim
    x = img.clone().requires_grad_(True)
    s = fused_ssim(x, gt)
    s.backward()
    ref = O.image_loss(img.double(), gt.double(), LAM)
    _close_scalar(s, z[f"{name}/ssim"], "fused_ssim")
    _grad_bar(x.grad, ref["grad_ssim"], "grad_ssim", floor=1.0 / n)
    if f"{name}/ssim_per_image" in z.files:
        u = torch.tensor(z["upstream_per_image"], dtype=torch.float32, device=DEV)
        x = img.clone().requires_grad_(True)
        v = fused_ssim(x, gt, size_average=False)
        assert v.shape == (img.shape[0],)
        for a, b in zip(v.tolist(), z[f"{name}/ssim_per_image"]):
            _close_scalar(a, b, "ssim_per_image")
        (v * u).sum().backward()
        _grad_bar(x.grad, torch.from_numpy(z[f"{name}/grad_ssim_per_image"]).to(DEV), "grad_ssim_per_image", floor=1.0 / n)


@pytest.mark.parametrize("shape", [(3, 256, 256), (1, 3, 256, 256), (3, 1080, 1920), (2, 4, 67, 131)])
def test_random_images_against_the_oracle_and_the_torch_ops(shape):
    img, gt = _random(shape, 11)
    loss, l1, ssim, grad = _fused(img, gt)
    ref = O.image_loss(img, gt, LAM)
    _close_scalar(loss, ref["loss"], "loss")
    _close_scalar(l1, ref["l1"], "l1")
    _close_scalar(ssim, ref["ssim"], "ssim")
    _grad_bar(grad, ref["grad_loss"], "grad_loss")
    # no worse than the reference's own fp32 ops against the same fp64 oracle
    x = img.clone().requires_grad_(True)
    _torch_ops(x, gt).backward()
    err_fused = float((grad.double() - ref["grad_loss"]).abs().max())
    err_torch = float((x.grad.double() - ref["grad_loss"]).abs().max())
    assert err_fused <= 2 * err_torch + 1e-6 * float(ref["grad_loss"].abs().max()), (err_fused, err_torch)


# (H, W) at the window's and the tile's edges: smaller than the 5-pixel halo, the 11-tap window exactly, the 64 x 16 tile exactly,
# one more and one fewer in both directions, odd sizes inside one tile column and across three.  Two (N, C) per shape; together
# every pair of N in {1, 3} and C in {1, 3, 4} occurs.
_EDGE_CASES = [(1, 1, (1, 1)), (1, 1, (3, 4)), (5, 5, (1, 3)), (5, 5, (3, 1)), (11, 11, (1, 4)), (11, 11, (3, 3)),
               (16, 64, (1, 1)), (16, 64, (3, 4)), (17, 65, (1, 3)), (17, 65, (3, 1)), (15, 63, (1, 4)), (15, 63, (3, 3)),
               (37, 53, (1, 1)), (37, 53, (3, 4)), (33, 129, (1, 3)), (33, 129, (3, 1))]


@pytest.mark.parametrize("H,W,nc", _EDGE_CASES, ids=[f"{h}x{w}-n{nc[0]}c{nc[1]}" for h, w, nc in _EDGE_CASES])
def test_tile_and_window_edges_against_the_oracle(H, W, nc):
    img, gt = _random((nc[0], nc[1], H, W), 100 * H + W)
    loss, l1, ssim, grad = _fused(img, gt)
    ref = O.image_loss(img, gt, LAM)
    _close_scalar(loss, ref["loss"], "loss")
    _close_scalar(l1, ref["l1"], "l1")
    _close_scalar(ssim, ref["ssim"], "ssim")
    _grad_bar(grad, ref["grad_loss"], "grad_loss", floor=1.0 / img.numel())


def test_unaligned_planes_take_the_element_path():
    """W % 4 == 0 but an image and a ground truth whose planes start 4 bytes off a 16-byte boundary: the same bits as the
    aligned call, which stages with float4 loads."""
    from image_loss import fused_l1_dssim
    img, gt = _random((2, 3, 20, 68), 18)
    want = _fused(img, gt)

    def shifted(t):
        flat = torch.empty(t.numel() + 1, device=DEV)
        flat[1:] = t.reshape(-1)
        s = flat[1:].view(t.shape)
        assert s.data_ptr() % 16 == 4 and s.is_contiguous()
        return s
    x = shifted(img).requires_grad_(True)
    loss, l1, ssim = fused_l1_dssim(x, shifted(gt), LAM, return_parts=True)
    loss.backward()
    assert x.data_ptr() % 16 == 4
    for got, w, what in zip((loss.detach(), l1, ssim, x.grad), want, ("loss", "l1", "ssim", "grad")):
        assert torch.equal(got, w), what


def test_upstream_gradient_scales_the_result():
    img, gt = _random((3, 96, 80), 12)
    _l, _a, _b, g1 = _fused(img, gt)
    _l, _a, _b, g25 = _fused(img, gt, upstream=2.5)
    assert torch.allclose(g25, 2.5 * g1, rtol=1e-6, atol=0)


def test_two_calls_are_bit_identical_and_no_grad_gives_the_same_loss():
    from image_loss import fused_l1_dssim
    img, gt = _random((3, 300, 420), 13)
    a, b = _fused(img, gt), _fused(img, gt)
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    with torch.no_grad():
        c = fused_l1_dssim(img.clone().requires_grad_(True), gt)
    assert c.grad_fn is None and torch.equal(c, a[0])
    d = fused_l1_dssim(img, gt)             # no gradient asked for: the same value, no graph
    assert d.grad_fn is None and torch.equal(d, a[0])


def test_identical_images():
    img, _ = _random((1, 3, 64, 48), 14)
    loss, l1, ssim, grad = _fused(img, img.clone())
    assert abs(float(ssim) - 1.0) <= 1e-6 and float(l1) == 0.0
    # sign(0) = 0: no L1 term; what is left is the SSIM term at its maximum, zero up to rounding
    assert float(grad.abs().max()) <= 1e-4 / img.numel()


def test_non_contiguous_input():
    img, gt = _random((3, 64, 96), 15)
    nc_img = img.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not nc_img.is_contiguous()
    from image_loss import fused_l1_dssim
    x = nc_img.clone(memory_format=torch.preserve_format).requires_grad_(True)
    loss = fused_l1_dssim(x, gt[:, :, :])
    loss.backward()
    want = _fused(img, gt)
    assert torch.equal(loss.detach(), want[0]) and torch.equal(x.grad.contiguous(), want[3])
    # a strided ground truth
    gt_wide = torch.zeros(3, 64, 192, device=DEV)
    gt_wide[:, :, ::2] = gt
    assert torch.equal(fused_l1_dssim(img, gt_wide[:, :, ::2]), want[0])


def test_bad_inputs_raise_named_errors():
    from image_loss import fused_l1_dssim, fused_ssim
    img, gt = _random((3, 32, 32), 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        fused_l1_dssim(img.cpu(), gt)
    with pytest.raises(RuntimeError, match="shapes differ"):
        fused_l1_dssim(img, gt[:, :, :31])
    with pytest.raises(RuntimeError, match="float32"):
        fused_l1_dssim(img.half(), gt.half())
    with pytest.raises(RuntimeError, match="dimensions"):
        fused_l1_dssim(img[0], gt[0])
    with pytest.raises(ValueError, match="ground-truth"):
        fused_l1_dssim(img, gt.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="window_size"):
        fused_ssim(img, gt, window_size=9)


def test_4k_on_sampled_pixels():
    img, gt = _random((3, 2160, 3840), 17)
    loss, l1, ssim, grad = _fused(img, gt)
    # the loss over the whole image: the fp64 oracle of the moments runs on the device
    ref = O.image_loss(img, gt, LAM)
    _close_scalar(loss, ref["loss"], "loss")
    _close_scalar(ssim, ref["ssim"], "ssim")
    n = img.numel()
    # gradients on a strided sample of pixels (every 7th row, every 13th column: every tile position and both image edges)
    want = ref["grad_loss"][:, ::7, ::13]
    got = grad[:, ::7, ::13]
    bound = 1e-3 * want.abs() + 1e-5 * float(ref["grad_loss"].abs().max())
    assert float(((got.double() - want).abs() / bound).max()) <= 1.0
    assert n == 3 * 2160 * 3840
    del ref


# ---- end to end: the rasterizer's parameter gradients through the fused loss -------------------------------------------

def _render_step(scene, loss_fn):
    """A forward + backward of the rasterizer on static tensors with `loss_fn(color)` as the loss: (fn, grads, outs)."""
    import diff_gaussian_rasterization as dgr
    t = lambda x: x.to(DEV)
    P = scene["means3D"].shape[0]
    settings = dgr.GaussianRasterizationSettings(
        image_height=scene["image_height"], image_width=scene["image_width"], tanfovx=scene["tanfovx"],
        tanfovy=scene["tanfovy"], bg=t(scene["bg"]), scale_modifier=scene["scale_modifier"],
        viewmatrix=t(scene["viewmatrix"]), projmatrix=t(scene["projmatrix"]), sh_degree=scene["sh_degree"],
        campos=t(scene["campos"]), prefiltered=False, debug=False)
    names = ("means3D", "opacities", "semantic_feature", "shs", "scales", "rotations")
    L = {k: t(scene[k]).clone().requires_grad_(True) for k in names}
    L["means2D"] = torch.zeros(P, 3, device=DEV, requires_grad=True)
    rast = dgr.GaussianRasterizer(settings)
    grads = {k: torch.zeros_like(v) for k, v in L.items()}
    outs = {}

    def fn():
        color, _feat, _radii, _depth = rast(**L)
        loss = loss_fn(color)
        keys = [k for k in grads]
        gs = torch.autograd.grad(loss, [L[k] for k in keys] + [color], allow_unused=True)
        for k, g in zip(keys, gs):
            if g is not None and g.numel():
                grads[k].copy_(g)
        outs["loss"] = loss.detach()
        outs["d_color"] = gs[-1]
        return outs["loss"]
    return fn, grads, outs


def _scene():
    from synth import make_scene
    return make_scene(P=4000, C=8, width=160, height=96, seed=5, scale_lo=0.01, scale_hi=0.1)


def _target(scene):
    g = torch.Generator().manual_seed(3)
    return torch.rand(3, scene["image_height"], scene["image_width"], generator=g).to(DEV)


def _snap(grads):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().double().clone() for k, v in grads.items()}


def _param_bar(got, want, what):
    for k, v in want.items():
        if v.numel() == 0:
            continue
        bound = 1e-3 * v.abs() + 1e-5 * float(v.abs().max())
        worst = float(((got[k] - v).abs() / (bound + 1e-30)).max())
        assert worst <= 1.0, (what, k, worst)


def test_rasterizer_gradients_through_the_fused_loss(option):
    from image_loss import fused_l1_dssim
    option("bwd_bf16", 0)           # exact fp32 contraction: the two losses' image gradients meet the same backward
    scene = _scene()
    gt = _target(scene)
    fn_f, g_f, o_f = _render_step(scene, lambda c: fused_l1_dssim(c, gt, LAM))
    fn_t, g_t, o_t = _render_step(scene, lambda c: _torch_ops(c, gt))
    fn_f()
    got = _snap(g_f)
    fn_t()
    want = _snap(g_t)
    _close_scalar(o_f["loss"], o_t["loss"], "loss")
    _param_bar(got, want, "fused vs torch ops")


def test_captured_step_replays_the_eager_step(option):
    from graph_step import CapturedStep
    from image_loss import fused_l1_dssim
    option("bwd_bf16", 1)
    scene = _scene()
    gt = _target(scene)
    fn, grads, outs = _render_step(scene, lambda c: fused_l1_dssim(c, gt, LAM))
    fn()
    loss_eager, dcol_eager = outs["loss"].clone(), outs["d_color"].clone()
    want = _snap(grads)
    step = CapturedStep(fn).capture()
    graph_outs = dict(outs)
    for v in grads.values():
        v.zero_()
    for _ in range(2):
        step.replay()
    assert step.check()
    got = _snap(grads)
    assert torch.equal(graph_outs["loss"], loss_eager)
    assert torch.equal(graph_outs["d_color"], dcol_eager)
    _param_bar(got, want, "replay")
