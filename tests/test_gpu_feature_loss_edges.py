"""The fused feature-map loss and decode (csrc/feature_loss.hip) at every tile, list and store-path edge of its kernels, against
the float64 chain of oracle/feature_loss_oracle.py.  The cases (tests/feature_loss_cases.py) carry a margin ground truth - every
residual is at least 0.2 from zero - so no L1 sign can differ between fp32 and float64 and the gradients are compared with the
bounds of tests/test_feature_loss.py WITHOUT its slack for sign flips: loss within 2e-6 max(1, loss), every gradient within
1e-5 of the reference gradient's largest magnitude.  Exact zeros of the residual (gradient 0, as torch.abs) are pinned on inputs
on which fp32 arithmetic is exact."""
import numpy as np
import pytest
import torch

import feature_loss_cases as flc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UP = 2.5            # the upstream gradient of the sweeps


def _poison_free_blocks(fm, gt, w):
    """The call's scratch (resized map, g_x, sign bytes padded to 64 pixels per row) is a torch.empty: leave the allocator's
    free blocks of that size full of 0x7f bytes, so that a pad byte or a row that is read without having been written is a
    large number and not, by luck, the zero of a fresh allocation."""
    import ctypes
    import os
    from util import ROOT
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_feature_l1_scratch_bytes.restype = ctypes.c_size_t
    n = lib.f3dgs_feature_l1_scratch_bytes(fm.shape[0], gt.shape[0], gt.shape[1], gt.shape[2], 0 if w is None else 1)
    junk = [torch.full((n,), 0x7f, dtype=torch.uint8, device=DEV) for _ in range(6)]
    torch.cuda.synchronize()
    del junk


def _run_loss(fm, gt, w, b, up):
    from feature_loss import fused_feature_l1
    _poison_free_blocks(fm, gt, w)
    fm_d = fm.to(DEV).requires_grad_(True)
    w_d = w.to(DEV).reshape(w.shape[0], w.shape[1], 1, 1).requires_grad_(True) if w is not None else None      # nn.Conv2d's weight shape
    b_d = b.to(DEV).requires_grad_(True) if b is not None else None
    loss = fused_feature_l1(fm_d, gt.to(DEV), w_d, b_d)
    (up * loss).backward()
    torch.cuda.synchronize()
    return (loss.detach().cpu(), fm_d.grad.cpu(), None if w is None else w_d.grad.cpu().reshape(w.shape), None if b is None else b_d.grad.cpu())


@pytest.mark.parametrize("case", flc.LOSS_CASES, ids=flc.case_id)
def test_loss_and_gradients_match_float64_without_slack(case):
    c = flc.build_case(case)
    want = c["want"]
    loss, g_fm, g_w, g_b = _run_loss(c["fm"], c["gt"], c["w"], c["b"], UP)
    figs = {"loss": abs(float(loss) - float(want["loss"])) / max(1.0, float(want["loss"]))}
    pairs = [("d_feature_map", g_fm, want["d_feature_map"])]
    if c["w"] is not None:
        pairs += [("d_weight", g_w, want["d_weight"]), ("d_bias", g_b, want["d_bias"])]
    for name, got, ref in pairs:
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), name
        scale = float(ref.abs().max())
        assert scale > 0, name
        figs[name] = float((got.double() / UP - ref).abs().max()) / scale
    print(flc.case_id(case), " ".join(f"{k}={v:.3g}" for k, v in figs.items()))
    assert figs.pop("loss") <= 2e-6
    for name, v in figs.items():
        assert v <= 1e-5, (name, v)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", flc.DECODE_CASES, ids=flc.case_id)
def test_decode_matches_float64(case, half):
    """Forward only: F.interpolate(bilinear, align_corners=True) -> conv2d in float64 (the `decoded` map of the shared case);
    fp32 output to 1e-5 of the map's scale, fp16 output to one half-ulp of the float64 value on top of 2e-5 of the scale."""
    from feature_loss import fused_feature_decode
    c = flc.build_case(case)
    C, H, W, Cout, Hg, Wg, dec = case
    x = c["want"]["decoded"]
    got = fused_feature_decode(c["fm"].to(DEV), (Hg, Wg), c["w"].to(DEV) if dec else None, c["b"].to(DEV) if dec else None, half=half)
    assert got.shape == (Cout, Hg, Wg) and got.dtype == (torch.float16 if half else torch.float32)
    scale = float(x.abs().max())
    err = (got.double().cpu() - x).abs()
    if half:
        fig = float((err - x.abs() * 2.0 ** -11).max())
        print(flc.case_id(case), f"fp16 excess={fig:.3g} scale={scale:.3g}")
        assert fig <= 2e-5 * scale + 2.0 ** -25
    else:
        print(flc.case_id(case), f"fp32 err={float(err.max()) / scale:.3g}")
        assert float(err.max()) <= 1e-5 * scale


# ---- residuals that are exactly zero ----------------------------------------------------------------------------------------

def _quantised(shape, g):
    """Multiples of 2^-6 in [-4, 4]."""
    return torch.randint(-256, 257, shape, generator=g).float() / 64.0


def test_exact_zero_residuals_without_a_decoder():
    """Identity resize (scale exactly 1: taps 1 and 0) of a map of multiples of 2^-6: the resized value IS the source value.
    gt == fm on a seeded third of the elements: there d_feature_map is +0 or -0 - nothing else - and elsewhere it is
    +-fp32(1 / (N C)) by the sign of the exact residual, bit for bit (upstream gradient 0.5: an exact scaling)."""
    g = torch.Generator().manual_seed(21)
    C, H, W = 5, 7, 19                      # N = 133: three 64-pixel tiles, the last one ragged
    fm = _quantised((C, H, W), g)
    k = torch.randint(1, 65, (C, H, W), generator=g).float() / 64.0
    sgn = torch.randint(0, 2, (C, H, W), generator=g).float() * 2 - 1
    zero = torch.rand(C, H, W, generator=g) < 1 / 3
    gt = torch.where(zero, fm, fm + sgn * k)
    assert bool(zero.any()) and bool((~zero).any()) and bool(((gt == fm) == zero).all())
    up = 0.5
    loss, g_fm, _gw, _gb = _run_loss(fm, gt, None, None, up)
    inv_n = np.float32(1.0) / (np.float32(H * W) * np.float32(C))
    got = (g_fm / up).numpy()
    r = (fm.double() - gt.double()).numpy()             # exact in float64 as in fp32
    want = np.where(r > 0, inv_n, np.where(r < 0, -inv_n, np.float32(0))).astype(np.float32)
    assert np.array_equal(got, want)                    # (+0 == -0 compares equal; anything else at a zero residual does not)
    assert abs(float(loss) - float(np.abs(r).mean())) <= 2e-6


def test_exact_zero_residuals_behind_the_decoder():
    """C = 32 -> Cout = 33, identity resize, quantised map, every W row one-hot with +-1 or +-0.5, bias a multiple of 2^-6: y is
    exact in fp32.  gt == y on whole rows 0, 7, 32 (the last one alone in the ragged second W tile) and on a seeded third of the
    rest: the sign byte 0 must come back as gradient 0 in K2 (g_x), K3 (dW, db) alike.

    d_bias[co] is (#pos - #neg) / (N Cout) to 1e-6 relative.  Rows 4, 14 and 25 of this seed have as many positive as negative
    residuals without being all zero: the value is 0 and a relative bound says nothing, while the sum of +-1/(N Cout) over
    pixel ranges is rounded in fp32.  There the bound is the reference's own arithmetic: the same three torch ops run in fp32
    on the CPU miss 0 by 1.1641532e-10 (2^-33) on these inputs; allowed is 4 x that figure."""
    from oracle.feature_loss_oracle import reference_feature_l1
    g = torch.Generator().manual_seed(22)
    C, Cout, H, W = 32, 33, 5, 27           # N = 135: two 128-pixel workgroups, three 64-pixel tiles
    N = H * W
    fm = _quantised((C, H, W), g)
    hot = torch.randint(0, C, (Cout,), generator=g)
    val = torch.tensor([1.0, -1.0, 0.5, -0.5])[torch.randint(0, 4, (Cout,), generator=g)]
    w = torch.zeros(Cout, C)
    w[torch.arange(Cout), hot] = val
    b = torch.randint(-64, 65, (Cout,), generator=g).float() / 64.0
    y = fm[hot] * val[:, None, None] + b[:, None, None]                     # exact: |y| <= 5, multiples of 2^-7
    assert bool((y.double() == fm.double()[hot] * val.double()[:, None, None] + b.double()[:, None, None]).all())
    k = torch.randint(1, 65, (Cout, H, W), generator=g).float() / 64.0
    sgn = torch.randint(0, 2, (Cout, H, W), generator=g).float() * 2 - 1
    zero = torch.rand(Cout, H, W, generator=g) < 1 / 3
    zero[[0, 7, 32]] = True
    allzero = torch.zeros(Cout, dtype=torch.bool)
    allzero[[0, 7, 32]] = True
    gt = torch.where(zero, y, y + sgn * k)
    assert bool(((gt == y) == zero).all())
    up = 0.5
    loss, g_fm, g_w, g_b = _run_loss(fm, gt, w, b, up)
    want = reference_feature_l1(fm, gt, w, b)
    assert bool((want["decoded"] == y.double()).all())
    r = (y.double() - gt.double())
    assert abs(float(loss) - float(r.abs().mean())) <= 2e-6
    g_w, g_b, g_fm = g_w / up, g_b / up, g_fm / up
    for row in (0, 7, 32):
        assert float(g_b[row]) == 0.0 and bool((g_w[row] == 0).all()), row
    pos, neg = (r > 0).sum(dim=(1, 2)).double(), (r < 0).sum(dim=(1, 2)).double()
    want_b = (pos - neg) / (N * Cout)
    err_b = (g_b.double() - want_b).abs()
    live = want_b != 0
    print("d_bias: rel", float((err_b[live] / want_b[live].abs()).max()), "balanced rows", err_b[~live & ~allzero].tolist())
    assert bool((err_b[live] <= 1e-6 * want_b[live].abs()).all())
    assert int((~live & ~allzero).sum()) >= 1 and bool((err_b[~live] <= 4 * 1.1641532e-10).all())
    assert float((want["d_bias"] - want_b).abs().max()) <= 1e-15          # the float64 chain says the same: abs'(0) = 0
    assert float((g_w.double() - want["d_weight"]).abs().max()) <= 1e-5 * float(want["d_weight"].abs().max())
    assert float((g_fm.double() - want["d_feature_map"]).abs().max()) <= 1e-5 * float(want["d_feature_map"].abs().max())


# ---- views ------------------------------------------------------------------------------------------------------------------

def test_views_give_the_results_of_their_contiguous_copies():
    """A transposed feature map and ground truth, and a (Cout, C, 1, 1) weight that starts at storage offset 1 (not 16-byte
    aligned: the binding copies it, the C ABI would refuse it): bit-identical to the contiguous, aligned tensors."""
    from feature_loss import fused_feature_l1, fused_feature_decode
    C, H, W, Cout, Hg, Wg = 32, 9, 13, 33, 5, 13
    c = flc.build_case((C, H, W, Cout, Hg, Wg, True))
    fm, gt, w, b = (c[k].to(DEV) for k in ("fm", "gt", "w", "b"))
    fm_v = fm.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    gt_v = gt.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    store = torch.zeros(Cout * C + 1, device=DEV)
    store[1:] = w.reshape(-1)
    w_v = store[1:].view(Cout, C, 1, 1)
    assert not fm_v.is_contiguous() and not gt_v.is_contiguous() and w_v.storage_offset() == 1 and w_v.data_ptr() % 16 == 4
    assert torch.equal(fm_v, fm) and torch.equal(gt_v, gt) and torch.equal(w_v.reshape(Cout, C), w)

    def run(fm_, gt_, w_):
        leaves = [fm_.detach().requires_grad_(True), w_.detach().requires_grad_(True), b.detach().requires_grad_(True)]
        loss = fused_feature_l1(leaves[0], gt_, leaves[1], leaves[2])
        (UP * loss).backward()
        return [loss.detach()] + [x.grad.reshape(-1).clone() for x in leaves]

    base = run(fm, gt, w.reshape(Cout, C, 1, 1))
    # d_weight / d_bias are atomic sums over pixel ranges: N = 65 is two 64-pixel tiles, one per range, and the order of two
    # additions onto zero is immaterial (fp32 addition commutes), so the sums are bit-identical from run to run
    for got in (run(fm_v, gt_v, w.reshape(Cout, C, 1, 1)), run(fm, gt, w_v), run(fm_v, gt_v, w_v)):
        for a, e in zip(got, base):
            assert torch.equal(a, e)
    for half in (False, True):
        e = fused_feature_decode(fm, (Hg, Wg), w, b, half=half)
        assert torch.equal(fused_feature_decode(fm_v, (Hg, Wg), w_v, b, half=half), e)
    # without a decoder
    c = flc.build_case((5, H, W, 5, Hg, Wg, False))
    fm, gt = c["fm"].to(DEV), c["gt"].to(DEV)
    fm_v = fm.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    gt_v = gt.permute(0, 2, 1).contiguous().permute(0, 2, 1)
    outs = []
    for f, t in ((fm, gt), (fm_v, gt_v)):
        leaf = f.detach().requires_grad_(True)
        loss = fused_feature_l1(leaf, t)
        (UP * loss).backward()
        outs.append((loss.detach(), leaf.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(fused_feature_decode(fm_v, (Hg, Wg)), fused_feature_decode(fm, (Hg, Wg)))


# ---- the C ABI refuses what its kernels would fault on ----------------------------------------------------------------------

def test_c_abi_refuses_misaligned_weight_and_scratch():
    """The decoder kernels read `weight` and the scratch arrays with 16-byte accesses (include/f3dgs.h, Alignment): an aligned
    device pointer + 4 comes back as F3DGS_ERR_INVALID_ARGUMENT from the argument checks - no kernel ever sees it."""
    import ctypes
    import os
    import diff_gaussian_rasterization  # noqa: F401 (loads libf3dgs_hip.so next to torch's HIP runtime)
    from util import ROOT
    lib = ctypes.CDLL(os.path.join(ROOT, "feature-3dgs_amd", "csrc", "libf3dgs_hip.so"))
    lib.f3dgs_last_error.restype = ctypes.c_char_p
    vp = ctypes.c_void_p
    lib.f3dgs_feature_l1.argtypes = [ctypes.c_int] * 6 + [vp] * 10
    lib.f3dgs_feature_decode.argtypes = [ctypes.c_int] * 6 + [vp] * 4 + [ctypes.c_int, vp, vp]
    lib.f3dgs_feature_l1_scratch_bytes.restype = ctypes.c_size_t
    lib.f3dgs_feature_decode_scratch_bytes.restype = ctypes.c_size_t
    C, H, W, Cout, Hg, Wg = 32, 8, 8, 33, 4, 4
    INVALID = -1                                   # F3DGS_ERR_INVALID_ARGUMENT
    z = lambda n: torch.zeros(n + 8, device=DEV)
    fm, wt, bias, gt, loss, dfm, dw, db, out = z(C * H * W), z(Cout * C), z(Cout), z(Cout * Hg * Wg), z(1), z(C * H * W), z(Cout * C), z(Cout), z(Cout * Hg * Wg)
    nbytes = max(lib.f3dgs_feature_l1_scratch_bytes(C, Cout, Hg, Wg, 1), lib.f3dgs_feature_decode_scratch_bytes(C, Hg, Wg, 1))
    scratch = torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()
    assert all(p(t) % 16 == 0 for t in (fm, wt, scratch))
    for dw_off, ds_off in ((4, 0), (0, 4), (8, 0), (0, 1)):
        rc = lib.f3dgs_feature_l1(C, H, W, Cout, Hg, Wg, p(fm), p(wt) + dw_off, p(bias), p(gt), p(loss), p(dfm), p(dw), p(db),
                                  p(scratch) + ds_off, None)
        assert rc == INVALID and b"16-byte" in lib.f3dgs_last_error(), (dw_off, ds_off, rc)
        rc = lib.f3dgs_feature_decode(C, H, W, Cout, Hg, Wg, p(fm), p(wt) + dw_off, p(bias), p(out), 0, p(scratch) + ds_off, None)
        assert rc == INVALID and b"16-byte" in lib.f3dgs_last_error(), (dw_off, ds_off, rc)
    torch.cuda.synchronize()
    assert float(loss.abs().sum()) == 0 and float(out.abs().sum()) == 0 and float(dw.abs().sum()) == 0      # nothing ran
