"""GPU tests of the viewer's render modes (csrc/view_modes.hip, view_modes.py) against the float64 oracle on the host
(tests/view_modes_oracle.py).  The judge is always that oracle, never the kernels' output.

The kernels' tile edge is T = 16 (F3DGS_VIEW_TILE, asserted below); the shapes are 2x2, 2x9, 9x2, T-1, T, T+1, 17x23, 33x70
(2T+1 rows) and 64x129 (4T rows, 8T+1 columns), each with two of the four cameras and four depth fields
(view_modes_oracle.DEPTH_CASES), and eleven images of 1, 3 and 5 channels, two of them constant (IMAGE_CASES).

Bars:
  normals, curvature   per case, the kernel's |error| against the oracle at its median, 99th percentile and maximum must not
                       exceed the reference's own float32 error at the same statistic (fixture: e_normals, e_curvature), factor
                       1.  Where the depth has a hole of zeros the statistics run over the pixels whose depth footprint holds
                       no zero; everywhere else the output must be finite where the oracle's is.
  edge operator        maximum error <= 8 x E_EDGE, E_EDGE the largest error the reference's float32 conv2d chain showed over
                       the fixture's images (another summation order is another realisation of the same rounding; the factor
                       of tests/test_gpu_feature_pca.py)
  palette              fed a float32 field and its min and max, indices equal the oracle's (evaluated in float64 on that same
                       field) outside the band |s - (k + 1/2)| <= 255 * 2^-22 and differ by at most 1 inside it; at most 1 % of
                       a case's pixels lie in the band.  End to end through the kernels' own field the band is widened by
                       255 e / (max - min), e the case's permitted field error: for 'Edge' (e = 8 E_EDGE) and 'Depth' (e = 0).
                       For 'Curvature' e is the reference's own maximum error, of order 0.1, and the widened band covers every
                       index: that rule says nothing there and is not claimed; the curvature frame is held by its field's
                       bars, by the palette's exactness on the field it is given and by the min/max slot's.
"""
import os
import types

import numpy as np
import pytest
import torch

import view_modes_oracle as O
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "reference_view_modes.npz"))
E_EDGE = max(float(GOLDEN[f"{n}/e_edge"][2]) for n in O.IMAGE_CASES)
TURBO, JET = GOLDEN["turbo"], GOLDEN["jet"]
_cache = {}


def _depth_case(name):
    """inputs on host and device, camera, oracle normals and curvature: computed once, shared, never modified"""
    if name not in _cache:
        depth, proj, full = O.make_inputs(name)
        cam = O.Camera(torch.from_numpy(proj).to(DEV), torch.from_numpy(full).to(DEV))
        _cache[name] = (depth, torch.from_numpy(depth).to(DEV), cam, O.depth_to_normal(depth, proj, full), O.curvature(depth, proj, full))
    return _cache[name]


def _image_case(name):
    if name not in _cache:
        img = O.make_inputs(name)
        _cache[name] = (img, torch.from_numpy(img).to(DEV), O.gradient_map(img))
    return _cache[name]


def _lut(a):
    return torch.from_numpy(a).to(DEV)


def _matrices(cam):
    import view_modes as V
    return V._camera_matrices(cam, DEV)


def _within(name, what, got, want, mask, bars):
    e = O.error_stats(got, want, mask)
    print(f"{name}: {what} median {e[0]:.2e} p99 {e[1]:.2e} max {e[2]:.2e}   bars {bars[0]:.2e} {bars[1]:.2e} {bars[2]:.2e}")
    assert (e <= bars).all(), (name, what, e, bars)


def _indices_follow_the_rule(name, got_idx, field32, lo, hi, widen=0.0):
    """`field32`: the float32 field the kernel read (or, end to end, the ORACLE's field); indices against the oracle's"""
    want = O.colormap_index(field32, lo, hi)
    band = O.in_band(field32, lo, hi, widen=widen)
    diff = np.abs(got_idx.astype(np.int64) - want)
    share = float(band.mean())
    print(f"{name}: {int((diff != 0).sum())} of {diff.size} indices off the oracle, band share {share:.4f}")
    assert not diff[~band].any() and diff.max(initial=0) <= 1 and share <= O.BAND_CAP, name


def _index_of(frame, lut):
    px = frame.transpose(1, 2, 0).reshape(-1, 1, 3)
    hit = (px == lut[None]).all(-1)
    assert hit.any(1).all(), "a colour of the frame is not a row of the table"
    return hit.argmax(1).reshape(frame.shape[1:])


def test_the_tile_edge_is_what_the_shapes_assume():
    from diff_gaussian_rasterization import _C
    assert _C.VIEW_TILE == O.TILE == 16


@pytest.mark.parametrize("name", list(O.DEPTH_CASES))
def test_normals_against_the_oracle(name):
    import view_modes as V
    depth, dd, cam, want, _ = _depth_case(name)
    before = dd.clone()
    n = V.depth_to_normal(dd[None], cam)
    assert n.shape == depth.shape + (3,) and n.dtype == torch.float32 and n.device == dd.device
    assert torch.equal(dd, before), "the input was modified"
    got = n.cpu().numpy()
    assert np.isfinite(got[np.isfinite(want).all(-1)]).all()
    assert not got[-1, -1].any(), "the corner pixel"
    _within(name, "normals", got, want, O.clean_footprint(depth, 0, 1), GOLDEN[f"{name}/e_normals"])
    assert torch.equal(n, V.depth_to_normal(dd, cam)), "two calls, (1, H, W) and (H, W)"
    # the 'Normal' mode's image: (n + 1) / 2, channel-major, from the same kernel
    img = V.render_net_image({"depth": dd[None]}, list(V.RENDER_MODES), 3, cam)
    assert img.shape == (3,) + depth.shape and torch.equal(img, (n.permute(2, 0, 1) + 1) / 2)


@pytest.mark.parametrize("name", list(O.DEPTH_CASES))
def test_curvature_against_the_oracle_and_bit_for_bit_against_the_two_kernels(name):
    from diff_gaussian_rasterization import _C
    depth, dd, cam, _, want = _depth_case(name)
    proj, inv = _matrices(cam)
    field, mm = _C.view_curvature(dd, proj, inv)
    assert field.shape == depth.shape and field.dtype == torch.float32
    got = field.cpu().numpy()
    assert np.isfinite(got[np.isfinite(want)]).all()
    _within(name, "curvature", got, want, O.clean_footprint(depth, 1, 2), GOLDEN[f"{name}/e_curvature"])
    two, mm2 = _C.view_gradient(_C.view_normals(dd, proj, inv, True, True))
    assert torch.equal(field, two), "fused curvature != gradient of the normal image"
    assert torch.equal(mm, mm2) and torch.equal(mm, torch.stack(torch.aminmax(field)))
    again, mm3 = _C.view_curvature(dd, proj, inv)
    assert torch.equal(field, again) and torch.equal(mm, mm3), "two calls differ"


@pytest.mark.parametrize("name", list(O.IMAGE_CASES))
def test_edge_operator_against_the_oracle(name):
    import view_modes as V
    from diff_gaussian_rasterization import _C
    img, di, want = _image_case(name)
    before = di.clone()
    g = V.gradient_map(di)
    assert g.shape == (1,) + img.shape[1:] and g.dtype == torch.float32 and torch.equal(di, before)
    e = O.error_stats(g[0].cpu().numpy(), want)
    print(f"{name}: edge median {e[0]:.2e} p99 {e[1]:.2e} max {e[2]:.2e}   bar {8 * E_EDGE:.2e} (reference's own: {GOLDEN[f'{name}/e_edge']})")
    assert e[2] <= 8 * E_EDGE
    field, mm = _C.view_gradient(di)
    assert torch.equal(field, g[0]) and torch.equal(mm, torch.stack(torch.aminmax(field))), "two calls / the min-max slot"
    view = di.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert torch.equal(V.gradient_map(view), g), "a non-contiguous image"


@pytest.mark.parametrize("name", ["2x2_posed_smooth", "15x15_centred_smooth", "16x16_posed_step", "17x23_offcentre_step", "33x70_aniso_hole",
                                  "64x129_posed_hole"])
def test_palette_on_the_oracles_field(name):
    """the palette kernel alone: the oracle's curvature and the raw depth as float32 fields with their own min and max; both
    modes, the float image and the bytes"""
    from diff_gaussian_rasterization import _C
    depth, dd, _, _, curv = _depth_case(name)
    for what, f32 in (("curvature", curv.astype(np.float32)), ("depth", depth)):
        fd = torch.from_numpy(f32).to(DEV)
        mm = torch.tensor([float(f32.min()), float(f32.max())], device=DEV)
        img, u8 = _C.view_palette(fd, mm, _lut(TURBO), _C.VIEW_PALETTE_MINMAX, True, True)
        assert img.shape == (3,) + f32.shape and u8.shape == f32.shape + (3,) and u8.dtype == torch.uint8
        img = img.cpu().numpy()
        _indices_follow_the_rule(f"{name} {what}", _index_of(img, TURBO), f32, f32.min(), f32.max())
        assert np.array_equal(u8.cpu().numpy(), O.to_bytes(img)), "bytes of the float image"
        only = _C.view_palette(fd, mm, _lut(TURBO), _C.VIEW_PALETTE_MINMAX, False, True)
        assert only[0] is None and torch.equal(only[1], u8)
        assert torch.equal(_C.view_minmax(fd), mm), "view_minmax != the field's min and max"
    # `max` mode on a 256-entry jet table: matplotlib's float call, exact outside the truncation's band
    img, u8 = _C.view_palette(dd, _C.view_minmax(dd), _lut(JET), _C.VIEW_PALETTE_MAX, True, True)
    got, want, band = _index_of(img.cpu().numpy(), JET), O.max_index(depth), O.in_max_band(depth)
    assert not (got != want)[~band].any() and np.abs(got - want).max() <= 1 and band.mean() <= O.BAND_CAP
    assert np.array_equal(got[~band], GOLDEN[f"{name}/idx_jet"][~band]), "matplotlib's own indices"
    assert np.array_equal(u8.cpu().numpy(), O.to_bytes(img.cpu().numpy()))


def test_palette_of_a_constant_map_and_other_table_sizes():
    import view_modes as V
    flat = torch.full((1, 5, 7), 2.5, device=DEV)
    img = V.colormap(flat, lut=_lut(TURBO))
    assert img.shape == (3, 5, 7) and torch.equal(img, _lut(TURBO)[0][:, None, None].expand(3, 5, 7)), "max == min: index 0 everywhere"
    ramp = torch.arange(0, 9, device=DEV, dtype=torch.float32).reshape(1, 3, 3)                 # s = v / 8 * (L - 1)
    for L in (2, 9, 4096):
        lut = torch.rand(L, 3, generator=torch.Generator().manual_seed(L)).to(DEV)
        want = np.rint(np.arange(9) / 8 * (L - 1)).astype(np.int64).reshape(3, 3)
        assert torch.equal(V.colormap(ramp, lut=lut), lut[torch.from_numpy(want).to(DEV)].permute(2, 0, 1)), L
    # signed fields and -0: the slot holds the field's own extremes
    from diff_gaussian_rasterization import _C
    for vals in ([-3.0, -1.5, -2.0], [-0.0, 4.0, -7.25, 3.0], [0.0, -0.0], [5.0]):
        f = torch.tensor(vals, device=DEV)
        assert torch.equal(_C.view_minmax(f), torch.stack(torch.aminmax(f))), vals
    big = torch.randn(3_000_017, generator=torch.Generator().manual_seed(5)).to(DEV)             # more than one grid stride
    assert torch.equal(_C.view_minmax(big), torch.stack(torch.aminmax(big)))


@pytest.mark.parametrize("name", ["c3_2x9", "c3_15x15", "c5_17x17", "c1_17x23", "c5_33x70", "c3_64x129", "c3_17x23_constant"])
def test_edge_frame_end_to_end(name):
    """render_net_image('Edge') and net_image_bytes through the kernels' own field and slot, against the ORACLE's field; the
    band is widened by 255 * 8 E_EDGE / (max - min)"""
    import view_modes as V
    img, di, want = _image_case(name)
    pkg = {"render": di}
    frame = V.render_net_image(pkg, list(V.RENDER_MODES), 2, None)
    assert frame.shape == (3,) + img.shape[1:] and frame.dtype == torch.float32
    widen = 255 * 8 * E_EDGE / (want.max() - want.min())
    _indices_follow_the_rule(name, _index_of(frame.cpu().numpy(), TURBO), want, want.min(), want.max(), widen=widen)
    u8 = V.net_image_bytes(pkg, list(V.RENDER_MODES), 2, None)
    assert u8.shape == img.shape[1:] + (3,) and np.array_equal(u8.cpu().numpy(), O.to_bytes(frame.cpu().numpy()))
    assert torch.equal(frame, V.render_net_image(pkg, list(V.RENDER_MODES), 2, None)), "two calls differ"


@pytest.mark.parametrize("name", ["2x9_aniso_step", "17x17_centred_hole", "17x23_posed_smooth", "33x70_centred_step"])
def test_depth_and_curvature_frames_end_to_end(name):
    import view_modes as V
    from diff_gaussian_rasterization import _C
    depth, dd, cam, _, _ = _depth_case(name)
    pkg = {"depth": dd[None]}
    modes = list(V.RENDER_MODES)
    frame = V.render_net_image(pkg, modes, 1, cam)                        # 'Depth': the field is the input, e = 0
    got = _index_of(frame.cpu().numpy(), TURBO)
    _indices_follow_the_rule(name + " depth", got, depth, depth.min(), depth.max())
    band = O.in_band(depth)
    assert np.array_equal(got[~band], GOLDEN[f"{name}/idx_depth"][~band]), "the reference's own 'Depth' frame"
    assert torch.equal(frame, V.colormap(dd[None]))
    # 'Curvature': the frame is the palette of the kernel's OWN field with the slot's min and max (the field itself is held
    # by test_curvature_against_the_oracle...; the widened-band rule is vacuous for it, see the module docstring)
    frame = V.render_net_image(pkg, modes, 4, cam)
    field, mm = _C.view_curvature(dd, *_matrices(cam))
    f32 = field.cpu().numpy()
    assert frame.shape == (3,) + depth.shape
    idx = _index_of(frame.cpu().numpy(), TURBO)
    want, inb = O.colormap_index(f32, f32.min(), f32.max()), O.in_band(f32, f32.min(), f32.max())
    assert not (idx != want)[~inb].any() and np.abs(idx - want).max() <= 1
    u8 = V.net_image_bytes(pkg, modes, 4, cam)
    assert np.array_equal(u8.cpu().numpy(), O.to_bytes(frame.cpu().numpy()))


def test_install_and_all_six_modes():
    import view_modes as V
    m = V.install(types.ModuleType("utils.image_utils"))
    for n in ("depth_to_normal", "gradient_map", "colormap", "render_net_image"):
        assert getattr(m, n) is getattr(V, n)
    depth, dd, cam, _, _ = _depth_case("17x23_posed_smooth")
    img, di, _ = _image_case("c3_17x23_constant")
    import feature_pca_oracle as PO
    fm = torch.from_numpy(PO.make_inputs("c20_45x60")).to(DEV)[:, :17, :23].contiguous()
    pkg = {"render": torch.rand(3, 17, 23, generator=torch.Generator().manual_seed(1)).to(DEV) * 1.2 - 0.1, "depth": dd[None], "feature_map": fm}
    V.reset_feature_basis()
    frames = []
    for mode in range(6):
        out = m.render_net_image(pkg, list(V.RENDER_MODES), mode, cam)
        assert out.shape == (3, 17, 23) and out.dtype == torch.float32 and out.device == dd.device, V.RENDER_MODES[mode]
        u8 = V.net_image_bytes(pkg, list(V.RENDER_MODES), mode, cam)
        assert u8.shape == (17, 23, 3) and u8.dtype == torch.uint8
        assert np.array_equal(u8.cpu().numpy(), O.to_bytes(out.cpu().numpy())), V.RENDER_MODES[mode]
        frames.append(out)
    assert torch.equal(frames[0], pkg["render"])
    # 'Feature Map': shape, range and determinism only; the basis of the first frame is kept until it is reset
    assert float(frames[5].min()) >= 0 and float(frames[5].max()) <= 1
    assert torch.equal(frames[5], V.render_net_image(pkg, list(V.RENDER_MODES), 5, cam))
    basis = V._feature_basis
    V.render_net_image({"feature_map": fm * 0.5 + 0.1}, list(V.RENDER_MODES), 5, cam)
    assert V._feature_basis is basis
    V.reset_feature_basis()
    assert V._feature_basis is None
    # a one-channel `render` is coloured like any one-channel result
    one = V.render_net_image({"render": dd[None]}, list(V.RENDER_MODES), 0, cam)
    assert torch.equal(one, V.colormap(dd[None]))


def test_capture_in_a_graph():
    """every launch goes to the current stream, nothing is read back or allocated by the library: the curvature frame replays"""
    from diff_gaussian_rasterization import _C
    depth, dd, cam, _, _ = _depth_case("33x70_centred_step")
    proj, inv = _matrices(cam)
    lut = _lut(TURBO)
    field, mm = _C.view_curvature(dd, proj, inv)
    want = _C.view_palette(field, mm, lut, _C.VIEW_PALETTE_MINMAX, False, True)[1]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f2, m2 = _C.view_curvature(dd, proj, inv)
        u8 = _C.view_palette(f2, m2, lut, _C.VIEW_PALETTE_MINMAX, False, True)[1]
    u8.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(u8, want)
