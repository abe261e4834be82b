"""Timing of the viewer's render modes (view_modes.py, csrc/view_modes.hip) against a torch restatement of the reference's chain
(utils/image_utils.py:60-161), on the same GPU in the same process, at 1080p and at 256 x 256.

Per mode ('Depth', 'Edge', 'Normal', 'Curvature') and size: 5 warm-up calls, then 30 calls of each side, alternating, each
timed by device events; the median.  Timed are the float frame (render_net_image) and the uint8 frame (net_image_bytes against
the chain's clamp * 255 -> byte -> permute).  Also: the bytes the fused mode moves (read + written, counted from shapes) against
the compulsory 4 HW read of the depth map (12 HW of `render` for 'Edge') and 3 HW write of the byte frame, and the achieved rate
of the fused byte frame.  One JSON line per row, then a table.  A measurement needs a GPU: there is no CPU path.

    python tools/view_modes_bench.py [--sizes 1080x1920,256x256] [--errors]

--errors prints the kernels' errors on every case of tests/test_gpu_view_modes.py against the float64 oracle instead.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "feature-3dgs_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import view_modes as V                      # noqa: E402
import view_modes_oracle as O               # noqa: E402

DEV = "cuda:0"
MODES = {"Depth": 1, "Edge": 2, "Normal": 3, "Curvature": 4}


# ---- the reference's chain, restated with torch ops ------------------------------------------------------------------------
def chain_unproject(depth, cam):
    H, W = depth.shape
    x = torch.linspace(0, W - 1, W, device=depth.device)
    y = torch.linspace(0, H - 1, H, device=depth.device)
    Y, X = torch.meshgrid(y, x, indexing="ij")
    d = depth.reshape(-1)
    pc = torch.stack([X.reshape(-1) / (W - 1) * 2 - 1, Y.reshape(-1) / (H - 1) * 2 - 1, d], dim=-1)
    K = cam.projection_matrix
    sd = (K[2, 2] * pc[..., 2:3] + K[3, 2]) / (pc[..., 2:3] + 1e-8)
    pc = torch.cat((pc[..., 0:2], sd), dim=-1).view(H, W, 3)
    pc = torch.cat([pc, torch.ones_like(pc[:, :, :1])], dim=-1)
    pw = torch.matmul(pc, cam.full_proj_transform.inverse())
    return (pw[:, :, :3] / pw[:, :, 3:]).view(H, W, 3)


def chain_normals(depth, cam):
    depth = depth.squeeze()
    H, W = depth.shape
    pw = torch.zeros((H + 1, W + 1, 3), device=depth.device)
    pw[:H, :W, :] = chain_unproject(depth, cam)
    p1, p2, p3 = pw[:-1, :-1, :], pw[1:, :-1, :], pw[:-1, 1:, :]
    n = torch.cross(p2 - p1, p3 - p1, dim=-1)
    return n / (torch.norm(n, dim=-1, keepdim=True) + 1e-8)


def chain_gradient(image):
    sx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]).float().unsqueeze(0).unsqueeze(0).to(image.device) / 4
    sy = torch.tensor([[-1, -2, -1], [0, 0, 0], [1, 2, 1]]).float().unsqueeze(0).unsqueeze(0).to(image.device) / 4
    gx = torch.cat([F.conv2d(image[i].unsqueeze(0), sx, padding=1) for i in range(image.shape[0])])
    gy = torch.cat([F.conv2d(image[i].unsqueeze(0), sy, padding=1) for i in range(image.shape[0])])
    return torch.sqrt(gx ** 2 + gy ** 2).norm(dim=0, keepdim=True)


def chain_colormap(m, lut):
    m = (m - m.min()) / (m.max() - m.min())
    return lut[(m * 255).round().long().squeeze()].permute(2, 0, 1)


def chain_net_image(pkg, mode, cam, lut):
    if mode == "Depth":
        net = pkg["depth"]
    elif mode == "Edge":
        net = chain_gradient(pkg["render"])
    else:
        net = (chain_normals(pkg["depth"], cam).permute(2, 0, 1) + 1) / 2
        if mode == "Curvature":
            net = chain_gradient(net)
    return chain_colormap(net, lut) if net.shape[0] == 1 else net


def chain_bytes(pkg, mode, cam, lut):
    return (torch.clamp(chain_net_image(pkg, mode, cam, lut), min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous()


def alternating_medians(fa, fb, warmup=5, calls=30):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(calls):
        for fn, ts in ((fa, ta), (fb, tb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
    return float(np.median(ta)), float(np.median(tb))


def moved_bytes(mode, HW):
    """(fused float frame, fused byte frame, compulsory): bytes read + written, from shapes"""
    read_in = 12 * HW if mode == "Edge" else 4 * HW
    if mode == "Normal":
        return read_in + 12 * HW, read_in + 12 * HW + 12 * HW + 3 * HW, read_in + 3 * HW
    field = 0 if mode == "Depth" else 4 * HW                        # the one-channel field is written once
    minmax = 4 * HW if mode == "Depth" else 0                       # and the raw depth is read once more for its extremes
    return read_in + minmax + field + 4 * HW + 12 * HW, read_in + minmax + field + 4 * HW + 3 * HW, read_in + 3 * HW


def scene(H, W):
    P, full = O.make_camera("posed")
    cam = types.SimpleNamespace(projection_matrix=torch.from_numpy(P).to(DEV), full_proj_transform=torch.from_numpy(full).to(DEV))
    depth = torch.from_numpy(O.make_depth("step", H, W)).to(DEV)[None]
    render = torch.from_numpy(O.make_image("smooth", 3, H, W, 7)).to(DEV)
    return {"depth": depth, "render": render}, cam


def errors():
    from diff_gaussian_rasterization import _C
    print("case                         normals: median p99 max            curvature: median p99 max")
    for name in O.DEPTH_CASES:
        depth, proj, full = O.make_inputs(name)
        cam = types.SimpleNamespace(projection_matrix=torch.from_numpy(proj).to(DEV), full_proj_transform=torch.from_numpy(full).to(DEV))
        dd = torch.from_numpy(depth).to(DEV)
        n = V.depth_to_normal(dd, cam).cpu().numpy()
        c = _C.view_curvature(dd, *V._camera_matrices(cam, DEV))[0].cpu().numpy()
        en = O.error_stats(n, O.depth_to_normal(depth, proj, full), O.clean_footprint(depth, 0, 1))
        ec = O.error_stats(c, O.curvature(depth, proj, full), O.clean_footprint(depth, 1, 2))
        print(f"{name:26s} {en[0]:9.2e} {en[1]:9.2e} {en[2]:9.2e}      {ec[0]:9.2e} {ec[1]:9.2e} {ec[2]:9.2e}", flush=True)
    print("case                         edge: median p99 max")
    for name in O.IMAGE_CASES:
        img = O.make_inputs(name)
        e = O.error_stats(V.gradient_map(torch.from_numpy(img).to(DEV))[0].cpu().numpy(), O.gradient_map(img))
        print(f"{name:26s} {e[0]:9.2e} {e[1]:9.2e} {e[2]:9.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080x1920,256x256")
    ap.add_argument("--errors", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("view_modes_bench: no GPU: nothing is measured")
    if args.errors:
        return errors()
    lut = V.matplotlib_lut("turbo", DEV)
    items = list(V.RENDER_MODES)
    rows = []
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        pkg, cam = scene(H, W)
        for mode, k in MODES.items():
            with torch.no_grad():
                f_ms, c_ms = alternating_medians(lambda: V.render_net_image(pkg, items, k, cam), lambda: chain_net_image(pkg, mode, cam, lut))
                fb_ms, cb_ms = alternating_medians(lambda: V.net_image_bytes(pkg, items, k, cam), lambda: chain_bytes(pkg, mode, cam, lut))
                same = (V.net_image_bytes(pkg, items, k, cam).int() - chain_bytes(pkg, mode, cam, lut).int()).abs()
            bf, bb, need = moved_bytes(mode, H * W)
            row = {"H": H, "W": W, "mode": mode, "fused_ms": f_ms, "chain_ms": c_ms, "fused_bytes_ms": fb_ms, "chain_bytes_ms": cb_ms,
                   "moved_float_frame": bf, "moved_byte_frame": bb, "compulsory": need, "byte_frame_gbs": bb / (fb_ms * 1e-3) / 1e9,
                   "frame_pixels_differing_from_chain": float((same.amax(-1) > 0).float().mean())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\n    H     W  mode        fused    chain   ratio | bytes: fused    chain   ratio | moved / compulsory   GB/s   frame != chain")
    for r in rows:
        print(f"{r['H']:5d} {r['W']:5d}  {r['mode']:9s} {r['fused_ms']:7.3f}  {r['chain_ms']:7.3f}  {r['chain_ms'] / r['fused_ms']:6.1f} |"
              f"        {r['fused_bytes_ms']:7.3f}  {r['chain_bytes_ms']:7.3f}  {r['chain_bytes_ms'] / r['fused_bytes_ms']:6.1f} |"
              f"   {r['moved_byte_frame'] / r['compulsory']:6.2f}          {r['byte_frame_gbs']:7.0f}   {r['frame_pixels_differing_from_chain']:.4f}")


if __name__ == "__main__":
    main()
