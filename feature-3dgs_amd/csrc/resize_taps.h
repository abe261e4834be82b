// resize_taps.h - the bilinear resize of the feature-map loss (F.interpolate(mode='bilinear', align_corners=True),
// R/train.py:99-101) as per-axis tap lists, shared by the loss kernels (feature_loss.hip) and by the blend backward when it
// takes the loss's gradient at the LOSS's resolution (render_bwd_pl.hip, f3dgs_set_feature_grad_lowres), and the bilinear
// point itself, shared by the loss, the decode and the segmentation (segment.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace f3dgs {

struct ResizeGeom {
    int H, W, Hg, Wg;
    float sy, sx;      // (in - 1) / (out - 1), 0 when out == 1 (PyTorch: area_pixel_compute_scale, align_corners)
};

inline ResizeGeom make_resize_geom(int H, int W, int Hg, int Wg) {
    ResizeGeom g;
    g.H = H; g.W = W; g.Hg = Hg; g.Wg = Wg;
    g.sy = Hg > 1 ? (float)(H - 1) / (float)(Hg - 1) : 0.f;
    g.sx = Wg > 1 ? (float)(W - 1) / (float)(Wg - 1) : 0.f;
    return g;
}

// source taps of output index o (PyTorch upsample_bilinear2d, align_corners = true)
__device__ __forceinline__ void taps(int o, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    const float src = scale * (float)o;
    i0 = (int)src;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

// the taps of output pixel (yo, xo) along both axes
struct PixelTaps {
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
};

__device__ __forceinline__ PixelTaps pixel_taps(const ResizeGeom& g, int yo, int xo) {
    PixelTaps t;
    taps(yo, g.sy, g.H, t.y0, t.y1, t.ly0, t.ly1);
    taps(xo, g.sx, g.W, t.x0, t.x1, t.lx0, t.lx1);
    return t;
}

// The bilinear point from its four source values v<row><column>: THE order of operations of the resize - the decode, the loss
// and the segmentation promise each other the same bits, so nobody writes this expression out again
__device__ __forceinline__ float bilinear_mix(const PixelTaps& t, float v00, float v01, float v10, float v11) {
    return t.ly0 * (t.lx0 * v00 + t.lx1 * v01) + t.ly1 * (t.lx0 * v10 + t.lx1 * v11);
}

// ... of a plane of row width W
__device__ __forceinline__ float bilinear_point(const float* pl, int W, const PixelTaps& t) {
    return bilinear_mix(t, pl[t.y0 * W + t.x0], pl[t.y0 * W + t.x1], pl[t.y1 * W + t.x0], pl[t.y1 * W + t.x1]);
}

// candidate outputs of a source index i: outputs o whose taps can include i.
// scale 0: out == 1 (only output 0 exists) or in == 1 (EVERY output reads source index 0, the only one) - both are "all
// outputs, for source index 0".  ANY_SIZE = false is for callers that never enlarge (in >= out: the blend backward), where
// scale 0 can only mean out == 1 and the last output is the constant 0.
template <bool ANY_SIZE = false>
__device__ __forceinline__ void resize_cand(int i, float scale, int out, int& lo, int& hi) {
    if (scale <= 0.f) { lo = 0; hi = (i == 0) ? (ANY_SIZE ? out - 1 : 0) : -1; return; }
    lo = max(0, (int)floorf((float)(i - 1) / scale) - 1);
    hi = min(out - 1, (int)ceilf((float)(i + 1) / scale) + 1);
}

// The transposed resize along one axis: the (output, weight) list of source index i, outputs ascending, zero weights
// dropped; returns the count, or -1 when it exceeds CAP.  Shrinking (in >= out) never needs more than two entries.
template <int CAP, bool ANY_SIZE = false>
__device__ __forceinline__ int resize_build(int i, float scale, int in, int out, int* oo, float* ww) {
    int lo, hi, n = 0;
    resize_cand<ANY_SIZE>(i, scale, out, lo, hi);
    for (int o = lo; o <= hi; o++) {
        int a0, a1;
        float l0, l1;
        taps(o, scale, in, a0, a1, l0, l1);
        const float wv = (a0 == i ? l0 : 0.f) + (a1 == i ? l1 : 0.f);
        if (wv == 0.f) continue;
        if (n == CAP) return -1;
        oo[n] = o; ww[n] = wv; n++;
    }
    return n;
}

}  // namespace f3dgs
