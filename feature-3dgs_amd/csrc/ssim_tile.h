// ssim_tile.h - the SSIM tile machine shared by the fused image loss (image_loss.hip) and the image metrics (image_metrics.hip).
//
// Both tile an (N, C, H, W) batch into 64 x 16 outputs of one plane per workgroup of 256 threads, stage the tile with a 5-pixel
// halo in LDS (zero outside the image: the reference's zero padding), take the 11-tap Gaussian window (sigma 1.5, built in
// fp32 as the reference builds it) along the rows into LDS and along the columns in registers, evaluate
//     S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) = A1 A2 / (B1 B2)
// in the reference's order of operations, and reduce per-workgroup partial sums in a fixed order in fp64.  This header holds
// the one copy of what they share; the row passes (11 taps per lane in the loss, a sliding run of 8 pixels in the metrics)
// and the metrics' byte staging stay with their kernels.
//
// It is a header on purpose and must not become an object file of its own: image_metrics.o is compiled with
// -ffp-contract=off (the same bits for every input form), image_loss.o with the default contraction, so the same text
// legitimately compiles to different roundings in the two units, and each unit keeps its own flags and so its own bits.
// Everything here is `inline` (host) or `__device__ __forceinline__`.
#pragma once

#include <math.h>

#include "common.h"

namespace f3dgs {

namespace ssim_tile {

constexpr int R = 5;                 // window radius (window_size 11)
constexpr int TW = 64;               // output tile: one column per lane in the column pass
constexpr int TH = 16;               // four rows per wave
constexpr int SH = TH + 2 * R;       // staged rows
constexpr int SW = TW + 16;          // staged columns: x0 - 8 .. x0 + 71, whole 16-byte groups; the halo is 3 .. 76
constexpr int SOFF = 8 - R;          // staged column of the halo's first column
constexpr float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;

struct Window {
    float w[2 * R + 1];
};

// The reference's 1-D window (loss_utils.py:24-26): the Gaussian in fp32 (torch.Tensor of Python floats), normalised in fp32.
inline Window make_window() {
    Window win;
    float g[2 * R + 1], sum = 0.f;
    for (int i = 0; i <= 2 * R; i++) {
        g[i] = (float)exp(-(double)((i - R) * (i - R)) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i <= 2 * R; i++) win.w[i] = g[i] / sum;
    return win;
}

struct Geom {
    int N, C, H, W;
    int tiles_x, tiles_y;
};

inline Geom make_geom(int N, int C, int H, int W) {
    Geom g;
    g.N = N; g.C = C; g.H = H; g.W = W;
    g.tiles_x = (W + TW - 1) / TW;
    g.tiles_y = (H + TH - 1) / TH;
    return g;
}

// workgroups of a tile kernel = per-workgroup partials of each sum: one per (plane, tile row, tile column)
inline long long tile_blocks(int N, int C, int H, int W) {
    const Geom g = make_geom(N, C, H, W);
    return (long long)N * C * g.tiles_x * g.tiles_y;
}

inline bool bad_sizes(int N, int C, int H, int W) {
    return N <= 0 || C <= 0 || H <= 0 || W <= 0 || (long long)N * C * H * W >= (1ll << 40) ||
           tile_blocks(N, C, H, W) >= (1ll << 31);
}

// grid: one workgroup per (plane, tile row, tile column), plane-major, so that the partials of image n are one contiguous range
struct TilePos {
    int plane, x0, y0;
};

__device__ __forceinline__ TilePos tile_pos(const Geom& g, int b) {
    const int tiles = g.tiles_x * g.tiles_y;
    const int plane = b / tiles, t = b - plane * tiles;
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    return {plane, tx * TW, ty * TH};
}

// Stage Q planes (Q pointers at the same plane offset) of the tile with its halo into s[Q][SH][SW], zeros outside the image.
// With W % 4 == 0 and 16-byte aligned planes every staged 16-byte group is either wholly inside or wholly outside a row:
// float4 loads.
template <int Q>
__device__ __forceinline__ void stage_tile(float (&s)[Q][SH][SW], const float* const (&src)[Q], const Geom& g, int x0, int y0,
                                           bool vec4) {
    if (vec4) {
        constexpr int GROUPS = SW / 4;
        for (int i = threadIdx.x; i < SH * GROUPS; i += 256) {
            const int r = i / GROUPS, j = 4 * (i - r * GROUPS);
            const int gy = y0 - R + r, gx = x0 - 8 + j;
            const bool in = gy >= 0 && gy < g.H && gx >= 0 && gx < g.W;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in) v = *reinterpret_cast<const float4*>(src[q] + (size_t)gy * g.W + gx);
                *reinterpret_cast<float4*>(&s[q][r][j]) = v;
            }
        }
    } else {
        for (int i = threadIdx.x; i < SH * SW; i += 256) {
            const int r = i / SW, j = i - r * SW;
            const int gy = y0 - R + r, gx = x0 - 8 + j;
            const bool in = gy >= 0 && gy < g.H && gx >= 0 && gx < g.W;
#pragma unroll
            for (int q = 0; q < Q; q++) s[q][r][j] = in ? src[q][(size_t)gy * g.W + gx] : 0.f;
        }
    }
}

// Columns: the four output rows rb .. rb + 3 of this lane's column, 11 taps along y of the Q row sums in h, in registers.
template <int Q>
__device__ __forceinline__ void column_pass(const float (&h)[Q][SH][TW], const Window& win, int rb, int lane,
                                            float (&acc)[TH / 4][Q]) {
#pragma unroll
    for (int i = 0; i < TH / 4; i++)
#pragma unroll
        for (int q = 0; q < Q; q++) acc[i][q] = 0.f;
#pragma unroll
    for (int j = 0; j < TH / 4 + 2 * R; j++) {
        float v[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) v[q] = h[q][rb + j][lane];
#pragma unroll
        for (int i = 0; i < TH / 4; i++) {
            const int k = j - i;
            if (k >= 0 && k <= 2 * R) {
#pragma unroll
                for (int q = 0; q < Q; q++) acc[i][q] = fmaf(win.w[k], v[q], acc[i][q]);
            }
        }
    }
}

// SSIM of one pixel from its five windowed moments m = {G*x, G*y, G*x^2, G*y^2, G*xy}, in the reference's order of
// operations (loss_utils.py:44-58); the factors are what the loss's derivative maps are made of.
struct SsimPoint {
    float S, A1, A2, B1, B2, D;      // S = A1 A2 / D, D = B1 B2
};

__device__ __forceinline__ SsimPoint ssim_point(const float (&m)[5]) {
    const float mu1 = m[0], mu2 = m[1];
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu1_mu2;
    SsimPoint p;
    p.A1 = 2.f * mu1_mu2 + C1; p.A2 = 2.f * s12 + C2;
    p.B1 = mu1_sq + mu2_sq + C1; p.B2 = s1 + s2 + C2;
    p.D = p.B1 * p.B2;
    p.S = (p.A1 * p.A2) / p.D;
    return p;
}

// the workgroup's sum from its four waves' sums, in a fixed order
template <typename T>
__device__ __forceinline__ T four_wave_sum(const T* v) {
    return (v[0] + v[1]) + (v[2] + v[3]);
}

__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();            // (sh is re-used from one call to the next)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return four_wave_sum(sh);
}

}  // namespace ssim_tile

}  // namespace f3dgs
