// image_loss.hip - fused L1 + D-SSIM image loss, forward and backward (include/f3dgs.h: f3dgs_image_loss_*).
//
// Replaces the reference's (train.py:99-105, utils/loss_utils.py:17-18, :33-63)
//     loss = (1 - lambda) * l1_loss(image, gt) + lambda * (1 - ssim(image, gt))
// and its autograd backward: five depthwise 11x11 convolutions, about twenty elementwise kernels and, backward, three
// transposed convolutions.  Per (image, channel) plane, with G the normalised Gaussian window (sigma 1.5, zero padding 5):
//     mu1 = G*x   mu2 = G*y   s1 = G*x^2 - mu1^2   s2 = G*y^2 - mu2^2   s12 = G*xy - mu1 mu2
//     S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) = A1 A2 / (B1 B2)
// S depends on x only through mu1, E[x^2] and E[xy]; its total derivatives with respect to those three
//     g_mu = 2 (mu2 (A2 - A1) + mu1 S (B1 - B2)) / (B1 B2)    g_11 = -S / B2    g_12 = 2 A1 / (B1 B2)
// are written per pixel by K1, and K2 applies the transposed window (G is symmetric: the same stencil) to them:
//     dS_sum/dx = G*g_mu + 2 x G*g_11 + y G*g_12.
// Stages:
//   K1 il_forward_kernel    one 64 x 16 output tile of one plane per workgroup: x and y with a 5-pixel halo staged in LDS
//                           (zero outside the image), the 11-tap rows of the five moments into LDS, the 11-tap columns in
//                           registers; S, |x - y| partial sums per workgroup; the three maps when a gradient is wanted
//   K2 il_reduce_kernel     one workgroup: the partial sums in a fixed order (fp64) -> loss, l1, ssim, per-image ssim
//   K3 il_backward_kernel   the same halo scheme over the three maps, combined with x, y, sign(x - y) and the upstream
//                           gradient (a device scalar, or one per image) into d_image
// No atomics anywhere: two calls give the same bits.  Nothing is read back to the host and nothing is cleared with a
// memset: the calls may be captured into a graph.

#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "common.h"

namespace f3dgs {

namespace {

constexpr int IL_R = 5;                   // window radius (window_size 11)
constexpr int IL_TW = 64;                 // output tile: one column per lane
constexpr int IL_TH = 16;                 // four rows per wave
constexpr int IL_SH = IL_TH + 2 * IL_R;   // staged rows
constexpr int IL_SW = IL_TW + 16;         // staged columns: x0 - 8 .. x0 + 71, whole 16-byte groups; the halo is 3 .. 76
constexpr int IL_SOFF = 8 - IL_R;         // staged column of the halo's first column
constexpr float IL_C1 = 0.01f * 0.01f, IL_C2 = 0.03f * 0.03f;

struct Window {
    float w[2 * IL_R + 1];
};

// The reference's 1-D window (loss_utils.py:24-26): the Gaussian in fp32 (torch.Tensor of Python floats), normalised in fp32.
Window make_window() {
    Window win;
    float g[2 * IL_R + 1], sum = 0.f;
    for (int i = 0; i <= 2 * IL_R; i++) {
        g[i] = (float)exp(-(double)((i - IL_R) * (i - IL_R)) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i <= 2 * IL_R; i++) win.w[i] = g[i] / sum;
    return win;
}

struct Geom {
    int N, C, H, W;
    int tiles_x, tiles_y;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Stage Q planes (Q pointers at the same plane offset) of the tile with its halo, zeros outside the image.  With W % 4 == 0
// and 16-byte aligned planes every staged 16-byte group is either wholly inside or wholly outside a row: float4 loads.
template <int Q>
__device__ __forceinline__ void stage_tile(float (&s)[Q][IL_SH][IL_SW], const float* const (&src)[Q], const Geom& g, int x0, int y0,
                                           bool vec4) {
    if (vec4) {
        constexpr int GROUPS = IL_SW / 4;
        for (int i = threadIdx.x; i < IL_SH * GROUPS; i += 256) {
            const int r = i / GROUPS, j = 4 * (i - r * GROUPS);
            const int gy = y0 - IL_R + r, gx = x0 - 8 + j;
            const bool in = gy >= 0 && gy < g.H && gx >= 0 && gx < g.W;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in) v = *reinterpret_cast<const float4*>(src[q] + (size_t)gy * g.W + gx);
                *reinterpret_cast<float4*>(&s[q][r][j]) = v;
            }
        }
    } else {
        for (int i = threadIdx.x; i < IL_SH * IL_SW; i += 256) {
            const int r = i / IL_SW, j = i - r * IL_SW;
            const int gy = y0 - IL_R + r, gx = x0 - 8 + j;
            const bool in = gy >= 0 && gy < g.H && gx >= 0 && gx < g.W;
#pragma unroll
            for (int q = 0; q < Q; q++) s[q][r][j] = in ? src[q][(size_t)gy * g.W + gx] : 0.f;
        }
    }
}

struct FwdLds {
    float s[2][IL_SH][IL_SW];        // x, y with halo
    float h[5][IL_SH][IL_TW];        // 11-tap rows of x, y, x^2, y^2, xy
    float red[2][4];
};

// grid: one workgroup per (plane, tile row, tile column), plane-major, so that the partials of image n are one contiguous range
__global__ void __launch_bounds__(256)
il_forward_kernel(Geom g, Window win, const float* __restrict__ img, const float* __restrict__ gt, float* __restrict__ g_mu,
                  float* __restrict__ g_11, float* __restrict__ g_12, float* __restrict__ part_ssim, float* __restrict__ part_l1,
                  int vec4) {
    __shared__ __attribute__((aligned(16))) FwdLds L;
    const int b = blockIdx.x;
    const int tiles = g.tiles_x * g.tiles_y;
    const int plane = b / tiles, t = b - plane * tiles;
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    const int x0 = tx * IL_TW, y0 = ty * IL_TH;
    const size_t poff = (size_t)plane * g.H * g.W;
    const float* const src[2] = {img + poff, gt + poff};
    stage_tile<2>(L.s, src, g, x0, y0, vec4 != 0);
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // rows: 11 taps along x of the five moments, for every staged row
    for (int r = w; r < IL_SH; r += 4) {
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * IL_R; k++) {
            const float x = L.s[0][r][lane + IL_SOFF + k], y = L.s[1][r][lane + IL_SOFF + k];
            const float wk = win.w[k];
            m1 = fmaf(wk, x, m1);
            m2 = fmaf(wk, y, m2);
            e11 = fmaf(wk, x * x, e11);
            e22 = fmaf(wk, y * y, e22);
            e12 = fmaf(wk, x * y, e12);
        }
        L.h[0][r][lane] = m1; L.h[1][r][lane] = m2; L.h[2][r][lane] = e11; L.h[3][r][lane] = e22; L.h[4][r][lane] = e12;
    }
    __syncthreads();

    // columns: this wave's four output rows, 11 taps along y, in registers
    float acc[IL_TH / 4][5];
#pragma unroll
    for (int i = 0; i < IL_TH / 4; i++)
#pragma unroll
        for (int q = 0; q < 5; q++) acc[i][q] = 0.f;
    const int rb = w * (IL_TH / 4);
#pragma unroll
    for (int j = 0; j < IL_TH / 4 + 2 * IL_R; j++) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; q++) v[q] = L.h[q][rb + j][lane];
#pragma unroll
        for (int i = 0; i < IL_TH / 4; i++) {
            const int k = j - i;
            if (k >= 0 && k <= 2 * IL_R) {
#pragma unroll
                for (int q = 0; q < 5; q++) acc[i][q] = fmaf(win.w[k], v[q], acc[i][q]);
            }
        }
    }

    float ssum = 0.f, lsum = 0.f;
    const int gx = x0 + lane;
#pragma unroll
    for (int i = 0; i < IL_TH / 4; i++) {
        const int gy = y0 + rb + i;
        if (gx < g.W && gy < g.H) {
            const float mu1 = acc[i][0], mu2 = acc[i][1];
            // the reference's order of operations (loss_utils.py:44-58)
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const float s1 = acc[i][2] - mu1_sq, s2 = acc[i][3] - mu2_sq, s12 = acc[i][4] - mu1_mu2;
            const float A1 = 2.f * mu1_mu2 + IL_C1, A2 = 2.f * s12 + IL_C2;
            const float B1 = mu1_sq + mu2_sq + IL_C1, B2 = s1 + s2 + IL_C2;
            const float D = B1 * B2;
            const float S = (A1 * A2) / D;
            ssum += S;
            const float x = L.s[0][rb + i + IL_R][lane + 8], y = L.s[1][rb + i + IL_R][lane + 8];
            lsum += fabsf(x - y);
            if (g_mu) {
                const size_t o = poff + (size_t)gy * g.W + gx;
                const float invD = 1.f / D;
                g_mu[o] = 2.f * (mu2 * (A2 - A1) + mu1 * S * (B1 - B2)) * invD;
                g_11[o] = -S / B2;
                g_12[o] = 2.f * A1 * invD;
            }
        }
    }
    ssum = wave_sum(ssum);
    lsum = wave_sum(lsum);
    if (lane == 0) { L.red[0][w] = ssum; L.red[1][w] = lsum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_ssim[b] = (L.red[0][0] + L.red[0][1]) + (L.red[0][2] + L.red[0][3]);
        part_l1[b] = (L.red[1][0] + L.red[1][1]) + (L.red[1][2] + L.red[1][3]);
    }
}

__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();            // (sh is re-used from one call to the next)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// One workgroup; image by image, every thread sums a fixed strided set of the image's partials in fp64, then a fixed tree.
__global__ void __launch_bounds__(256)
il_reduce_kernel(int N, int per_image_blocks, double inv_chw, double inv_n, double lam, const float* __restrict__ part_ssim,
                 const float* __restrict__ part_l1, float* __restrict__ loss, float* __restrict__ l1, float* __restrict__ ssim,
                 float* __restrict__ ssim_img) {
    __shared__ double sh[4];
    double ts = 0.0, tl = 0.0;
    for (int n = 0; n < N; n++) {
        double s = 0.0, l = 0.0;
        const size_t base = (size_t)n * per_image_blocks;
        for (int i = threadIdx.x; i < per_image_blocks; i += 256) {
            s += (double)part_ssim[base + i];
            l += (double)part_l1[base + i];
        }
        s = block_sum(s, sh);
        l = block_sum(l, sh);
        ts += s;
        tl += l;
        if (ssim_img && threadIdx.x == 0) ssim_img[n] = (float)(s * inv_chw);
    }
    if (threadIdx.x == 0) {
        const double mean_l1 = tl * inv_n, mean_s = ts * inv_n;
        if (l1) *l1 = (float)mean_l1;
        if (ssim) *ssim = (float)mean_s;
        if (loss) *loss = (float)((1.0 - lam) * mean_l1 + lam * (1.0 - mean_s));
    }
}

struct BwdLds {
    float s[3][IL_SH][IL_SW];        // g_mu, g_11, g_12 with halo
    float h[3][IL_SH][IL_TW];        // their 11-tap rows
};

// d_image = u * (ssim_coef * (G*g_mu + 2 x G*g_11 + y G*g_12) + l1_coef * sign(x - y)); u = upstream[0], or upstream[image]
__global__ void __launch_bounds__(256)
il_backward_kernel(Geom g, Window win, const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ g_mu,
                   const float* __restrict__ g_11, const float* __restrict__ g_12, const float* __restrict__ upstream,
                   int upstream_per_image, float ssim_coef, float l1_coef, float* __restrict__ d_img, int vec4) {
    __shared__ __attribute__((aligned(16))) BwdLds L;
    const int b = blockIdx.x;
    const int tiles = g.tiles_x * g.tiles_y;
    const int plane = b / tiles, t = b - plane * tiles;
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    const int x0 = tx * IL_TW, y0 = ty * IL_TH;
    const size_t poff = (size_t)plane * g.H * g.W;
    const float* const src[3] = {g_mu + poff, g_11 + poff, g_12 + poff};
    stage_tile<3>(L.s, src, g, x0, y0, vec4 != 0);
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r = w; r < IL_SH; r += 4) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * IL_R; k++) {
            const float wk = win.w[k];
            a0 = fmaf(wk, L.s[0][r][lane + IL_SOFF + k], a0);
            a1 = fmaf(wk, L.s[1][r][lane + IL_SOFF + k], a1);
            a2 = fmaf(wk, L.s[2][r][lane + IL_SOFF + k], a2);
        }
        L.h[0][r][lane] = a0; L.h[1][r][lane] = a1; L.h[2][r][lane] = a2;
    }
    __syncthreads();

    float acc[IL_TH / 4][3];
#pragma unroll
    for (int i = 0; i < IL_TH / 4; i++)
#pragma unroll
        for (int q = 0; q < 3; q++) acc[i][q] = 0.f;
    const int rb = w * (IL_TH / 4);
#pragma unroll
    for (int j = 0; j < IL_TH / 4 + 2 * IL_R; j++) {
        float v[3];
#pragma unroll
        for (int q = 0; q < 3; q++) v[q] = L.h[q][rb + j][lane];
#pragma unroll
        for (int i = 0; i < IL_TH / 4; i++) {
            const int k = j - i;
            if (k >= 0 && k <= 2 * IL_R) {
#pragma unroll
                for (int q = 0; q < 3; q++) acc[i][q] = fmaf(win.w[k], v[q], acc[i][q]);
            }
        }
    }

    const float u = upstream[upstream_per_image ? plane / g.C : 0];
    const int gx = x0 + lane;
#pragma unroll
    for (int i = 0; i < IL_TH / 4; i++) {
        const int gy = y0 + rb + i;
        if (gx < g.W && gy < g.H) {
            const size_t o = poff + (size_t)gy * g.W + gx;
            const float x = img[o], y = gt[o];
            const float ds = acc[i][0] + 2.f * x * acc[i][1] + y * acc[i][2];
            const float sg = x > y ? 1.f : (x < y ? -1.f : 0.f);
            d_img[o] = u * (ssim_coef * ds + l1_coef * sg);
        }
    }
}

struct Scratch {
    float* g_mu;
    float* g_11;
    float* g_12;
    float* part_ssim;
    float* part_l1;
    static Scratch carve(char* base, int N, int C, int H, int W, bool maps, size_t* bytes) {
        Carver c(base);
        Scratch s;
        const size_t n = (size_t)N * C * H * W;
        const size_t blocks = (size_t)N * C * ((W + IL_TW - 1) / IL_TW) * ((H + IL_TH - 1) / IL_TH);
        s.part_ssim = c.take<float>(blocks);
        s.part_l1 = c.take<float>(blocks);
        s.g_mu = c.take<float>(maps ? n : 0);
        s.g_11 = c.take<float>(maps ? n : 0);
        s.g_12 = c.take<float>(maps ? n : 0);
        if (bytes) *bytes = c.total();
        return s;
    }
};

Geom make_geom(int N, int C, int H, int W) {
    Geom g;
    g.N = N; g.C = C; g.H = H; g.W = W;
    g.tiles_x = (W + IL_TW - 1) / IL_TW;
    g.tiles_y = (H + IL_TH - 1) / IL_TH;
    return g;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int bad(int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return report_error(code, buf);
}

bool bad_sizes(int N, int C, int H, int W) {
    return N <= 0 || C <= 0 || H <= 0 || W <= 0 || (long long)N * C * H * W >= (1ll << 40) ||
           (long long)N * C * ((W + IL_TW - 1) / IL_TW) * ((H + IL_TH - 1) / IL_TH) >= (1ll << 31);
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_image_loss_scratch_bytes(int N, int C, int H, int W, int want_grad) {
    if (bad_sizes(N, C, H, W)) return 0;
    size_t b = 0;
    Scratch::carve(nullptr, N, C, H, W, want_grad != 0, &b);
    return b;
}

int f3dgs_image_loss_forward(int N, int C, int H, int W, const float* image, const float* gt, float lambda_dssim, int want_grad,
                             float* loss, float* l1, float* ssim, float* ssim_per_image, void* scratch, void* stream) {
    if (bad_sizes(N, C, H, W)) return bad(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: bad sizes N=%d C=%d H=%d W=%d", N, C, H, W);
    if (!image || !gt || !loss || !l1 || !ssim || !scratch) return bad(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: null pointer");
    const Geom g = make_geom(N, C, H, W);
    const Scratch sc = Scratch::carve(static_cast<char*>(scratch), N, C, H, W, want_grad != 0, nullptr);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = N * C * g.tiles_x * g.tiles_y;
    const int vec4 = (W % 4 == 0) && aligned16(image) && aligned16(gt);
    hipLaunchKernelGGL(il_forward_kernel, dim3(blocks), dim3(256), 0, s, g, make_window(), image, gt,
                       want_grad ? sc.g_mu : nullptr, sc.g_11, sc.g_12, sc.part_ssim, sc.part_l1, vec4);
    const double n = (double)N * C * H * W;
    hipLaunchKernelGGL(il_reduce_kernel, dim3(1), dim3(256), 0, s, N, blocks / N, 1.0 / ((double)C * H * W), 1.0 / n,
                       (double)lambda_dssim, sc.part_ssim, sc.part_l1, loss, l1, ssim, ssim_per_image);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bad(F3DGS_ERR_HIP, "image_loss forward: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

int f3dgs_image_loss_backward(int N, int C, int H, int W, const float* image, const float* gt, float lambda_dssim, int mode,
                              const float* upstream, const void* scratch, float* d_image, void* stream) {
    if (bad_sizes(N, C, H, W)) return bad(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: bad sizes N=%d C=%d H=%d W=%d", N, C, H, W);
    if (!image || !gt || !upstream || !scratch || !d_image) return bad(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: null pointer");
    float ssim_coef, l1_coef;
    const double n = (double)N * C * H * W;
    if (mode == F3DGS_IMAGE_LOSS_L1_DSSIM) {
        ssim_coef = (float)(-(double)lambda_dssim / n);
        l1_coef = (float)((1.0 - (double)lambda_dssim) / n);
    } else if (mode == F3DGS_IMAGE_LOSS_SSIM) {
        ssim_coef = (float)(1.0 / n);
        l1_coef = 0.f;
    } else if (mode == F3DGS_IMAGE_LOSS_SSIM_PER_IMAGE) {
        ssim_coef = (float)(1.0 / ((double)C * H * W));
        l1_coef = 0.f;
    } else {
        return bad(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: unknown mode %d", mode);
    }
    const Geom g = make_geom(N, C, H, W);
    const Scratch sc = Scratch::carve(static_cast<char*>(const_cast<void*>(scratch)), N, C, H, W, true, nullptr);
    const int blocks = N * C * g.tiles_x * g.tiles_y;
    const int vec4 = (W % 4 == 0) && aligned16(sc.g_mu) && aligned16(sc.g_11) && aligned16(sc.g_12);
    hipLaunchKernelGGL(il_backward_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g, make_window(), image, gt,
                       sc.g_mu, sc.g_11, sc.g_12, upstream, mode == F3DGS_IMAGE_LOSS_SSIM_PER_IMAGE ? 1 : 0, ssim_coef, l1_coef,
                       d_image, vec4);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return bad(F3DGS_ERR_HIP, "image_loss backward: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
