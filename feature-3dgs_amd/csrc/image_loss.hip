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
// The tile, the window, the halo staging, the column pass, the expression of S and the fixed-order sums are ssim_tile.h's,
// shared with the image metrics; the row passes are this file's.
// Stages:
//   K1 il_forward_kernel    one 64 x 16 output tile of one plane per workgroup: x and y with a 5-pixel halo staged in LDS
//                           (zero outside the image), the 11-tap rows of the five moments into LDS, the 11-tap columns in
//                           registers; S, |x - y| partial sums per workgroup; the three maps when a gradient is wanted
//   K2 il_reduce_kernel     one workgroup: the partial sums in a fixed order (fp64) -> loss, l1, ssim, per-image ssim
//   K3 il_backward_kernel   the same halo scheme over the three maps, combined with x, y, sign(x - y) and the upstream
//                           gradient (a device scalar, or one per image) into d_image
// No atomics anywhere: two calls give the same bits.  Nothing is read back to the host and nothing is cleared with a
// memset: the calls may be captured into a graph.

#include "common.h"
#include "ssim_tile.h"

namespace f3dgs {

namespace {

using namespace ssim_tile;

struct FwdLds {
    float s[2][SH][SW];     // x, y with halo
    float h[5][SH][TW];     // 11-tap rows of x, y, x^2, y^2, xy
    float red[2][4];
};

// grid: one workgroup per (plane, tile row, tile column), plane-major, so that the partials of image n are one contiguous range
__global__ void __launch_bounds__(256)
il_forward_kernel(Geom g, Window win, const float* __restrict__ img, const float* __restrict__ gt, float* __restrict__ g_mu,
                  float* __restrict__ g_11, float* __restrict__ g_12, float* __restrict__ part_ssim, float* __restrict__ part_l1,
                  int vec4) {
    __shared__ __attribute__((aligned(16))) FwdLds L;
    const int b = blockIdx.x;
    const TilePos tp = tile_pos(g, b);
    const int plane = tp.plane, x0 = tp.x0, y0 = tp.y0;
    const size_t poff = (size_t)plane * g.H * g.W;
    const float* const src[2] = {img + poff, gt + poff};
    stage_tile<2>(L.s, src, g, x0, y0, vec4 != 0);
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // rows: 11 taps along x of the five moments, for every staged row
    for (int r = w; r < SH; r += 4) {
        float m1 = 0.f, m2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) {
            const float x = L.s[0][r][lane + SOFF + k], y = L.s[1][r][lane + SOFF + k];
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
    float acc[TH / 4][5];
    const int rb = w * (TH / 4);
    column_pass<5>(L.h, win, rb, lane, acc);

    float ssum = 0.f, lsum = 0.f;
    const int gx = x0 + lane;
#pragma unroll
    for (int i = 0; i < TH / 4; i++) {
        const int gy = y0 + rb + i;
        if (gx < g.W && gy < g.H) {
            const SsimPoint p = ssim_point(acc[i]);
            ssum += p.S;
            const float x = L.s[0][rb + i + R][lane + 8], y = L.s[1][rb + i + R][lane + 8];
            lsum += fabsf(x - y);
            if (g_mu) {
                const size_t o = poff + (size_t)gy * g.W + gx;
                const float mu1 = acc[i][0], mu2 = acc[i][1], invD = 1.f / p.D;
                g_mu[o] = 2.f * (mu2 * (p.A2 - p.A1) + mu1 * p.S * (p.B1 - p.B2)) * invD;
                g_11[o] = -p.S / p.B2;
                g_12[o] = 2.f * p.A1 * invD;
            }
        }
    }
    ssum = wave_sum(ssum);
    lsum = wave_sum(lsum);
    if (lane == 0) { L.red[0][w] = ssum; L.red[1][w] = lsum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_ssim[b] = four_wave_sum(L.red[0]);
        part_l1[b] = four_wave_sum(L.red[1]);
    }
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
    float s[3][SH][SW];     // g_mu, g_11, g_12 with halo
    float h[3][SH][TW];     // their 11-tap rows
};

// d_image = u * (ssim_coef * (G*g_mu + 2 x G*g_11 + y G*g_12) + l1_coef * sign(x - y)); u = upstream[0], or upstream[image]
__global__ void __launch_bounds__(256)
il_backward_kernel(Geom g, Window win, const float* __restrict__ img, const float* __restrict__ gt, const float* __restrict__ g_mu,
                   const float* __restrict__ g_11, const float* __restrict__ g_12, const float* __restrict__ upstream,
                   int upstream_per_image, float ssim_coef, float l1_coef, float* __restrict__ d_img, int vec4) {
    __shared__ __attribute__((aligned(16))) BwdLds L;
    const int b = blockIdx.x;
    const TilePos tp = tile_pos(g, b);
    const int plane = tp.plane, x0 = tp.x0, y0 = tp.y0;
    const size_t poff = (size_t)plane * g.H * g.W;
    const float* const src[3] = {g_mu + poff, g_11 + poff, g_12 + poff};
    stage_tile<3>(L.s, src, g, x0, y0, vec4 != 0);
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int r = w; r < SH; r += 4) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) {
            const float wk = win.w[k];
            a0 = fmaf(wk, L.s[0][r][lane + SOFF + k], a0);
            a1 = fmaf(wk, L.s[1][r][lane + SOFF + k], a1);
            a2 = fmaf(wk, L.s[2][r][lane + SOFF + k], a2);
        }
        L.h[0][r][lane] = a0; L.h[1][r][lane] = a1; L.h[2][r][lane] = a2;
    }
    __syncthreads();

    float acc[TH / 4][3];
    const int rb = w * (TH / 4);
    column_pass<3>(L.h, win, rb, lane, acc);

    const float u = upstream[upstream_per_image ? plane / g.C : 0];
    const int gx = x0 + lane;
#pragma unroll
    for (int i = 0; i < TH / 4; i++) {
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
        const size_t blocks = (size_t)tile_blocks(N, C, H, W);
        s.part_ssim = c.take<float>(blocks);
        s.part_l1 = c.take<float>(blocks);
        s.g_mu = c.take<float>(maps ? n : 0);
        s.g_11 = c.take<float>(maps ? n : 0);
        s.g_12 = c.take<float>(maps ? n : 0);
        if (bytes) *bytes = c.total();
        return s;
    }
};

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
    if (bad_sizes(N, C, H, W))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: bad sizes N=%d C=%d H=%d W=%d", N, C, H, W);
    if (!image || !gt || !loss || !l1 || !ssim || !scratch)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: null pointer");
    const Geom g = make_geom(N, C, H, W);
    const Scratch sc = Scratch::carve(static_cast<char*>(scratch), N, C, H, W, want_grad != 0, nullptr);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = (int)tile_blocks(N, C, H, W);
    const int vec4 = (W % 4 == 0) && aligned16(image) && aligned16(gt);
    hipLaunchKernelGGL(il_forward_kernel, dim3(blocks), dim3(256), 0, s, g, make_window(), image, gt,
                       want_grad ? sc.g_mu : nullptr, sc.g_11, sc.g_12, sc.part_ssim, sc.part_l1, vec4);
    const double n = (double)N * C * H * W;
    hipLaunchKernelGGL(il_reduce_kernel, dim3(1), dim3(256), 0, s, N, blocks / N, 1.0 / ((double)C * H * W), 1.0 / n,
                       (double)lambda_dssim, sc.part_ssim, sc.part_l1, loss, l1, ssim, ssim_per_image);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "image_loss forward: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

int f3dgs_image_loss_backward(int N, int C, int H, int W, const float* image, const float* gt, float lambda_dssim, int mode,
                              const float* upstream, const void* scratch, float* d_image, void* stream) {
    if (bad_sizes(N, C, H, W))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: bad sizes N=%d C=%d H=%d W=%d", N, C, H, W);
    if (!image || !gt || !upstream || !scratch || !d_image)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: null pointer");
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
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_loss: unknown mode %d", mode);
    }
    const Geom g = make_geom(N, C, H, W);
    const Scratch sc = Scratch::carve(static_cast<char*>(const_cast<void*>(scratch)), N, C, H, W, true, nullptr);
    const int blocks = (int)tile_blocks(N, C, H, W);
    const int vec4 = (W % 4 == 0) && aligned16(sc.g_mu) && aligned16(sc.g_11) && aligned16(sc.g_12);
    hipLaunchKernelGGL(il_backward_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), g, make_window(), image,
                       gt, sc.g_mu, sc.g_11, sc.g_12, upstream, mode == F3DGS_IMAGE_LOSS_SSIM_PER_IMAGE ? 1 : 0, ssim_coef, l1_coef,
                       d_image, vec4);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "image_loss backward: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
