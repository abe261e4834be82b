// image_metrics.hip - image-quality metrics of N pairs of views in one launch chain (include/f3dgs.h: f3dgs_image_metrics*).
//
// Replaces the image half of the reference's evaluation (metrics.py:71-74 `ssim`, `psnr`; train.py:210-239 `l1_loss`, `psnr`):
// per view pair five depthwise 11x11 convolutions, a squared-error pass and a host read.  Per image n of the batch
//     l1[n] = mean |x - y|      mse[n] = mean (x - y)^2      psnr[n] = 20 log10(1 / sqrt(mse[n]))   (fp32, from the fp32 mse)
//     ssim[n] = mean S          S of ssim_tile.h: Gaussian window 11, sigma 1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2
// Forward only: no derivative maps.  Each side is fp32 planes, fp32 planes quantised to the 8-bit value a saved PNG holds, or
// uint8 (planar or interleaved); an 8-bit side is staged as BYTES and widened with byte_to_unit, which is v / 255 bit for bit.
// Stages:
//   K1 im_tile_kernel     one 64 x 16 output tile of one plane per workgroup (the tile, fp32 staging, column pass and S of
//                         ssim_tile.h): x and y with a 5-pixel halo staged in LDS (zero outside the image); the 11-tap rows
//                         of the five moments by 208 threads, each sliding the window over a run of 8 pixels held in
//                         registers (18 staged values per side instead of 88), into LDS; the 11-tap columns in registers;
//                         S, |d|, d^2 partial sums
//   K2 im_reduce_kernel   one workgroup per image: its partials in a fixed order (fp64) -> l1, mse, psnr, ssim
// No atomics, no memset, no host read: two calls give the same bits and the call may be captured into a graph.

#include <math.h>

#include "common.h"
#include "ssim_tile.h"

namespace f3dgs {

namespace {

using namespace ssim_tile;

constexpr int RUN = 8;                // output pixels per thread of the row pass
constexpr int RUN_IN = RUN + 2 * R;   // staged values it reads: 18, from staged column 8 g + 3 on

// where a side's values come from
constexpr int SRC_F32 = 0, SRC_F32_QUANT = 1, SRC_U8_PLANAR = 2, SRC_U8_INTERLEAVED = 3;

struct Side {
    const void* p;
    int src;       // SRC_*
    int vec;       // whole 4-element groups may be loaded at once: W % 4 == 0 and the base aligned to 4 elements
};

// b / 255 for an integer 0 <= b <= 255, bit for bit the fp32 quotient torch's `div(255)` forms (to_tensor): the product with the
// rounded reciprocal is off by an ulp for 190 of the 256 values, one residual step corrects every one of them
// (tests/test_image_metrics_cpu.py checks all 256 in exact arithmetic).  Three instructions instead of a division per tap.
__device__ __forceinline__ float byte_to_unit(float b) {
    constexpr float RCP = 1.0f / 255.0f;
    const float q = __fmul_rn(b, RCP);
    const float e = __fmaf_rn(-q, 255.0f, b);
    return __fmaf_rn(e, RCP, q);
}

// What `mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)` makes of v (torchvision's save_image): two roundings, never one
// fused multiply-add; fmaxf drops a NaN, so NaN gives 0 - the value tests/golden/reference_image_metrics.npz pins for torch's
// cast on the CPU.
__device__ __forceinline__ uint32_t quantize(float v) {
    const float t = __fadd_rn(__fmul_rn(v, 255.0f), 0.5f);
    return (uint32_t)fminf(fmaxf(t, 0.0f), 255.0f);
}

__device__ __forceinline__ size_t planar_index(const Geom& g, int plane, int gy, int gx) {
    return ((size_t)plane * g.H + gy) * g.W + gx;
}
__device__ __forceinline__ size_t interleaved_index(const Geom& g, int plane, int gy, int gx) {
    const int n = plane / g.C, c = plane - n * g.C;
    return (((size_t)n * g.H + gy) * g.W + gx) * g.C + c;
}

// One 8-bit element of a side (in range)
__device__ __forceinline__ uint32_t load_byte(const Side& sd, const Geom& g, int plane, int gy, int gx) {
    if (sd.src == SRC_F32_QUANT) return quantize(static_cast<const float*>(sd.p)[planar_index(g, plane, gy, gx)]);
    if (sd.src == SRC_U8_PLANAR) return static_cast<const unsigned char*>(sd.p)[planar_index(g, plane, gy, gx)];
    return static_cast<const unsigned char*>(sd.p)[interleaved_index(g, plane, gy, gx)];
}

// Stage the tile of one side with its halo as bytes, four to a dword, zeros outside the image.
__device__ __forceinline__ void stage_bytes(unsigned char* s, const Side& sd, const Geom& g, int plane, int x0, int y0) {
    constexpr int GROUPS = SW / 4;
    uint32_t* const out = reinterpret_cast<uint32_t*>(s);
    for (int i = threadIdx.x; i < SH * GROUPS; i += 256) {
        const int r = i / GROUPS, j = i - r * GROUPS;
        const int gy = y0 - R + r, gx = x0 - 8 + 4 * j;
        uint32_t pack = 0;
        if (gy >= 0 && gy < g.H) {
            if (sd.vec && gx >= 0 && gx + 3 < g.W && sd.src != SRC_U8_INTERLEAVED) {
                const size_t o = planar_index(g, plane, gy, gx);
                if (sd.src == SRC_F32_QUANT) {
                    const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(sd.p) + o);
                    pack = quantize(v.x) | (quantize(v.y) << 8) | (quantize(v.z) << 16) | (quantize(v.w) << 24);
                } else {
                    pack = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(sd.p) + o);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (gx + e >= 0 && gx + e < g.W) pack |= load_byte(sd, g, plane, gy, gx + e) << (8 * e);
            }
        }
        out[i] = pack;
    }
}

// The same tile as fp32 (an unquantised fp32 side), or as bytes
template <bool BYTES>
__device__ __forceinline__ void stage(unsigned char* s, const Side& sd, const Geom& g, int plane, int x0, int y0) {
    if constexpr (BYTES) {
        stage_bytes(s, sd, g, plane, x0, y0);
    } else {
        const float* const src[1] = {static_cast<const float*>(sd.p) + (size_t)plane * g.H * g.W};
        stage_tile<1>(*reinterpret_cast<float(*)[1][SH][SW]>(s), src, g, x0, y0, sd.vec != 0);
    }
}

// The 18 staged values of row r from staged column 8 g + 3 on
template <bool BYTES>
__device__ __forceinline__ void load_run(const unsigned char* s, int r, int g, float (&v)[RUN_IN]) {
    if constexpr (BYTES) {
        const uint2* const p = reinterpret_cast<const uint2*>(s + r * SW + RUN * g);      // (8-byte aligned: SW % 8 == 0)
        uint32_t d[6];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint2 u = p[j];
            d[2 * j] = u.x;
            d[2 * j + 1] = u.y;
        }
#pragma unroll
        for (int i = 0; i < RUN_IN; i++) {
            const int e = i + 8 - R;
            v[i] = byte_to_unit((float)((d[e >> 2] >> (8 * (e & 3))) & 255u));
        }
    } else {
        // whole 16-byte groups from staged column 8 g on: single dwords at this lane stride would meet on four banks
        const float4* const p = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(s) + r * SW + RUN * g);
        float f[24];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const float4 u = p[j];
            f[4 * j] = u.x; f[4 * j + 1] = u.y; f[4 * j + 2] = u.z; f[4 * j + 3] = u.w;
        }
#pragma unroll
        for (int i = 0; i < RUN_IN; i++) v[i] = f[i + 8 - R];
    }
}

template <bool BYTES>
__device__ __forceinline__ float staged_value(const unsigned char* s, int r, int c) {
    if constexpr (BYTES) return byte_to_unit((float)s[r * SW + c]);
    else return reinterpret_cast<const float*>(s)[r * SW + c];
}

template <bool XB, bool YB>
struct TileLds {
    alignas(16) unsigned char sx[SH * SW * (XB ? 1 : 4)];      // x with halo: bytes, or fp32
    alignas(16) unsigned char sy[SH * SW * (YB ? 1 : 4)];
    alignas(16) float h[5][SH][TW];                            // 11-tap rows of x, y, x^2, y^2, xy
    float red[3][4];
};

// grid: one workgroup per (plane, tile row, tile column), plane-major, so that the partials of image n are one contiguous range.
// part: three lists of gridDim.x floats - S, |d|, d^2.
template <bool XB, bool YB>
__global__ void __launch_bounds__(256)
im_tile_kernel(Geom g, Window win, Side sx, Side sy, int want_ssim, float* __restrict__ part) {
    __shared__ TileLds<XB, YB> L;
    const int b = blockIdx.x;
    const TilePos tp = tile_pos(g, b);
    const int plane = tp.plane, x0 = tp.x0, y0 = tp.y0;
    stage<XB>(L.sx, sx, g, plane, x0, y0);
    stage<YB>(L.sy, sy, g, plane, x0, y0);
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rb = w * (TH / 4);
    float ssum = 0.f;
    if (want_ssim) {          // (the same in every thread)
        // rows: thread (r, run) slides the 11 taps along x over 8 pixels of staged row r, for the five moments
        if (threadIdx.x < SH * (TW / RUN)) {
            const int r = threadIdx.x >> 3, run = threadIdx.x & 7;
            float xv[RUN_IN], yv[RUN_IN];
            load_run<XB>(L.sx, r, run, xv);
            load_run<YB>(L.sy, r, run, yv);
            float acc[5][RUN];
#pragma unroll
            for (int q = 0; q < 5; q++)
#pragma unroll
                for (int o = 0; o < RUN; o++) acc[q][o] = 0.f;
            // input-major: every product is formed once; each output still takes its taps in the order k = 0 .. 10
#pragma unroll
            for (int i = 0; i < RUN_IN; i++) {
                const float x = xv[i], y = yv[i];
                const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
                for (int o = 0; o < RUN; o++) {
                    const int k = i - o;
                    if (k >= 0 && k <= 2 * R) {
                        const float wk = win.w[k];
                        acc[0][o] = fmaf(wk, x, acc[0][o]);
                        acc[1][o] = fmaf(wk, y, acc[1][o]);
                        acc[2][o] = fmaf(wk, xx, acc[2][o]);
                        acc[3][o] = fmaf(wk, yy, acc[3][o]);
                        acc[4][o] = fmaf(wk, xy, acc[4][o]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 5; q++) {
                float4* const dst = reinterpret_cast<float4*>(&L.h[q][r][RUN * run]);
                dst[0] = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
                dst[1] = make_float4(acc[q][4], acc[q][5], acc[q][6], acc[q][7]);
            }
        }
        __syncthreads();

        // columns: this wave's four output rows, 11 taps along y, in registers
        float acc[TH / 4][5];
        column_pass<5>(L.h, win, rb, lane, acc);
#pragma unroll
        for (int i = 0; i < TH / 4; i++)
            if (x0 + lane < g.W && y0 + rb + i < g.H) ssum += ssim_point(acc[i]).S;
    }

    float lsum = 0.f, msum = 0.f;
#pragma unroll
    for (int i = 0; i < TH / 4; i++) {
        if (x0 + lane < g.W && y0 + rb + i < g.H) {
            const float d = staged_value<XB>(L.sx, rb + i + R, lane + 8) - staged_value<YB>(L.sy, rb + i + R, lane + 8);
            lsum += fabsf(d);
            msum = fmaf(d, d, msum);
        }
    }
    ssum = wave_sum(ssum);
    lsum = wave_sum(lsum);
    msum = wave_sum(msum);
    if (lane == 0) { L.red[0][w] = ssum; L.red[1][w] = lsum; L.red[2][w] = msum; }
    __syncthreads();
    if (threadIdx.x < 3) part[(size_t)threadIdx.x * gridDim.x + b] = four_wave_sum(L.red[threadIdx.x]);
}

// One workgroup per image: every thread sums a fixed strided set of the image's partials in fp64, then a fixed tree; thread 0
// finalises.  psnr as utils/image_utils.py:23-25 forms it in fp32, from the fp32 mse: 20 * log10(1 / sqrt(mse)), +inf at mse 0.
__global__ void __launch_bounds__(256)
im_reduce_kernel(int per_image_blocks, size_t blocks, double inv_chw, int want_ssim, const float* __restrict__ part,
                 float* __restrict__ l1, float* __restrict__ mse, float* __restrict__ psnr, float* __restrict__ ssim) {
    __shared__ double sh[4];
    const int n = blockIdx.x;
    const float* const ps = part + (size_t)n * per_image_blocks;
    const float* const pl = ps + blocks;
    const float* const pm = pl + blocks;
    double s = 0.0, l = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < per_image_blocks; i += 256) {
        if (want_ssim) s += (double)ps[i];
        l += (double)pl[i];
        m += (double)pm[i];
    }
    s = block_sum(s, sh);
    l = block_sum(l, sh);
    m = block_sum(m, sh);
    if (threadIdx.x == 0) {
        const float mse_f = (float)(m * inv_chw);
        if (l1) l1[n] = (float)(l * inv_chw);
        if (mse) mse[n] = mse_f;
        if (psnr) psnr[n] = 20.0f * log10f(1.0f / sqrtf(mse_f));
        if (ssim) ssim[n] = (float)(s * inv_chw);
    }
}

// 0 on success; the side's description for the kernels
int make_side(const void* p, int format, bool quant, int W, const char* name, Side* out) {
    if (format != F3DGS_IMAGE_F32 && format != F3DGS_IMAGE_U8_PLANAR && format != F3DGS_IMAGE_U8_INTERLEAVED)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_metrics: unknown format %d of %s", format, name);
    if (quant && format != F3DGS_IMAGE_F32)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT,
                             "image_metrics: quantize flag on the uint8 side %s (it holds 8-bit values already)", name);
    out->p = p;
    out->src = format == F3DGS_IMAGE_F32 ? (quant ? SRC_F32_QUANT : SRC_F32)
                                         : (format == F3DGS_IMAGE_U8_PLANAR ? SRC_U8_PLANAR : SRC_U8_INTERLEAVED);
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    out->vec = (W % 4 == 0) && (format == F3DGS_IMAGE_F32 ? (a & 15) == 0 : (a & 3) == 0) ? 1 : 0;
    return F3DGS_OK;
}

template <bool XB, bool YB>
void launch_tiles(int blocks, hipStream_t s, const Geom& g, const Side& sx, const Side& sy, int want_ssim, float* part) {
    hipLaunchKernelGGL((im_tile_kernel<XB, YB>), dim3(blocks), dim3(256), 0, s, g, make_window(), sx, sy, want_ssim, part);
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_image_metrics_scratch_bytes(int N, int C, int H, int W) {
    if (bad_sizes(N, C, H, W)) return 0;
    Carver c(nullptr);
    c.take<float>(3 * (size_t)tile_blocks(N, C, H, W));
    return c.total();
}

int f3dgs_image_metrics(int N, int C, int H, int W, const void* image, int image_format, const void* gt, int gt_format, int flags,
                        float* l1, float* mse, float* psnr, float* ssim, void* scratch, void* stream) {
    if (N == 0) return F3DGS_OK;
    if (bad_sizes(N, C, H, W))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_metrics: bad sizes N=%d C=%d H=%d W=%d", N, C, H, W);
    if (flags & ~(F3DGS_METRICS_QUANTIZE_IMAGE | F3DGS_METRICS_QUANTIZE_GT))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_metrics: unknown flags 0x%x", flags);
    Side sx, sy;
    if (make_side(image, image_format, (flags & F3DGS_METRICS_QUANTIZE_IMAGE) != 0, W, "image", &sx) != F3DGS_OK ||
        make_side(gt, gt_format, (flags & F3DGS_METRICS_QUANTIZE_GT) != 0, W, "gt", &sy) != F3DGS_OK)
        return F3DGS_ERR_INVALID_ARGUMENT;
    if (!image || !gt || !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "image_metrics: null pointer");
    if (!l1 && !mse && !psnr && !ssim) return F3DGS_OK;
    const Geom g = make_geom(N, C, H, W);
    const size_t nblocks = (size_t)tile_blocks(N, C, H, W);
    const int blocks = (int)nblocks;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    float* const part = Carver(static_cast<char*>(scratch)).take<float>(3 * nblocks);
    const int want_ssim = ssim ? 1 : 0;
    const bool xb = sx.src != SRC_F32, yb = sy.src != SRC_F32;
    if (xb && yb) launch_tiles<true, true>(blocks, s, g, sx, sy, want_ssim, part);
    else if (xb) launch_tiles<true, false>(blocks, s, g, sx, sy, want_ssim, part);
    else if (yb) launch_tiles<false, true>(blocks, s, g, sx, sy, want_ssim, part);
    else launch_tiles<false, false>(blocks, s, g, sx, sy, want_ssim, part);
    hipLaunchKernelGGL(im_reduce_kernel, dim3(N), dim3(256), 0, s, blocks / N, nblocks, 1.0 / ((double)C * H * W), want_ssim, part,
                       l1, mse, psnr, ssim);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "image_metrics: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
