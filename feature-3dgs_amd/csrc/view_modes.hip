// view_modes.hip - the viewer's render modes of a rendered view: normals from depth, the edge operator, curvature (the edge
// operator of the normal image) in one pass, and the palette-coloured frame of a one-channel map.
//
// Replaces the torch chain behind the reference's render_net_image (utils/image_utils.py:60-161; callers view.py:25 and
// train.py:164):
//     unproject_depth_map   meshgrid, stacks, an (HW,4) x (4,4) matmul with full_proj_transform.inverse(), a divide
//     depth_to_normal       a zero-padded (H+1,W+1,3) copy, three shifted slices, two differences, cross, norm
//     gradient_map          two conv2d per channel, squares, sqrt, norm over channels
//     colormap              min, max, scale, round, LUT gather, permute
// Formulation of the normals: the reference turns depth into an NDC z of about 0.9975 in float32 and differences float32 world
// points, which leaves rounding noise of order 1 on some normals.  Here the unprojection - the reference's own
// formula, with the inverse of the full projection handed in as doubles - and the two differences p2 - p1, p3 - p1 are float64,
// everything after them float32.
//
// Kernels (tile = VT x VT pixels per workgroup of 256 threads, one thread per pixel):
//   view_normals_kernel    (VT+1)^2 world points (tile + right/bottom halo) in LDS, each depth unprojected once per tile
//   view_gradient_kernel   per channel a (VT+2)^2 tile of the image in LDS, zeros outside the image
//   view_curvature_kernel  (VT+3)^2 points -> (VT+2)^2 values of (n + 1) / 2 in LDS (zeros outside the image) -> the edge
//                          operator; same __device__ functions as the two kernels above, so the same bits
//   view_minmax_kernel     min and max of a field (grid-stride)
//   view_palette_kernel    index from the field and the min/max slot, LUT row -> (3,HW) float and / or (HW,3) bytes
//   view_bytes_kernel      (3,HW) float image -> (HW,3) bytes
// Min and max: fminf / fmaxf through wave shuffles and LDS, then INTEGER atomics on the float's own bit pattern (signed
// compare for one sign, unsigned for the other - the slot holds a float at every moment); a one-thread launch sets the slot
// to (+inf, -inf) first.  min and max are exact in any order: two calls give identical bits.
// The file is compiled with -ffp-contract=off: which products are fused is written out (none), not left to the optimiser,
// so that the fused curvature and gradient-of-normals agree bit for bit.

#include <math.h>

#include "common.h"

namespace f3dgs {

namespace {

constexpr int VT = F3DGS_VIEW_TILE;

struct Camera {
    double m[16];        // the inverse of full_proj_transform, row-major
    double f1, f2;       // projection_matrix[2][2], [3][2]
    double sx, sy;       // 2 / (W - 1), 2 / (H - 1)
};

__device__ __forceinline__ Camera load_camera(int H, int W, const float* __restrict__ proj, const double* __restrict__ inv) {
    Camera c;
#pragma unroll
    for (int i = 0; i < 16; i++) c.m[i] = inv[i];
    c.f1 = (double)proj[10];
    c.f2 = (double)proj[14];
    c.sx = 2.0 / (double)(W - 1);
    c.sy = 2.0 / (double)(H - 1);
    return c;
}

// unproject_depth_map for one pixel; the zero vector outside the image (the reference's zero padding to (H+1, W+1))
__device__ __forceinline__ void unproject(const Camera& c, int y, int x, int H, int W, const float* __restrict__ depth, double* p) {
    if (y < 0 || x < 0 || y >= H || x >= W) {
        p[0] = p[1] = p[2] = 0.0;
        return;
    }
    const double d = (double)depth[(size_t)y * W + x];
    const double X = (double)x * c.sx - 1.0, Y = (double)y * c.sy - 1.0;
    const double sd = (c.f1 * d + c.f2) / (d + 1e-8);
    const double iw = 1.0 / (X * c.m[3] + Y * c.m[7] + sd * c.m[11] + c.m[15]);
    p[0] = (X * c.m[0] + Y * c.m[4] + sd * c.m[8] + c.m[12]) * iw;
    p[1] = (X * c.m[1] + Y * c.m[5] + sd * c.m[9] + c.m[13]) * iw;
    p[2] = (X * c.m[2] + Y * c.m[6] + sd * c.m[10] + c.m[14]) * iw;
}

// cross(p2 - p1, p3 - p1) / (|.| + 1e-8): the differences in float64, the rest float32
__device__ __forceinline__ void normal_of(const double* p1, const double* p2, const double* p3, float* n) {
    const float ax = (float)(p2[0] - p1[0]), ay = (float)(p2[1] - p1[1]), az = (float)(p2[2] - p1[2]);
    const float bx = (float)(p3[0] - p1[0]), by = (float)(p3[1] - p1[1]), bz = (float)(p3[2] - p1[2]);
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const float len = sqrtf(cx * cx + cy * cy + cz * cz) + 1e-8f;
    n[0] = cx / len;
    n[1] = cy / len;
    n[2] = cz / len;
}

__device__ __forceinline__ float half_map(float n) { return (n + 1.f) * 0.5f; }

// acc + gx^2 + gy^2 of the 3 x 3 neighbourhood whose top-left corner is a[0]; taps [[-1,0,1],[-2,0,2],[-1,0,1]] / 4 and
// its transpose
__device__ __forceinline__ float edge_accumulate(float acc, const float* a, int ld) {
    const float a00 = a[0], a01 = a[1], a02 = a[2];
    const float a10 = a[ld], a12 = a[ld + 2];
    const float a20 = a[2 * ld], a21 = a[2 * ld + 1], a22 = a[2 * ld + 2];
    const float gx = ((a02 - a00) + (a22 - a20)) * 0.25f + (a12 - a10) * 0.5f;
    const float gy = ((a20 - a00) + (a22 - a02)) * 0.25f + (a21 - a01) * 0.5f;
    return (acc + gx * gx) + gy * gy;
}

// float min / max by integer atomics on the value's own bits.  v is not NaN and not -0 (callers add +0.f).
__device__ __forceinline__ void atomic_min_float(float* addr, float v) {
    if (v >= 0.f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_float(float* addr, float v) {
    if (v >= 0.f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

// every thread of the 256 calls it; lo = +inf, hi = -inf where a thread has no value
__device__ __forceinline__ void block_minmax(float lo, float hi, float* __restrict__ minmax) {
    __shared__ float red[2][4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d, 64));
        hi = fmaxf(hi, __shfl_xor(hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = lo;
        red[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
        if (lo <= hi) {                     // at least one value, none of them NaN
            atomic_min_float(minmax, lo + 0.f);
            atomic_max_float(minmax + 1, hi + 0.f);
        }
    }
}

__global__ void view_minmax_init_kernel(float* __restrict__ minmax) {
    if (threadIdx.x == 0) {
        minmax[0] = INFINITY;
        minmax[1] = -INFINITY;
    }
}

__global__ void __launch_bounds__(256) view_normals_kernel(int H, int W, int tiles_x, const float* __restrict__ depth,
                                                           const float* __restrict__ proj, const double* __restrict__ inv,
                                                           float* __restrict__ out, int chw, int half) {
    __shared__ double P[VT + 1][VT + 1][3];
    const int y0 = (int)(blockIdx.x / tiles_x) * VT, x0 = (int)(blockIdx.x % tiles_x) * VT;
    const Camera cam = load_camera(H, W, proj, inv);
    for (int i = threadIdx.x; i < (VT + 1) * (VT + 1); i += 256) {
        const int ly = i / (VT + 1), lx = i % (VT + 1);
        unproject(cam, y0 + ly, x0 + lx, H, W, depth, P[ly][lx]);
    }
    __syncthreads();
    const int ty = threadIdx.x / VT, tx = threadIdx.x % VT;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) return;
    float n[3];
    normal_of(P[ty][tx], P[ty + 1][tx], P[ty][tx + 1], n);
    const size_t p = (size_t)y * W + x, HW = (size_t)H * W;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float v = half ? half_map(n[k]) : n[k];
        if (chw) out[k * HW + p] = v;
        else out[p * 3 + k] = v;
    }
}

__global__ void __launch_bounds__(256) view_gradient_kernel(int Cn, int H, int W, int tiles_x, const float* __restrict__ image,
                                                            float* __restrict__ out, float* __restrict__ minmax) {
    __shared__ float S[VT + 2][VT + 3];
    const int y0 = (int)(blockIdx.x / tiles_x) * VT, x0 = (int)(blockIdx.x % tiles_x) * VT;
    const int ty = threadIdx.x / VT, tx = threadIdx.x % VT;
    const size_t HW = (size_t)H * W;
    float acc = 0.f;
    for (int c = 0; c < Cn; c++) {
        const float* src = image + (size_t)c * HW;
        __syncthreads();
        for (int i = threadIdx.x; i < (VT + 2) * (VT + 2); i += 256) {
            const int ly = i / (VT + 2), lx = i % (VT + 2);
            const int y = y0 + ly - 1, x = x0 + lx - 1;
            S[ly][lx] = (y >= 0 && x >= 0 && y < H && x < W) ? src[(size_t)y * W + x] : 0.f;
        }
        __syncthreads();
        acc = edge_accumulate(acc, &S[ty][tx], VT + 3);
    }
    const int y = y0 + ty, x = x0 + tx;
    const bool in = y < H && x < W;
    const float v = sqrtf(acc);
    if (in) out[(size_t)y * W + x] = v;
    if (minmax) block_minmax(in ? v : INFINITY, in ? v : -INFINITY, minmax);
}

__global__ void __launch_bounds__(256) view_curvature_kernel(int H, int W, int tiles_x, const float* __restrict__ depth,
                                                             const float* __restrict__ proj, const double* __restrict__ inv,
                                                             float* __restrict__ out, float* __restrict__ minmax) {
    __shared__ double P[VT + 3][VT + 3][3];
    __shared__ float N[3][VT + 2][VT + 3];
    const int y0 = (int)(blockIdx.x / tiles_x) * VT, x0 = (int)(blockIdx.x % tiles_x) * VT;
    const Camera cam = load_camera(H, W, proj, inv);
    for (int i = threadIdx.x; i < (VT + 3) * (VT + 3); i += 256) {
        const int ly = i / (VT + 3), lx = i % (VT + 3);
        unproject(cam, y0 + ly - 1, x0 + lx - 1, H, W, depth, P[ly][lx]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (VT + 2) * (VT + 2); i += 256) {
        const int ly = i / (VT + 2), lx = i % (VT + 2);
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        float n[3] = {0.f, 0.f, 0.f};
        const bool in = y >= 0 && x >= 0 && y < H && x < W;
        if (in) normal_of(P[ly][lx], P[ly + 1][lx], P[ly][lx + 1], n);
#pragma unroll
        for (int k = 0; k < 3; k++) N[k][ly][lx] = in ? half_map(n[k]) : 0.f;
    }
    __syncthreads();
    const int ty = threadIdx.x / VT, tx = threadIdx.x % VT;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) acc = edge_accumulate(acc, &N[k][ty][tx], VT + 3);
    const int y = y0 + ty, x = x0 + tx;
    const bool in = y < H && x < W;
    const float v = sqrtf(acc);
    if (in) out[(size_t)y * W + x] = v;
    if (minmax) block_minmax(in ? v : INFINITY, in ? v : -INFINITY, minmax);
}

__global__ void __launch_bounds__(256) view_minmax_kernel(size_t n, const float* __restrict__ field, float* __restrict__ minmax) {
    float lo = INFINITY, hi = -INFINITY;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = field[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax(lo, hi, minmax);
}

__device__ __forceinline__ unsigned char to_byte(float c) { return (unsigned char)(fminf(fmaxf(c, 0.f), 1.f) * 255.f); }

__global__ void __launch_bounds__(256) view_palette_kernel(size_t HW, const float* __restrict__ field, const float* __restrict__ minmax,
                                                           const float* __restrict__ lut, int L, int mode, float* __restrict__ out_float,
                                                           unsigned char* __restrict__ out_u8) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float v = field[p], lo = minmax[0], hi = minmax[1];
    float s = 0.f;
    if (mode == F3DGS_VIEW_PALETTE_MINMAX) {
        const float range = hi - lo;
        if (range > 0.f) s = rintf((v - lo) / range * (float)(L - 1));        // round half to even (torch.round)
    } else {
        if (hi != 0.f) s = truncf(v / hi * (float)L);
    }
    const int idx = (int)fminf(fmaxf(s, 0.f), (float)(L - 1));                // NaN -> 0
    const float r = lut[3 * idx], g = lut[3 * idx + 1], b = lut[3 * idx + 2];
    if (out_float) {
        out_float[p] = r;
        out_float[HW + p] = g;
        out_float[2 * HW + p] = b;
    }
    if (out_u8) {
        out_u8[3 * p] = to_byte(r);
        out_u8[3 * p + 1] = to_byte(g);
        out_u8[3 * p + 2] = to_byte(b);
    }
}

__global__ void __launch_bounds__(256) view_bytes_kernel(size_t HW, const float* __restrict__ image, unsigned char* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * p + k] = to_byte(image[k * HW + p]);
}

inline unsigned tiles_of(int H, int W, int* tiles_x) {
    *tiles_x = (W + VT - 1) / VT;
    return (unsigned)((size_t)*tiles_x * ((H + VT - 1) / VT));
}

hipError_t launch_view_normals(int H, int W, const float* depth, const float* proj, const double* inv, float* out, bool chw, bool half,
                               hipStream_t s) {
    int tx;
    const unsigned tiles = tiles_of(H, W, &tx);
    hipLaunchKernelGGL(view_normals_kernel, dim3(tiles), dim3(256), 0, s, H, W, tx, depth, proj, inv, out, chw ? 1 : 0, half ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_view_gradient(int Cn, int H, int W, const float* image, float* out, float* minmax, hipStream_t s) {
    int tx;
    const unsigned tiles = tiles_of(H, W, &tx);
    if (minmax) hipLaunchKernelGGL(view_minmax_init_kernel, dim3(1), dim3(64), 0, s, minmax);
    hipLaunchKernelGGL(view_gradient_kernel, dim3(tiles), dim3(256), 0, s, Cn, H, W, tx, image, out, minmax);
    return hipGetLastError();
}

hipError_t launch_view_curvature(int H, int W, const float* depth, const float* proj, const double* inv, float* out, float* minmax,
                                 hipStream_t s) {
    int tx;
    const unsigned tiles = tiles_of(H, W, &tx);
    if (minmax) hipLaunchKernelGGL(view_minmax_init_kernel, dim3(1), dim3(64), 0, s, minmax);
    hipLaunchKernelGGL(view_curvature_kernel, dim3(tiles), dim3(256), 0, s, H, W, tx, depth, proj, inv, out, minmax);
    return hipGetLastError();
}

hipError_t launch_view_minmax(size_t n, const float* field, float* minmax, hipStream_t s) {
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 2047) / 2048, 2048));
    hipLaunchKernelGGL(view_minmax_init_kernel, dim3(1), dim3(64), 0, s, minmax);
    hipLaunchKernelGGL(view_minmax_kernel, dim3(blocks), dim3(256), 0, s, n, field, minmax);
    return hipGetLastError();
}

hipError_t launch_view_palette(size_t HW, const float* field, const float* minmax, const float* lut, int L, int mode, float* out_float,
                               unsigned char* out_u8, hipStream_t s) {
    hipLaunchKernelGGL(view_palette_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, HW, field, minmax, lut, L, mode,
                       out_float, out_u8);
    return hipGetLastError();
}

hipError_t launch_view_bytes(size_t HW, const float* image, unsigned char* out, hipStream_t s) {
    hipLaunchKernelGGL(view_bytes_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, HW, image, out);
    return hipGetLastError();
}

// nullptr if the frame is served, else the reason
const char* view_unsupported(int H, int W, bool unprojects) {
    if ((long long)H * W > (1ll << 30)) return "view: %d x %d pixels: the frame is too large";
    if (unprojects && H > 0 && W > 0 && (H == 1 || W == 1))
        return "view: %d x %d pixels: normals need at least 2 rows and 2 columns (x / (W - 1), y / (H - 1))";
    return nullptr;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

int f3dgs_view_normals(int H, int W, const float* depth, const float* proj, const double* inv_full_proj, float* out, int flags,
                       void* stream) {
    if (H < 0 || W < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_normals: bad sizes H=%d W=%d", H, W);
    const int known = F3DGS_VIEW_NORMALS_CHW | F3DGS_VIEW_NORMALS_HALF;
    if (flags & ~known) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_normals: unknown flag bits 0x%x", flags & ~known);
    if (const char* why = view_unsupported(H, W, true)) return report_errorf(F3DGS_ERR_UNSUPPORTED, why, H, W);
    if (H == 0 || W == 0) return F3DGS_OK;
    if (!depth || !proj || !inv_full_proj || !out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_normals: null pointer");
    HIP_TRY(launch_view_normals(H, W, depth, proj, inv_full_proj, out, (flags & F3DGS_VIEW_NORMALS_CHW) != 0,
                                (flags & F3DGS_VIEW_NORMALS_HALF) != 0, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_view_gradient(int Cn, int H, int W, const float* image, float* out, float* minmax, void* stream) {
    if (Cn < 1 || H < 0 || W < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_gradient: bad sizes Cn=%d H=%d W=%d", Cn, H, W);
    if (const char* why = view_unsupported(H, W, false)) return report_errorf(F3DGS_ERR_UNSUPPORTED, why, H, W);
    if (H == 0 || W == 0) return F3DGS_OK;
    if (!image || !out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_gradient: null pointer");
    HIP_TRY(launch_view_gradient(Cn, H, W, image, out, minmax, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_view_curvature(int H, int W, const float* depth, const float* proj, const double* inv_full_proj, float* out, float* minmax,
                         void* stream) {
    if (H < 0 || W < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_curvature: bad sizes H=%d W=%d", H, W);
    if (const char* why = view_unsupported(H, W, true)) return report_errorf(F3DGS_ERR_UNSUPPORTED, why, H, W);
    if (H == 0 || W == 0) return F3DGS_OK;
    if (!depth || !proj || !inv_full_proj || !out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_curvature: null pointer");
    HIP_TRY(launch_view_curvature(H, W, depth, proj, inv_full_proj, out, minmax, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_view_minmax(long long n, const float* field, float* minmax, void* stream) {
    if (n < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_minmax: n = %lld", n);
    if (n > (1ll << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "view_minmax: %lld values: the field is too large", n);
    if (n == 0) return F3DGS_OK;
    if (!field || !minmax) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_minmax: null pointer");
    HIP_TRY(launch_view_minmax((size_t)n, field, minmax, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_view_palette(long long HW, const float* field, const float* minmax, const float* lut, int L, int mode, float* out_float,
                       uint8_t* out_u8, void* stream) {
    if (HW < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_palette: HW = %lld", HW);
    if (mode != F3DGS_VIEW_PALETTE_MINMAX && mode != F3DGS_VIEW_PALETTE_MAX)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_palette: unknown mode %d", mode);
    if (HW > (1ll << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "view_palette: %lld pixels: the frame is too large", HW);
    if (L < 2 || L > F3DGS_VIEW_PALETTE_MAX_ENTRIES)
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "view_palette: a palette of %d entries: supported are 2 to %d", L, F3DGS_VIEW_PALETTE_MAX_ENTRIES);
    if (HW == 0) return F3DGS_OK;
    if (!field || !minmax || !lut || (!out_float && !out_u8)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_palette: null pointer");
    HIP_TRY(launch_view_palette((size_t)HW, field, minmax, lut, L, mode, out_float, out_u8, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_view_bytes(long long HW, const float* image, uint8_t* out_u8, void* stream) {
    if (HW < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_bytes: HW = %lld", HW);
    if (HW > (1ll << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "view_bytes: %lld pixels: the frame is too large", HW);
    if (HW == 0) return F3DGS_OK;
    if (!image || !out_u8) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "view_bytes: null pointer");
    HIP_TRY(launch_view_bytes((size_t)HW, image, out_u8, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

}  // extern "C"
