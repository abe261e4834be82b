// model_front.hip - the glue between a model's raw parameters and the op (include/f3dgs.h: f3dgs_activate_forward,
// f3dgs_activate_backward, f3dgs_densify_stats), one launch each.
//
// Reference: scene/gaussian_model.py:98-127 (the getters every render() call runs: exp, F.normalize, sigmoid and the cat of
// the two SH tensors) with autograd's mirror of each, and train.py:132-133 / scene/gaussian_model.py:436-438 (the
// densification statistics, written there with boolean-mask indexing: a nonzero and a host read per mask).
//
// A workgroup owns FRONT_ROWS consecutive Gaussians.  The activations are element-wise.  The SH pack is a copy between two
// layouts whose rows do not line up (a `features_rest` row is 180 bytes at degree 3, an `shs` row 192): it goes through an
// LDS tile that holds a run of whole rows in the PACKED layout - the split side is read or written with consecutive dwords
// across the wave, the packed side with 16-byte accesses.  At 1M Gaussians the pack moves what torch.cat moves; what the
// kernels save is launches, host reads and the copies autograd keeps, not bytes.
#include "common.h"

namespace f3dgs {

namespace {

constexpr int FRONT_THREADS = 256;
constexpr int FRONT_ROWS = 256;             // Gaussians per workgroup
constexpr int FRONT_TILE_FLOATS = 3072;     // the LDS tile: 64 rows at M = 16 (12 KB, eight workgroups per CU)
constexpr int FRONT_UNROLL = 4;             // independent loads in flight per thread while a tile is staged
constexpr float NORMALIZE_EPS = 1e-12f;     // F.normalize's default eps

// rows of 3 M floats per tile: a multiple of four, so that every tile starts 16-byte aligned in the packed tensor
__host__ __device__ inline int tile_rows(int M) {
    const int r = (FRONT_TILE_FLOATS / (3 * M)) & ~3;
    return r > FRONT_ROWS ? FRONT_ROWS : r;
}

// e / w for e < 2^24 (tile-local indices): one float multiply, the estimate is off by at most one (densify.hip)
__device__ inline uint32_t div_small(uint32_t e, uint32_t w, float inv_w) {
    const uint32_t r = (uint32_t)(((float)e + 0.5f) * inv_w);
    return r * w > e ? r - 1 : (r * w + w <= e ? r + 1 : r);
}

__device__ inline bool vec4_ok(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ inline float4 load4(const float* p, bool aligned) {
    if (aligned) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ inline void store4(float* p, bool aligned, float4 v) {
    if (aligned) {
        *reinterpret_cast<float4*>(p) = v;
    } else {
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
    }
}

struct FrontForward {
    int P, M;
    const float* raw_scaling;
    const float* raw_rotation;
    const float* raw_opacity;
    const float* features_dc;
    const float* features_rest;
    float* scales;
    float* rotations;
    float* opacities;
    float* shs;
};

struct FrontBackward {
    int P, M;
    const float* scales;
    const float* raw_rotation;
    const float* opacities;
    const float* dL_dscale;
    const float* dL_drot;
    const float* dL_dopacity;
    const float* dL_dsh;
    float* d_raw_scaling;
    float* d_raw_rotation;
    float* d_raw_opacity;
    float* d_features_dc;
    float* d_features_rest;
};

// `n` consecutive floats of a split source (rows of `w` floats) into columns [col0, col0 + w) of the packed tile rows
__device__ inline void stage_split(float* tile, const float* __restrict__ src, uint32_t n, uint32_t w, uint32_t col0, uint32_t W) {
    const float inv_w = 1.0f / (float)w;
    for (uint32_t i = threadIdx.x; i < n; i += FRONT_THREADS * FRONT_UNROLL) {
        float v[FRONT_UNROLL];
#pragma unroll
        for (int k = 0; k < FRONT_UNROLL; k++) {
            const uint32_t j = i + k * FRONT_THREADS;
            v[k] = j < n ? src[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < FRONT_UNROLL; k++) {
            const uint32_t j = i + k * FRONT_THREADS;
            if (j < n) {
                const uint32_t r = div_small(j, w, inv_w);
                tile[r * W + col0 + (j - r * w)] = v[k];
            }
        }
    }
}

// the reverse: columns [col0, col0 + w) of the packed tile rows out to `n` consecutive floats
__device__ inline void unstage_split(const float* tile, float* __restrict__ dst, uint32_t n, uint32_t w, uint32_t col0, uint32_t W) {
    const float inv_w = 1.0f / (float)w;
    for (uint32_t j = threadIdx.x; j < n; j += FRONT_THREADS) {
        const uint32_t r = div_small(j, w, inv_w);
        dst[j] = tile[r * W + col0 + (j - r * w)];
    }
}

__global__ void __launch_bounds__(FRONT_THREADS) activate_forward_kernel(FrontForward a) {
    __shared__ float4 s_tile4[FRONT_TILE_FLOATS / 4];
    float* s_tile = reinterpret_cast<float*>(s_tile4);
    const size_t row0 = (size_t)blockIdx.x * FRONT_ROWS;
    const int rows = (int)((size_t)a.P - row0 < (size_t)FRONT_ROWS ? (size_t)a.P - row0 : (size_t)FRONT_ROWS);
    const int tid = threadIdx.x;

    if (a.scales) {
        const float* __restrict__ in = a.raw_scaling + row0 * 3;
        float* __restrict__ out = a.scales + row0 * 3;
        for (int e = tid; e < rows * 3; e += FRONT_THREADS) out[e] = expf(in[e]);
    }
    if (a.opacities && tid < rows) a.opacities[row0 + tid] = 1.0f / (1.0f + expf(-a.raw_opacity[row0 + tid]));
    if (a.rotations && tid < rows) {
        const float4 q = load4(a.raw_rotation + (row0 + tid) * 4, vec4_ok(a.raw_rotation));
        const float n = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), NORMALIZE_EPS);
        reinterpret_cast<float4*>(a.rotations)[row0 + tid] = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
    }
    if (a.shs) {
        const uint32_t W = 3u * (uint32_t)a.M, WR = W - 3u;
        const int RT = tile_rows(a.M);
        for (int t0 = 0; t0 < rows; t0 += RT) {
            const int rt = rows - t0 < RT ? rows - t0 : RT;
            const size_t r0 = row0 + t0;
            stage_split(s_tile, a.features_dc + r0 * 3, (uint32_t)rt * 3u, 3u, 0u, W);
            if (WR) stage_split(s_tile, a.features_rest + r0 * WR, (uint32_t)rt * WR, WR, 3u, W);
            __syncthreads();
            const uint32_t n = (uint32_t)rt * W, n4 = n / 4;
            float* __restrict__ out = a.shs + r0 * W;           // 16-byte aligned: r0 is a multiple of four rows
            for (uint32_t v = tid; v < n4; v += FRONT_THREADS) reinterpret_cast<float4*>(out)[v] = s_tile4[v];
            for (uint32_t e = n4 * 4 + tid; e < n; e += FRONT_THREADS) out[e] = s_tile[e];      // the last rows of the tensor
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(FRONT_THREADS) activate_backward_kernel(FrontBackward a) {
    __shared__ float4 s_tile4[FRONT_TILE_FLOATS / 4];
    float* s_tile = reinterpret_cast<float*>(s_tile4);
    const size_t row0 = (size_t)blockIdx.x * FRONT_ROWS;
    const int rows = (int)((size_t)a.P - row0 < (size_t)FRONT_ROWS ? (size_t)a.P - row0 : (size_t)FRONT_ROWS);
    const int tid = threadIdx.x;

    if (a.d_raw_scaling) {
        float* __restrict__ out = a.d_raw_scaling + row0 * 3;
        for (int e = tid; e < rows * 3; e += FRONT_THREADS)
            out[e] = a.dL_dscale ? a.dL_dscale[row0 * 3 + e] * a.scales[row0 * 3 + e] : 0.f;
    }
    if (a.d_raw_opacity && tid < rows) {
        float d = 0.f;
        if (a.dL_dopacity) {
            const float o = a.opacities[row0 + tid];
            d = (a.dL_dopacity[row0 + tid] * (1.0f - o)) * o;
        }
        a.d_raw_opacity[row0 + tid] = d;
    }
    if (a.d_raw_rotation && tid < rows) {
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.dL_drot) {
            const float4 g = load4(a.dL_drot + (row0 + tid) * 4, vec4_ok(a.dL_drot));
            const float4 q = load4(a.raw_rotation + (row0 + tid) * 4, vec4_ok(a.raw_rotation));
            const float n = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
            if (n >= NORMALIZE_EPS) {
                const float4 h = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
                const float dot = h.x * g.x + h.y * g.y + h.z * g.z + h.w * g.w;
                d = make_float4((g.x - h.x * dot) / n, (g.y - h.y * dot) / n, (g.z - h.z * dot) / n, (g.w - h.w * dot) / n);
            } else {        // the clamp is active: the forward divided by the constant
                d = make_float4(g.x / NORMALIZE_EPS, g.y / NORMALIZE_EPS, g.z / NORMALIZE_EPS, g.w / NORMALIZE_EPS);
            }
        }
        store4(a.d_raw_rotation + (row0 + tid) * 4, vec4_ok(a.d_raw_rotation), d);
    }
    if (a.d_features_dc || a.d_features_rest) {
        const uint32_t W = 3u * (uint32_t)a.M, WR = W - 3u;
        if (!a.dL_dsh) {
            if (a.d_features_dc)
                for (int e = tid; e < rows * 3; e += FRONT_THREADS) a.d_features_dc[row0 * 3 + e] = 0.f;
            if (a.d_features_rest)
                for (uint32_t e = tid; e < (uint32_t)rows * WR; e += FRONT_THREADS) a.d_features_rest[row0 * WR + e] = 0.f;
            return;
        }
        const int RT = tile_rows(a.M);
        for (int t0 = 0; t0 < rows; t0 += RT) {
            const int rt = rows - t0 < RT ? rows - t0 : RT;
            const size_t r0 = row0 + t0;
            const uint32_t n = (uint32_t)rt * W, n4 = n / 4;
            const float* __restrict__ in = a.dL_dsh + r0 * W;   // 16-byte aligned: r0 is a multiple of four rows
            for (uint32_t i = tid; i < n4; i += FRONT_THREADS * FRONT_UNROLL) {
                float4 v[FRONT_UNROLL];
#pragma unroll
                for (int k = 0; k < FRONT_UNROLL; k++) {
                    const uint32_t j = i + k * FRONT_THREADS;
                    v[k] = j < n4 ? reinterpret_cast<const float4*>(in)[j] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int k = 0; k < FRONT_UNROLL; k++) {
                    const uint32_t j = i + k * FRONT_THREADS;
                    if (j < n4) s_tile4[j] = v[k];
                }
            }
            for (uint32_t e = n4 * 4 + tid; e < n; e += FRONT_THREADS) s_tile[e] = in[e];
            __syncthreads();
            if (a.d_features_dc) unstage_split(s_tile, a.d_features_dc + r0 * 3, (uint32_t)rt * 3u, 3u, 0u, W);
            if (a.d_features_rest && WR) unstage_split(s_tile, a.d_features_rest + r0 * WR, (uint32_t)rt * WR, WR, 3u, W);
            __syncthreads();
        }
    }
}

// One thread per Gaussian.  The norm and the sum are formed in fp64 and rounded once, so the accumulator is the correctly
// rounded fp32 value of  accum + sqrt(gx^2 + gy^2)  (an fp32 chain would carry three roundings into it).
__global__ void __launch_bounds__(FRONT_THREADS)
densify_stats_kernel(int P, const float* __restrict__ dL_dmean2D, const int32_t* __restrict__ radii, float* __restrict__ accum,
                     float* __restrict__ denom, float* __restrict__ max_radii2D) {
    const size_t i = (size_t)blockIdx.x * FRONT_THREADS + threadIdx.x;
    if (i >= (size_t)P) return;
    const int32_t r = radii[i];
    if (r <= 0) return;
    if (accum && dL_dmean2D) {
        const double gx = dL_dmean2D[i * 3], gy = dL_dmean2D[i * 3 + 1];
        accum[i] = (float)((double)accum[i] + sqrt(gx * gx + gy * gy));
    }
    if (denom) denom[i] += 1.0f;
    if (max_radii2D) max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
}

int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

int f3dgs_activate_forward(int P, int M, const float* raw_scaling, const float* raw_rotation, const float* raw_opacity,
                           const float* features_dc, const float* features_rest, float* scales, float* rotations, float* opacities,
                           float* shs, void* stream) {
    const char* who = "f3dgs_activate_forward";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (M < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: M = %d, at least 1 (the DC coefficient)", who, M);
    if (P == 0) return F3DGS_OK;
    if (shs && 3 * (int64_t)M * 4 > FRONT_TILE_FLOATS)
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: M = %d, at most %d coefficients", who, M, FRONT_TILE_FLOATS / 12);
    if ((scales && !raw_scaling) || (rotations && !raw_rotation) || (opacities && !raw_opacity) || (shs && !features_dc) ||
        (shs && M > 1 && !features_rest))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null input of a group whose output was requested", who);
    if (!aligned16(rotations) || !aligned16(shs))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: rotations and shs must be 16-byte aligned (f3dgs.h, Alignment)", who);
    if (!scales && !rotations && !opacities && !shs) return F3DGS_OK;
    const FrontForward a{P, M, raw_scaling, raw_rotation, raw_opacity, features_dc, features_rest, scales, rotations, opacities, shs};
    const unsigned blocks = (unsigned)(((size_t)P + FRONT_ROWS - 1) / FRONT_ROWS);
    hipLaunchKernelGGL(activate_forward_kernel, dim3(blocks), dim3(FRONT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return launched(who);
}

int f3dgs_activate_backward(int P, int M, const float* scales, const float* raw_rotation, const float* opacities,
                            const float* dL_dscale, const float* dL_drot, const float* dL_dopacity, const float* dL_dsh,
                            float* d_raw_scaling, float* d_raw_rotation, float* d_raw_opacity, float* d_features_dc,
                            float* d_features_rest, void* stream) {
    const char* who = "f3dgs_activate_backward";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (M < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: M = %d, at least 1 (the DC coefficient)", who, M);
    if (P == 0) return F3DGS_OK;
    const bool sh = d_features_dc || (d_features_rest && M > 1);
    if (sh && 3 * (int64_t)M * 4 > FRONT_TILE_FLOATS)
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: M = %d, at most %d coefficients", who, M, FRONT_TILE_FLOATS / 12);
    if ((d_raw_scaling && dL_dscale && !scales) || (d_raw_rotation && dL_drot && !raw_rotation) ||
        (d_raw_opacity && dL_dopacity && !opacities))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null input of a group whose output was requested", who);
    if (sh && !aligned16(dL_dsh))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: dL_dsh must be 16-byte aligned (f3dgs.h, Alignment)", who);
    if (M == 1) d_features_rest = nullptr;      // no columns
    if (!d_raw_scaling && !d_raw_rotation && !d_raw_opacity && !d_features_dc && !d_features_rest) return F3DGS_OK;
    const FrontBackward a{P, M, scales, raw_rotation, opacities, dL_dscale, dL_drot, dL_dopacity, dL_dsh,
                          d_raw_scaling, d_raw_rotation, d_raw_opacity, d_features_dc, d_features_rest};
    const unsigned blocks = (unsigned)(((size_t)P + FRONT_ROWS - 1) / FRONT_ROWS);
    hipLaunchKernelGGL(activate_backward_kernel, dim3(blocks), dim3(FRONT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return launched(who);
}

int f3dgs_densify_stats(int P, const float* dL_dmean2D, const int32_t* radii, float* xyz_gradient_accum, float* denom,
                        float* max_radii2D, void* stream) {
    const char* who = "f3dgs_densify_stats";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (P == 0) return F3DGS_OK;
    if (!radii) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null radii", who);
    if (!xyz_gradient_accum && !denom && !max_radii2D) return F3DGS_OK;
    const unsigned blocks = (unsigned)(((size_t)P + FRONT_THREADS - 1) / FRONT_THREADS);
    hipLaunchKernelGGL(densify_stats_kernel, dim3(blocks), dim3(FRONT_THREADS), 0, static_cast<hipStream_t>(stream), P, dL_dmean2D, radii,
                       xyz_gradient_accum, denom, max_radii2D);
    return launched(who);
}

}  // extern "C"
