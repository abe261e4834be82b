// feature_pca.hip - PCA colour image of a (C,H,W) feature map: the moments of the L2-normalised sample pixels and the
// projection of every pixel onto three components, with the map read by kernels only and nothing of size C*HW allocated.
//
// Replaces the reference's feature_visualize_saving (render.py:38-53):
//     fmap = F.normalize(feature[None], dim=1);  f = fmap.permute(0, 2, 3, 1).reshape(-1, C)
//     pca = sklearn.decomposition.PCA(3).fit(f[::3].cpu().numpy())               # the host, every view
//     t = (f - mean) @ components.T;  q1, q99 = np.percentile(t[::3], [1, 99]);  ((t - q1) / (q99 - q1)).clamp(0, 1)
// Stages of the moments (n = ceil(HW / stride) samples, pixel s * stride of the flattened map; Z = the samples, normalised
// and centred, channel-major like the map itself):
//   pca_norm_kernel    inv[s] = 1 / max(||x_s||, 1e-12), one thread per sample
//   pca_sum_kernel     per (channel, chunk of samples): sum of x inv in float64
//   pca_mean_kernel    mean[c] in float64 (the result), its float32 rounding mu[c] (what Z is centred by) and the rest
//                      delta[c] = mean[c] - mu[c]
//   pca_gram_kernel    G = Z Z^T on v_mfma_f32_32x32x2_f32.  A workgroup = one pair (bi <= bj) of 64-channel blocks x one slab
//                      of samples; its four waves own the 32 x 32 quadrants of the 64 x 64 block (on the diagonal the
//                      quadrant below it is left out).  Both operands are rows of the map along the pixel axis: 64 samples
//                      of 64 (+ 64) channels are normalised and centred on their way into LDS, the next 64 in flight in
//                      registers during the MFMAs; channels beyond C and samples beyond the slab are zeros in LDS, never
//                      in memory.  The fp32 accumulator is emptied into a float64 one every 256 samples.
//   pca_cov_kernel     cov[i][j] = (sum over slabs of G - n delta_i delta_j) / (n - 1) in float64, both triangles
// No atomics anywhere: every sum has one owner and a fixed order, so two calls give the same bits.
// Projection: pca_project_kernel, one thread per pixel and one pass over its channels: ||x||^2 and x . c_k together, then
// t_k = (x . c_k) / max(||x||, 1e-12) - mu . c_k, written raw or - with lo / hi - as clamp((t - lo) / (hi - lo), 0, 1).

#include <math.h>

#include "common.h"
#include "decoder_tile.h"      // f32x16, mfma_row (the tiling here is its own)

namespace f3dgs {

namespace {

constexpr int PB = 64;           // channel block edge of a workgroup
constexpr int PK = 64;           // samples per stage
constexpr int PLD = PK + 4;      // LDS row stride: one b128 of padding, so that the b128 reads of 16 rows hit all banks evenly
constexpr int PFLUSH = 4;        // stages between two float64 flushes of the accumulator
constexpr int PSLAB = 1024;      // shortest slab (samples)
constexpr int PMAX_GROUPS = 1024;    // workgroups of the Gram kernel beyond which slabs grow instead
constexpr int PCHUNK = 16384;    // samples per workgroup of pca_sum_kernel

struct PcaGeom {
    size_t n;            // samples
    int nb, pairs;       // 64-channel blocks, block pairs bi <= bj
    int slabs;
    size_t slab_len;     // samples per slab, a multiple of PK
    int chunks;          // of pca_sum_kernel
};

PcaGeom pca_geom(int C, size_t HW, int stride) {
    PcaGeom g;
    g.n = (HW + (size_t)stride - 1) / (size_t)stride;
    g.nb = (C + PB - 1) / PB;
    g.pairs = g.nb * (g.nb + 1) / 2;
    const size_t most = (size_t)std::max(1, PMAX_GROUPS / g.pairs);
    size_t slabs = std::min<size_t>(std::max<size_t>(1, (g.n + PSLAB - 1) / PSLAB), most);
    g.slab_len = ((g.n + slabs - 1) / slabs + PK - 1) / PK * PK;
    g.slabs = (int)std::max<size_t>(1, (g.n + g.slab_len - 1) / g.slab_len);
    g.chunks = (int)std::max<size_t>(1, (g.n + PCHUNK - 1) / PCHUNK);
    return g;
}

struct PcaScratch {
    float* inv;          // n
    double* sum_part;    // chunks x C
    float* mu;           // C
    double* delta;       // C
    double* gram;        // slabs x pairs x 64 x 64
    static PcaScratch carve(char* base, int C, const PcaGeom& g, size_t* bytes) {
        Carver c(base);
        PcaScratch s;
        s.inv = c.take<float>(g.n);
        s.sum_part = c.take<double>((size_t)g.chunks * C);
        s.mu = c.take<float>(C);
        s.delta = c.take<double>(C);
        s.gram = c.take<double>((size_t)g.slabs * g.pairs * PB * PB);
        if (bytes) *bytes = c.total();
        return s;
    }
};

__global__ void __launch_bounds__(256) pca_norm_kernel(int C, size_t HW, size_t n, size_t stride, const float* __restrict__ fm,
                                                       float* __restrict__ inv) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const float* src = fm + s * stride;
    float ss = 0.f;
#pragma unroll 8
    for (int c = 0; c < C; c++) {
        const float x = src[(size_t)c * HW];
        ss = fmaf(x, x, ss);
    }
    inv[s] = 1.f / fmaxf(sqrtf(ss), 1e-12f);
}

// blockIdx.x = chunk of PCHUNK samples (up to 2^16 of them: more than grid.y holds), blockIdx.y = channel
__global__ void __launch_bounds__(256) pca_sum_kernel(int C, size_t HW, size_t n, size_t stride, const float* __restrict__ fm,
                                                      const float* __restrict__ inv, double* __restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const size_t s0 = (size_t)blockIdx.x * PCHUNK;
    const size_t s1 = s0 + PCHUNK < n ? s0 + PCHUNK : n;
    const float* src = fm + (size_t)c * HW;
    double acc = 0.0;
    for (size_t s = s0 + threadIdx.x; s < s1; s += 256) acc += (double)(src[s * stride] * inv[s]);
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * C + c] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ void __launch_bounds__(256) pca_mean_kernel(int C, int chunks, size_t n, const double* __restrict__ part,
                                                       double* __restrict__ mean, float* __restrict__ mu, double* __restrict__ delta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int k = 0; k < chunks; k++) s += part[(size_t)k * C + c];
    const double m = s / (double)n;
    const float f = (float)m;
    mean[c] = m;
    mu[c] = f;
    delta[c] = m - (double)f;
}

struct GramArgs {
    int C, nb, pairs;
    size_t HW, n, stride, slab_len;
    const float* fm;
    const float* inv;
    const float* mu;
    double* gram;
};

__global__ void __launch_bounds__(256) pca_gram_kernel(const GramArgs a) {
    __shared__ __attribute__((aligned(16))) float Z[2][PB][PLD];
    __shared__ float mus[2][PB];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, h = lane >> 5;
    // the pair: row bi of the upper triangle holds nb - bi blocks
    int bi = 0, rest = blockIdx.x;
    while (rest >= a.nb - bi) { rest -= a.nb - bi; bi++; }
    const int bj = bi + rest;
    const bool diag = bi == bj;
    const int qi = w >> 1, qj = w & 1;
    const bool idle = diag && qi > qj;           // the quadrant below the diagonal: its mirror image is computed
    const size_t s_begin = (size_t)blockIdx.y * a.slab_len;
    const size_t s_end = s_begin + a.slab_len < a.n ? s_begin + a.slab_len : a.n;
    const int nst = (int)((s_end - s_begin + PK - 1) / PK);
    const int col = lane, row0 = w;              // this thread stages sample `col` of channels row0 + 4 k of either block

    if (threadIdx.x < 2 * PB) {
        const int c = (threadIdx.x < PB ? bi : bj) * PB + (threadIdx.x & (PB - 1));
        mus[threadIdx.x >> 6][threadIdx.x & (PB - 1)] = c < a.C ? a.mu[c] : 0.f;
    }

    auto load = [&](int st, float (&v)[32], float& iv) {
        const size_t s = s_begin + (size_t)st * PK + col;
        const bool ok = s < s_end;
        iv = ok ? a.inv[s] : 0.f;
        const float* src = a.fm + (ok ? s * a.stride : 0);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int c = bi * PB + row0 + 4 * k;
            v[k] = (ok && c < a.C) ? src[(size_t)c * a.HW] : 0.f;
        }
        if (!diag) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int c = bj * PB + row0 + 4 * k;
                v[16 + k] = (ok && c < a.C) ? src[(size_t)c * a.HW] : 0.f;
            }
        }
    };
    auto store = [&](int st, const float (&v)[32], float iv) {
        const bool ok = s_begin + (size_t)st * PK + col < s_end;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int r = row0 + 4 * k;
            Z[0][r][col] = (ok && bi * PB + r < a.C) ? fmaf(v[k], iv, -mus[0][r]) : 0.f;
        }
        if (!diag) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int r = row0 + 4 * k;
                Z[1][r][col] = (ok && bj * PB + r < a.C) ? fmaf(v[16 + k], iv, -mus[1][r]) : 0.f;
            }
        }
    };

    f32x16 acc;
    double dacc[16];
#pragma unroll
    for (int r = 0; r < 16; r++) { acc[r] = 0.f; dacc[r] = 0.0; }
    float raw[32], iv;
    load(0, raw, iv);
    __syncthreads();                                         // mus
    const float* arow = &Z[0][qi * 32 + li][4 * h];
    const float* brow = &Z[diag ? 0 : 1][qj * 32 + li][4 * h];
    for (int st = 0; st < nst; st++) {
        store(st, raw, iv);
        __syncthreads();
        if (st + 1 < nst) load(st + 1, raw, iv);
        if (!idle) {
            // a lane's four values of a quad of steps are consecutive in LDS: step m contracts sample 8 q + m with 8 q + 4 + m
#pragma unroll
            for (int q = 0; q < PK / 8; q++) {
                const float4 av = *reinterpret_cast<const float4*>(arow + 8 * q);
                const float4 bv = *reinterpret_cast<const float4*>(brow + 8 * q);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            }
            if ((st + 1) % PFLUSH == 0 || st + 1 == nst) {
#pragma unroll
                for (int r = 0; r < 16; r++) { dacc[r] += (double)acc[r]; acc[r] = 0.f; }
            }
        }
        __syncthreads();
    }
    if (idle) return;
    double* out = a.gram + ((size_t)blockIdx.y * a.pairs + blockIdx.x) * (PB * PB);
#pragma unroll
    for (int r = 0; r < 16; r++) out[(qi * 32 + mfma_row(r, h)) * PB + qj * 32 + li] = dacc[r];
}

__global__ void __launch_bounds__(256) pca_cov_kernel(int C, int nb, int pairs, int slabs, size_t n, const double* __restrict__ gram,
                                                      const double* __restrict__ delta, double* __restrict__ cov) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)C * C) return;
    const int i = (int)(e / C), j = (int)(e - (size_t)i * C);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int bi = lo / PB, bj = hi / PB;
    const int pair = bi * nb - bi * (bi - 1) / 2 + (bj - bi);
    const double* src = gram + (size_t)pair * (PB * PB) + (lo % PB) * PB + (hi % PB);
    double s = 0.0;
    for (int k = 0; k < slabs; k++) s += src[(size_t)k * pairs * (PB * PB)];
    cov[e] = (s - (double)n * delta[lo] * delta[hi]) / (double)(n - 1);
}

__global__ void __launch_bounds__(256) pca_project_kernel(int C, size_t HW, const float* __restrict__ fm, const float* __restrict__ mean,
                                                          const float* __restrict__ comp, const float* __restrict__ lo,
                                                          const float* __restrict__ hi, float* __restrict__ out) {
    __shared__ double red[3][4];
    // mu . c_k in float64: every workgroup forms it for itself (3 C products)
    double m[3] = {0.0, 0.0, 0.0};
    for (int c = threadIdx.x; c < C; c += 256) {
        const double mu = (double)mean[c];
#pragma unroll
        for (int k = 0; k < 3; k++) m[k] += mu * (double)comp[(size_t)k * C + c];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        m[k] = wave_sum(m[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = m[k];
    }
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const float* src = fm + p;
    const float* c0 = comp;
    const float* c1 = comp + C;
    const float* c2 = comp + 2 * (size_t)C;
    float ss = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll 8
    for (int c = 0; c < C; c++) {
        const float x = src[(size_t)c * HW];
        ss = fmaf(x, x, ss);
        d0 = fmaf(x, c0[c], d0);
        d1 = fmaf(x, c1[c], d1);
        d2 = fmaf(x, c2[c], d2);
    }
    const double inv = (double)(1.f / fmaxf(sqrtf(ss), 1e-12f));
    const float d[3] = {d0, d1, d2};
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (float)(inv * (double)d[k] - (((red[k][0] + red[k][1]) + red[k][2]) + red[k][3]));
    if (lo) {
        const float l = *lo, range = *hi - l;
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = fminf(fmaxf((t[k] - l) / range, 0.f), 1.f);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) out[p * 3 + k] = t[k];
}

size_t feature_pca_scratch_bytes(int C, size_t HW, int stride) {
    size_t b = 0;
    PcaScratch::carve(nullptr, C, pca_geom(C, HW, stride), &b);
    return b;
}

hipError_t launch_feature_pca_moments(int C, size_t HW, int stride, const float* feature_map, double* mean, double* cov,
                                      char* scratch, hipStream_t s) {
    const PcaGeom g = pca_geom(C, HW, stride);
    const PcaScratch sc = PcaScratch::carve(scratch, C, g, nullptr);
    hipLaunchKernelGGL(pca_norm_kernel, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, s, C, HW, g.n, (size_t)stride, feature_map, sc.inv);
    hipLaunchKernelGGL(pca_sum_kernel, dim3(g.chunks, C), dim3(256), 0, s, C, HW, g.n, (size_t)stride, feature_map, sc.inv, sc.sum_part);
    hipLaunchKernelGGL(pca_mean_kernel, dim3((C + 255) / 256), dim3(256), 0, s, C, g.chunks, g.n, sc.sum_part, mean, sc.mu, sc.delta);
    GramArgs a;
    a.C = C; a.nb = g.nb; a.pairs = g.pairs;
    a.HW = HW; a.n = g.n; a.stride = (size_t)stride; a.slab_len = g.slab_len;
    a.fm = feature_map; a.inv = sc.inv; a.mu = sc.mu; a.gram = sc.gram;
    hipLaunchKernelGGL(pca_gram_kernel, dim3(g.pairs, g.slabs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pca_cov_kernel, dim3((unsigned)(((size_t)C * C + 255) / 256)), dim3(256), 0, s, C, g.nb, g.pairs, g.slabs, g.n,
                       sc.gram, sc.delta, cov);
    return hipGetLastError();
}

hipError_t launch_feature_pca_project(int C, size_t HW, const float* feature_map, const float* mean, const float* components,
                                      const float* lo, const float* hi, float* out, hipStream_t s) {
    hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, C, HW, feature_map, mean, components, lo,
                       hi, out);
    return hipGetLastError();
}

// nullptr if the shape is served, else the reason
const char* feature_pca_unsupported(int C, long long HW, int stride, bool moments) {
    if (C < 3) return "feature_pca: C = %d, at least 3 channels are needed for 3 components";
    if (C > F3DGS_FEATURE_PCA_MAX_CHANNELS) return "feature_pca: C = %d beyond the limit of 4096 channels";
    if (HW < 0 || HW > (1ll << 30)) return "feature_pca: C = %d: the map is too large";
    if (moments && stride < 1) return "feature_pca: C = %d: stride < 1";
    return nullptr;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_feature_pca_scratch_bytes(int C, long long HW, int stride) {
    if (feature_pca_unsupported(C, HW, stride, true) || HW == 0) return 0;
    return feature_pca_scratch_bytes(C, (size_t)HW, stride);
}

int f3dgs_feature_pca_moments(int C, long long HW, int stride, const float* feature_map, double* mean, double* cov, void* scratch,
                              void* stream) {
    if (const char* why = feature_pca_unsupported(C, HW, stride, true)) return report_errorf(F3DGS_ERR_UNSUPPORTED, why, C);
    if (HW == 0) return F3DGS_OK;
    const long long n = (HW + stride - 1) / stride;
    if (n < 3) return report_errorf(F3DGS_ERR_UNSUPPORTED, "feature_pca: %lld samples (HW = %lld, stride = %d), at least 3 are needed", n, HW, stride);
    if (!feature_map || !mean || !cov || !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "feature_pca_moments: null pointer");
    HIP_TRY(launch_feature_pca_moments(C, (size_t)HW, stride, feature_map, mean, cov, static_cast<char*>(scratch),
                                       static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_feature_pca_project(int C, long long HW, const float* feature_map, const float* mean, const float* components,
                              const float* lo, const float* hi, float* out, void* stream) {
    if (const char* why = feature_pca_unsupported(C, HW, 1, false)) return report_errorf(F3DGS_ERR_UNSUPPORTED, why, C);
    if ((lo == nullptr) != (hi == nullptr)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "feature_pca_project: lo and hi go together");
    if (HW == 0) return F3DGS_OK;
    if (!feature_map || !mean || !components || !out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "feature_pca_project: null pointer");
    HIP_TRY(launch_feature_pca_project(C, (size_t)HW, feature_map, mean, components, lo, hi, out, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

}  // extern "C"
