// codebook.hip - feature codebooks (include/f3dgs.h: f3dgs_codebook_assign, f3dgs_codebook_update): the two halves of Lloyd's
// iteration over the per-Gaussian semantic features, for vector / product quantisation of the features and for clustering the
// Gaussians where no label map and no masks exist.
//
// f3dgs_codebook_assign is a (P x C) . (C x K) product with an arg-min epilogue; the (P, K) scores never exist.
//   codebook_prepare_kernel  one wave per centroid, fp64: |c_k|^2 rounded once (L2), or c_k / |c_k| rounded once and a zero
//                            offset (cosine) - NaN as the offset of a centroid with a non-finite element: its score is NaN and
//                            never wins.  Block 0 clears `inertia` and `moved`.
//   codebook_assign_kernel   a workgroup of four waves owns PT = 128 rows, wave w the rows 32 w .. 32 w + 31, and walks the
//                            centroids in tiles of KT = 128: per tile the channels in chunks of 32, both operands staged through
//                            LDS (rows >= P, centroids >= K and channels >= C as zeros), 16 k-steps of
//                            v_mfma_f32_32x32x2_f32 per chunk and 32-centroid sub-tile: centroids are the A operand (rows =
//                            accumulator registers), points the B operand (column = lane & 31), so that a lane holds 16 scores
//                            of ITS row per sub-tile and reduces them into a running (score, k) that it carries across all
//                            tiles; the two lane halves meet once, at the end.  A sub-tile entirely >= K is skipped.
//                            The chain of a score is the instruction's own: fmaf over the channels ascending from 0, lane half h
//                            supplying channel 2 s + h of k-step s - the LDS image of a chunk keeps the even channels of a row in
//                            its first 16 words and the odd ones in the next 16, so that a lane reads four k-steps with one
//                            16-byte load.  score = fmaf(-2, dot, |c|^2) (L2) or -dot (cosine): a function of the inputs alone.
//   codebook_finish_kernel   only with dist2 or inertia: 16 lanes per row recompute the winner's distance in fp64
// f3dgs_codebook_update: group_stats.hip's accumulation (group_sums.h) with the codes as ids, then one workgroup per centroid:
// the fp64 quotient (normalised in fp64 under the cosine metric) rounded once; an empty cluster keeps its row or is reseeded.
//
// Not done here: more than one row tile per wave, a second LDS buffer, a bf16 split of the operands.  Tried and dropped: the global
// loads of the next (tile, chunk) step issued into registers before the MFMAs of this one and stored to LDS after them - 244
// registers instead of 170 and 11 - 17 % slower at K = 4096 (profiles/codebook_bench.md).

#include <math.h>

#include "common.h"
#include "decoder_tile.h"      // f32x16, mfma_row (the tiling here is its own)
#include "group_sums.h"

namespace f3dgs {

namespace {

constexpr int PT = 128;            // rows of a workgroup
constexpr int KT = 128;            // centroids of a tile: four sub-tiles of 32, one accumulator each
constexpr int CH = 32;             // channels of a chunk: 16 k-steps
constexpr int LS = CH + 4;         // words of a row of the LDS image (16-byte reads of a lane, rows 144 bytes apart)
static_assert(F3DGS_CODEBOOK_MAX_CENTROIDS == F3DGS_GROUP_MAX_GROUPS && F3DGS_CODEBOOK_MAX_CHANNELS == F3DGS_GROUP_MAX_CHANNELS,
              "the update runs the codes through the group sums");

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) < INFINITY; }                  // (false for NaN)

size_t offsets_bytes(int K) { return (((size_t)K * sizeof(float)) + 15) & ~(size_t)15; }
size_t workspace_bytes(int K, int C) { return offsets_bytes(K) + (size_t)K * C * sizeof(float) + 16; }

// one wave per centroid
__global__ void __launch_bounds__(256) codebook_prepare_kernel(int K, int C, const float* __restrict__ centroids, int cosine,
                                                               float* __restrict__ offset, float* __restrict__ unit,
                                                               double* __restrict__ inertia, int32_t* __restrict__ moved) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (inertia) *inertia = 0.0;
        if (moved) *moved = 0;
    }
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;
    const float* const row = centroids + (size_t)k * C;
    double ss = 0.0;
    int bad = 0;
    for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        bad |= !finite32(v);
        ss += (double)v * (double)v;
    }
    bad = __any(bad);
    ss = wave_sum(ss);
    if (lane == 0) offset[k] = bad ? NAN : (cosine ? 0.f : (float)ss);
    if (cosine) {
        const double inv = (!bad && ss > 0.0) ? 1.0 / sqrt(ss) : 0.0;
        for (int c = lane; c < C; c += 64) unit[(size_t)k * C + c] = inv > 0.0 ? (float)((double)row[c] * inv) : 0.f;
    }
}

struct AssignJob {
    int P, K, C;
    const float* x;            // features
    int64_t xs;                // their row stride
    const float* cb;           // the centroids the scores are taken against (K x C): the caller's, or the unit rows
    const float* offset;       // K
    float mult;                // -2 (L2), -1 (cosine)
    int vec_x, vec_c;          // 16-byte loads of a row
    const int32_t* prev;       // or nullptr
    int32_t* codes;
    int32_t* moved;            // or nullptr
};

// rows row0 .. row0 + 127 x channels c0 .. c0 + 31 of a (n x C) matrix into the LDS image, zeros outside; with s_bad, a row
// that holds a non-finite element is marked there
__device__ __forceinline__ void stage(float* dst, const float* src, int64_t stride, int n, int C, int row0, int c0, bool vec, int* s_bad) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int at = t * 256 + threadIdx.x;
        const int row = at >> 3, g = at & 7, c = c0 + 4 * g;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (row0 + row < n && c < C) {
            const float* p = src + (size_t)(row0 + row) * (size_t)stride + c;
            if (vec) {                                                       // (C % 4 == 0: all four or none)
                const float4 q = *reinterpret_cast<const float4*>(p);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (c + q < C) v[q] = p[q];
            }
        }
        if (s_bad && !(finite32(v[0]) && finite32(v[1]) && finite32(v[2]) && finite32(v[3]))) s_bad[row] = 1;
        float* const d = dst + row * LS + 2 * g;
        *reinterpret_cast<float2*>(d) = make_float2(v[0], v[2]);            // channels 2 s of the chunk
        *reinterpret_cast<float2*>(d + CH / 2) = make_float2(v[1], v[3]);   // channels 2 s + 1
    }
}

// (two workgroups per CU: 170 registers, nothing spilled; three would spill)
__global__ void __launch_bounds__(256, 2) codebook_assign_kernel(AssignJob a) {
    __shared__ __attribute__((aligned(16))) float s_c[KT * LS];
    __shared__ __attribute__((aligned(16))) float s_x[PT * LS];
    __shared__ float s_off[KT];
    __shared__ int s_bad[PT];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * PT;                                        // (P < 2^31 - PT is checked by the entry)
    if (threadIdx.x < PT) s_bad[threadIdx.x] = 0;
    float best = INFINITY;
    int best_k = -1;
    for (int k0 = 0; k0 < a.K; k0 += KT) {
        const int tiles = min(4, (a.K - k0 + 31) >> 5);                      // sub-tiles that hold a centroid
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[t][i] = 0.f;
        for (int c0 = 0; c0 < a.C; c0 += CH) {
            __syncthreads();                                                 // the image is free (and s_bad is cleared)
            stage(s_c, a.cb, a.C, a.K, a.C, k0, c0, a.vec_c != 0, nullptr);
            stage(s_x, a.x, a.xs, a.P, a.C, row0, c0, a.vec_x != 0, k0 == 0 ? s_bad : nullptr);
            if (c0 == 0 && threadIdx.x < KT) s_off[threadIdx.x] = k0 + (int)threadIdx.x < a.K ? a.offset[k0 + threadIdx.x] : NAN;
            __syncthreads();
            const float* const xrow = s_x + (32 * wave + r) * LS + (CH / 2) * h;
            const float* const crow = s_c + r * LS + (CH / 2) * h;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 b = *reinterpret_cast<const float4*>(xrow + 4 * q);
                float4 av[4];
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (t < tiles) av[t] = *reinterpret_cast<const float4*>(crow + t * 32 * LS + 4 * q);
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (t < tiles) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].x, b.x, acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (t < tiles) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].y, b.y, acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (t < tiles) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].z, b.z, acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; t++)
                    if (t < tiles) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t].w, b.w, acc[t], 0, 0, 0);
            }
        }
        // the lane's own 16 scores per sub-tile, k ascending: a strict comparison keeps the lowest k of a tie
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (t >= tiles) continue;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int kl = 32 * t + mfma_row(i, h);
                const float s = fmaf(a.mult, acc[t][i], s_off[kl]);          // (NaN for k >= K and for a non-finite centroid)
                if (s < best) {
                    best = s;
                    best_k = k0 + kl;
                }
            }
        }
    }
    const float other = __shfl_xor(best, 32, 64);
    const int other_k = __shfl_xor(best_k, 32, 64);
    if (other_k >= 0 && (best_k < 0 || other < best || (other == best && other_k < best_k))) best_k = other_k;
    __syncthreads();                                                         // (K >= 1, C >= 1: s_bad is complete)
    const int row = row0 + 32 * wave + r;
    bool differs = false;
    if (h == 0 && row < a.P) {
        const int code = s_bad[32 * wave + r] ? -1 : best_k;
        if (a.prev) differs = a.prev[row] != code;                           // (codes may be prev: read before the store)
        a.codes[row] = code;
    }
    if (a.moved) {
        const int n = __popcll(__ballot(differs));
        if (lane == 0 && n) atomicAdd(a.moved, n);
    }
}

// 16 lanes per row, 16 rows a round, FINISH_ROUNDS rounds a workgroup: the winner's distance again, in fp64; one atomic per
// workgroup (one per 16 rows took longer than everything else at small K)
constexpr int FINISH_ROUNDS = 16;
__global__ void __launch_bounds__(256) codebook_finish_kernel(int P, int C, const float* __restrict__ x, int64_t xs,
                                                              const float* __restrict__ centroids, int cosine,
                                                              const int32_t* __restrict__ codes, const float* __restrict__ weight,
                                                              float* __restrict__ dist2, double* __restrict__ inertia) {
    __shared__ double s_part[16];
    const int sub = threadIdx.x >> 4, l = threadIdx.x & 15;
    double mine = 0.0;                                                       // lane 0 of a sub-group: its rows' w * dist2
    for (int round = 0; round < FINISH_ROUNDS; round++) {
        const size_t row = ((size_t)blockIdx.x * FINISH_ROUNDS + round) * 16 + sub;
        double d = 0.0, xx = 0.0, cc = 0.0;
        int k = -1;
        if (row < (size_t)P) k = codes[row];
        if (k >= 0) {
            const float* const xr = x + row * (size_t)xs;
            const float* const cr = centroids + (size_t)k * C;
            for (int c = l; c < C; c += 16) {
                const double xv = (double)xr[c], cv = (double)cr[c];
                if (cosine) {
                    d += xv * cv;
                    xx += xv * xv;
                    cc += cv * cv;
                } else {
                    const double e = xv - cv;
                    d += e * e;
                }
            }
        }
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1) {
            d += __shfl_xor(d, s, 64);
            xx += __shfl_xor(xx, s, 64);
            cc += __shfl_xor(cc, s, 64);
        }
        if (cosine) d = k < 0 ? 0.0 : 1.0 - ((xx > 0.0 && cc > 0.0) ? d / sqrt(xx * cc) : 0.0);
        const float df = (float)d;
        if (l == 0 && row < (size_t)P) {
            if (dist2) dist2[row] = df;
            const float w = (k >= 0) ? (weight ? weight[row] : 1.f) : 0.f;
            if (w > 0.f && w < INFINITY) mine += (double)w * (double)df;
        }
    }
    if (!inertia) return;
    if (l == 0) s_part[sub] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int i = 0; i < 16; i++) sum += s_part[i];
        if (sum != 0.0) atomicAdd(inertia, sum);
    }
}

// one workgroup per centroid
__global__ void __launch_bounds__(256) codebook_move_kernel(int P, int K, int C, GroupSums sums, const float* __restrict__ x, int64_t xs,
                                                            int cosine, int reseed, unsigned long long iteration,
                                                            float* __restrict__ centroids, int32_t* __restrict__ count) {
    __shared__ double s_part[4];
    const int k = blockIdx.x;
    const double m = sums.mass[k];
    if (threadIdx.x == 0 && count) count[k] = (int32_t)sums.count[k];
    float* const out = centroids + (size_t)k * C;
    if (m > 0.0) {
        const double* const f = sums.feat + (size_t)k * C;
        double scale = 1.0;
        if (cosine) {
            double ss = 0.0;
            for (int c = threadIdx.x; c < C; c += 256) {
                const double v = f[c] / m;
                ss += v * v;
            }
            ss = wave_sum(ss);
            if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = ss;
            __syncthreads();
            ss = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
            if (ss > 0.0 && ss < (double)INFINITY) scale = 1.0 / sqrt(ss);   // (a zero or non-finite mean stays as it is)
        }
        for (int c = threadIdx.x; c < C; c += 256) out[c] = (float)(scale == 1.0 ? f[c] / m : (f[c] / m) * scale);
    } else if (reseed && P > 0) {
        const unsigned long long row = ((unsigned long long)k * 2654435761ull + iteration * 40503ull) % (unsigned long long)P;
        const float* const xr = x + (size_t)row * (size_t)xs;
        int bad = 0;
        for (int c = threadIdx.x; c < C; c += 256) bad |= !finite32(xr[c]);
        if (__syncthreads_or(bad)) return;                                   // the cluster keeps its centroid
        for (int c = threadIdx.x; c < C; c += 256) out[c] = xr[c];
    }
}

unsigned blocks_for(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_codebook_workspace_bytes(int K, int C) {
    return workspace_bytes(std::min(std::max(K, 0), F3DGS_CODEBOOK_MAX_CENTROIDS), std::min(std::max(C, 0), F3DGS_CODEBOOK_MAX_CHANNELS));
}

int f3dgs_codebook_assign(int P, int K, int C, const float* features, int64_t feature_stride, const float* centroids, int flags,
                          const int32_t* prev_codes, const float* weight, int32_t* codes, float* dist2, double* inertia, int32_t* moved,
                          void* workspace, size_t workspace_bytes_given, void* stream) {
    const char* who = "f3dgs_codebook_assign";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (K < 1 || K > F3DGS_CODEBOOK_MAX_CENTROIDS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: K = %d centroids, 1 .. %d are taken", who, K, F3DGS_CODEBOOK_MAX_CENTROIDS);
    if (C < 1 || C > F3DGS_CODEBOOK_MAX_CHANNELS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: C = %d channels, 1 .. %d are taken", who, C, F3DGS_CODEBOOK_MAX_CHANNELS);
    if (flags & ~F3DGS_CODEBOOK_COSINE) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: flags = %d, only F3DGS_CODEBOOK_COSINE is taken", who, flags);
    if (feature_stride < C)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: feature_stride = %lld below C = %d", who, (long long)feature_stride, C);
    if (!centroids) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (centroids)", who);
    if (P > 0 && (!features || !codes)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (features, codes)", who);
    if (moved && !prev_codes && P > 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: moved needs prev_codes", who);
    if (P > INT32_MAX - PT) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^31 - %d rows", who, PT + 1);
    if (!workspace || workspace_bytes_given < f3dgs_codebook_workspace_bytes(K, C))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: workspace of %zu bytes, %zu are needed", who, workspace ? workspace_bytes_given : (size_t)0,
                             f3dgs_codebook_workspace_bytes(K, C));
    if (!aligned16(workspace)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
    if ((reinterpret_cast<uintptr_t>(inertia) & 7u)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: inertia must be 8-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int cosine = (flags & F3DGS_CODEBOOK_COSINE) ? 1 : 0;
    float* const offset = static_cast<float*>(workspace);
    float* const unit = reinterpret_cast<float*>(static_cast<char*>(workspace) + offsets_bytes(K));
    hipLaunchKernelGGL(codebook_prepare_kernel, dim3(blocks_for((size_t)K, 4)), dim3(256), 0, st, K, C, centroids, cosine, offset, unit, inertia,
                       moved);
    if (P > 0) {
        AssignJob a{};
        a.P = P, a.K = K, a.C = C;
        a.x = features, a.xs = feature_stride;
        a.cb = cosine ? unit : centroids;
        a.offset = offset;
        a.mult = cosine ? -1.f : -2.f;
        a.vec_x = C % 4 == 0 && feature_stride % 4 == 0 && aligned16(features);
        a.vec_c = C % 4 == 0 && aligned16(a.cb);
        a.prev = prev_codes, a.codes = codes, a.moved = moved;
        hipLaunchKernelGGL(codebook_assign_kernel, dim3(blocks_for((size_t)P, PT)), dim3(256), 0, st, a);
        if (dist2 || inertia)
            hipLaunchKernelGGL(codebook_finish_kernel, dim3(blocks_for((size_t)P, 16 * FINISH_ROUNDS)), dim3(256), 0, st, P, C, features, feature_stride, centroids,
                               cosine, codes, weight, dist2, inertia);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

size_t f3dgs_codebook_update_scratch_bytes(int K, int C) {
    return group_feature_sums_bytes(std::min(std::max(K, 0), F3DGS_CODEBOOK_MAX_CENTROIDS), std::min(std::max(C, 0), F3DGS_CODEBOOK_MAX_CHANNELS));
}

int f3dgs_codebook_update(int P, int K, int C, const float* features, int64_t feature_stride, const int32_t* codes, const float* weight,
                          int flags, int iteration, float* centroids, int32_t* count, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "f3dgs_codebook_update";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (K < 1 || K > F3DGS_CODEBOOK_MAX_CENTROIDS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: K = %d centroids, 1 .. %d are taken", who, K, F3DGS_CODEBOOK_MAX_CENTROIDS);
    if (C < 1 || C > F3DGS_CODEBOOK_MAX_CHANNELS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: C = %d channels, 1 .. %d are taken", who, C, F3DGS_CODEBOOK_MAX_CHANNELS);
    if (flags & ~(F3DGS_CODEBOOK_COSINE | F3DGS_CODEBOOK_RESEED_EMPTY))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: flags = %d, F3DGS_CODEBOOK_COSINE | F3DGS_CODEBOOK_RESEED_EMPTY are taken", who, flags);
    if (iteration < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: iteration < 0", who);
    if (feature_stride < C)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: feature_stride = %lld below C = %d", who, (long long)feature_stride, C);
    if (!centroids) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (centroids)", who);
    if (P > 0 && (!features || !codes)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (features, codes)", who);
    if (!scratch || scratch_bytes < f3dgs_codebook_update_scratch_bytes(K, C))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch of %zu bytes, %zu are needed", who, scratch ? scratch_bytes : (size_t)0,
                             f3dgs_codebook_update_scratch_bytes(K, C));
    if (reinterpret_cast<uintptr_t>(scratch) & 7u) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 8-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupSums sums = launch_group_feature_sums(P, K, C, codes, weight, features, feature_stride, scratch, st);
    hipLaunchKernelGGL(codebook_move_kernel, dim3((unsigned)K), dim3(256), 0, st, P, K, C, sums, features, feature_stride,
                       (flags & F3DGS_CODEBOOK_COSINE) ? 1 : 0, (flags & F3DGS_CODEBOOK_RESEED_EMPTY) ? 1 : 0, (unsigned long long)iteration,
                       centroids, count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
