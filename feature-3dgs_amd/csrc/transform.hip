// transform.hip - object transforms (include/f3dgs.h: f3dgs_transform_gaussians): the Gaussians of every group moved, turned and
// scaled by the group's own similarity transform x' = s R (x - p) + p + t, in one launch: positions, quaternions, scales,
// precomputed covariances and the higher-order SH coefficients, band by band.
//
//   transform_table_kernel   one thread per group: the validity of its row, and - in fp64 - s R, p, p + t, q / |q|, ln s, s, s^2
//                            and the rotation matrices D_1 (3 x 3), D_2 (5 x 5), D_3 (7 x 7) of the SH bands in the rasterizer's
//                            basis (transform_table.h: the recursion of Ivanic and Ruedenberg in the entries of R).  A row of the
//                            table is written and read back by its own thread while the bands build on each other: no array
//                            in private memory.
//   transform_kernel<N_REST> a workgroup takes ROWS consecutive output rows.  A Gaussian's row is 12 to 180 bytes: a thread that
//                            read its own row would stride through memory, so every tensor of the chunk goes through LDS - read
//                            with consecutive lanes on consecutive floats (of the source rows: the gather form reads row
//                            src_rows[j], whole rows at a time; the loads of ALL the call's tensors are issued before the first
//                            is waited for), transformed by one thread per row out of LDS (an odd row length has no bank
//                            conflict), and written back the same way.  Every output element is one fp64
//                            chain of fused multiply-adds, rounded once.  A row that is not transformed keeps the bits it was
//                            read with; where output and input are the same array it is not stored at all.
// One shape for every (G, n_rest): n_rest is the template argument, the table row of a Gaussian is read through its group id -
// neighbouring rows mostly share an id (the coherent numbering of the lifters and the components), so the lanes of a wave read
// the same 8 bytes; random ids read G x 848 bytes through the caches and take no other path.

#include <math.h>

#include "common.h"
#include "transform_table.h"

namespace f3dgs {

namespace {

constexpr int ROWS = 256;            // output rows of a workgroup, one thread each

struct Job {
    int P, M, G;                     // input rows, output rows, groups
    int linear;                      // scales: multiply by s (otherwise add ln s)
    const int32_t* groups;
    const int32_t* src_rows;         // null: output row j is input row j
    const int32_t* status;
    const double* table;
    const float *xyz, *rot, *scales, *cov, *sh;
    float *xyz_out, *rot_out, *scales_out, *cov_out, *sh_out;
    int64_t sh_stride, sh_out_stride;
};

__global__ void __launch_bounds__(256) transform_table_kernel(int G, const float* __restrict__ quat, const float* __restrict__ scale,
                                                              const float* __restrict__ translation, const float* __restrict__ pivot,
                                                              double* table, int32_t* __restrict__ status) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    status[g] = tt_build_row(quat + (size_t)g * 4, scale[g], translation + (size_t)g * 3, pivot ? pivot + (size_t)g * 3 : nullptr,
                             table + (size_t)g * TT_ROW);
}

// c' = D c on one band: c the N x 3 coefficients of the thread's row in LDS, D (N x N) of the group
template <int N>
__device__ __forceinline__ void rotate_band(float* c, const double* __restrict__ D) {
    double v[N][3];
#pragma unroll
    for (int n = 0; n < N; n++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) v[n][ch] = (double)c[n * 3 + ch];
#pragma unroll
    for (int m = 0; m < N; m++) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int n = 0; n < N; n++) {
            const double d = D[m * N + n];
            a0 = fma(d, v[n][0], a0);
            a1 = fma(d, v[n][1], a1);
            a2 = fma(d, v[n][2], a2);
        }
        c[m * 3] = (float)a0, c[m * 3 + 1] = (float)a1, c[m * 3 + 2] = (float)a2;
    }
}

// One tensor of the chunk, W floats a row, in two steps.  fetch: W loads a thread - consecutive lanes on consecutive floats of the
// (source) rows -, every one of them issued before the first is used: no load stands behind a branch (an element beyond the chunk,
// or of a row of zeros, reads a valid address all the same - the chunk's last element, input row 0 - and drops it).  The kernel
// fetches ALL its tensors before it waits for one: a workgroup pays the memory latency once, not once per tensor.
template <int W>
__device__ __forceinline__ void fetch(const float* in, int64_t in_stride, int rows, const int* s_src, float (&v)[W]) {
    const int n = rows * W;                                                  // (>= W: the workgroup has a row)
#pragma unroll
    for (int k = 0; k < W; k++) {
        const int e = min(k * 256 + (int)threadIdx.x, n - 1);
        const int r = e / W, c = e - r * W;
        const int src = s_src[r] >> 1;                                       // (-1 >> 1 = -1: a row of zeros)
        const float x = in[(size_t)max(src, 0) * (size_t)in_stride + c];
        v[k] = src >= 0 ? x : 0.f;
    }
}

// pass: the fetched floats -> LDS -> f on the rows that move, one thread a row -> out, as they were fetched
template <int W, typename F>
__device__ __forceinline__ void pass(const float (&v)[W], const float* in, float* out, int64_t out_stride, size_t base, int rows,
                                     float* s_buf, const int* s_src, bool moves, F&& f) {
    const int n = rows * W;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const int e = k * 256 + (int)threadIdx.x;
        if (e < n) s_buf[e] = v[k];
    }
    __syncthreads();
    if (moves) f(s_buf + threadIdx.x * W);
    __syncthreads();
    const bool same = in == out;
#pragma unroll
    for (int k = 0; k < W; k++) {
        const int e = k * 256 + (int)threadIdx.x;
        if (e >= n) continue;
        const int r = e / W, c = e - r * W;
        if (same && !(s_src[r] & 1)) continue;                               // in place and not moved: the row is not touched
        out[(base + r) * (size_t)out_stride + c] = s_buf[e];
    }
    __syncthreads();
}

template <int N_REST>
__global__ void __launch_bounds__(256) transform_kernel(Job job) {
    constexpr int WIDEST = N_REST > 2 ? 3 * N_REST : 6;
    __shared__ float s_buf[ROWS * WIDEST];
    __shared__ int s_src[ROWS];                                              // source row << 1 | moves; -1: a row of zeros
    const size_t base = (size_t)blockIdx.x * ROWS;
    const int rows = (int)min((size_t)ROWS, (size_t)job.M - base);
    int g = -1, packed = -1;
    if ((int)threadIdx.x < rows) {
        const int src = job.src_rows ? job.src_rows[base + threadIdx.x] : (int)(base + threadIdx.x);
        if (src >= 0 && src < job.P) {
            const int id = job.groups[src];
            if (id >= 0 && id < job.G && job.status[id] == 0) g = id;
            packed = (int)(((uint32_t)src << 1) | (g >= 0 ? 1u : 0u));
        }
    }
    s_src[threadIdx.x] = packed;
    __syncthreads();
    const bool moves = g >= 0;
    const double* __restrict__ const T = job.table + (size_t)(moves ? g : 0) * TT_ROW;

    float v_xyz[3], v_rot[4], v_scales[3], v_cov[6], v_sh[N_REST > 0 ? N_REST * 3 : 1];
    if (job.xyz) fetch<3>(job.xyz, 3, rows, s_src, v_xyz);
    if (job.rot) fetch<4>(job.rot, 4, rows, s_src, v_rot);
    if (job.scales) fetch<3>(job.scales, 3, rows, s_src, v_scales);
    if (job.cov) fetch<6>(job.cov, 6, rows, s_src, v_cov);
    if constexpr (N_REST > 0) fetch<N_REST * 3>(job.sh, job.sh_stride, rows, s_src, v_sh);

    // the widest first: its 3 n_rest registers are free again before the bands are turned
    if constexpr (N_REST > 0)
        pass<N_REST * 3>(v_sh, job.sh, job.sh_out, job.sh_out_stride, base, rows, s_buf, s_src, moves, [&](float* c) {
            rotate_band<3>(c, T + TT_D1);
            if (N_REST >= 8) rotate_band<5>(c + 9, T + TT_D2);
            if (N_REST >= 15) rotate_band<7>(c + 24, T + TT_D3);
        });
    if (job.xyz)
        pass<3>(v_xyz, job.xyz, job.xyz_out, 3, base, rows, s_buf, s_src, moves, [&](float* x) {
            const double d0 = (double)x[0] - T[TT_PIVOT], d1 = (double)x[1] - T[TT_PIVOT + 1], d2 = (double)x[2] - T[TT_PIVOT + 2];
#pragma unroll
            for (int a = 0; a < 3; a++)
                x[a] = (float)fma(T[TT_SR + 3 * a], d0, fma(T[TT_SR + 3 * a + 1], d1, fma(T[TT_SR + 3 * a + 2], d2, T[TT_SHIFT + a])));
        });
    if (job.rot)
        pass<4>(v_rot, job.rot, job.rot_out, 4, base, rows, s_buf, s_src, moves, [&](float* q) {
            const double aw = T[TT_QUAT], ax = T[TT_QUAT + 1], ay = T[TT_QUAT + 2], az = T[TT_QUAT + 3];
            const double bw = q[0], bx = q[1], by = q[2], bz = q[3];
            q[0] = (float)fma(aw, bw, fma(-ax, bx, fma(-ay, by, -az * bz)));
            q[1] = (float)fma(aw, bx, fma(ax, bw, fma(ay, bz, -az * by)));
            q[2] = (float)fma(aw, by, fma(-ax, bz, fma(ay, bw, az * bx)));
            q[3] = (float)fma(aw, bz, fma(ax, by, fma(-ay, bx, az * bw)));
        });
    if (job.scales)
        pass<3>(v_scales, job.scales, job.scales_out, 3, base, rows, s_buf, s_src, moves, [&](float* s) {
            const bool linear = job.linear != 0;
            const double k = linear ? T[TT_S] : T[TT_LOG_S];
#pragma unroll
            for (int a = 0; a < 3; a++) s[a] = linear ? (float)((double)s[a] * k) : (float)((double)s[a] + k);
        });
    if (job.cov)
        pass<6>(v_cov, job.cov, job.cov_out, 6, base, rows, s_buf, s_src, moves, [&](float* c) {
            // (s R) Sigma (s R)^T, Sigma as xx xy xz yy yz zz
            const double S[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
            double A[3][3], MS[3][3];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) A[a][b] = T[TT_SR + 3 * a + b];
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int k = 0; k < 3; k++) MS[a][k] = fma(A[a][0], S[0][k], fma(A[a][1], S[1][k], A[a][2] * S[2][k]));
            int at = 0;
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = a; b < 3; b++) c[at++] = (float)fma(MS[a][0], A[b][0], fma(MS[a][1], A[b][1], MS[a][2] * A[b][2]));
        });
}

size_t table_bytes(int G) { return (size_t)G * TT_ROW * sizeof(double); }

// the floats [p, p + (rows - 1) stride + width) of an array; empty without rows
struct Span {
    const float* lo;
    const float* hi;
};
Span span_of(const float* p, int64_t rows, int64_t stride, int width) {
    if (!p || rows <= 0) return Span{nullptr, nullptr};
    return Span{p, p + (rows - 1) * stride + width};
}
bool overlap(Span a, Span b) { return a.lo && b.lo && a.lo < b.hi && b.lo < a.hi; }

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_transform_gaussians_scratch_bytes(int G) {
    return table_bytes(std::min(std::max(G, 0), F3DGS_GROUP_MAX_GROUPS)) + 8;           // (never 0)
}

int f3dgs_transform_gaussians(int P, int G, const float* quat, const float* scale, const float* translation, const float* pivot,
                              const int32_t* groups, const int32_t* src_rows, int M, const float* xyz, const float* rotations,
                              const float* scales, int scale_mode, const float* cov3d, const float* sh_rest, int n_rest,
                              int64_t sh_stride, float* xyz_out, float* rotations_out, float* scales_out, float* cov3d_out,
                              float* sh_rest_out, int64_t sh_out_stride, int32_t* status, void* scratch, size_t scratch_bytes,
                              void* stream) {
    const char* who = "f3dgs_transform_gaussians";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (G < 1 || G > F3DGS_GROUP_MAX_GROUPS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: G = %d groups, 1 .. %d are taken", who, G, F3DGS_GROUP_MAX_GROUPS);
    if (!quat || !scale || !translation || !status)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (quat, scale, translation, status)", who);
    if (P > (1 << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^30 Gaussians", who);
    if (src_rows && M < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: M < 0", who);
    if (n_rest != 0 && n_rest != 3 && n_rest != 8 && n_rest != 15)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: n_rest = %d, 0, 3, 8 and 15 are taken", who, n_rest);
    if (scale_mode != F3DGS_TRANSFORM_SCALES_LOG && scale_mode != F3DGS_TRANSFORM_SCALES_LINEAR)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scale_mode = %d", who, scale_mode);
    if ((n_rest > 0) != (sh_rest != nullptr))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: sh_rest and n_rest = %d do not agree", who, n_rest);
    if (!xyz && !rotations && !scales && !cov3d && !sh_rest)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: every input is NULL", who);
    if (!xyz != !xyz_out || !rotations != !rotations_out || !scales != !scales_out || !cov3d != !cov3d_out || !sh_rest != !sh_rest_out)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: an input without its output, or an output without its input", who);
    if (sh_rest && (sh_stride < 3 * n_rest || sh_out_stride < 3 * n_rest))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: sh_stride = %lld / sh_out_stride = %lld below 3 n_rest = %d", who,
                             (long long)sh_stride, (long long)sh_out_stride, 3 * n_rest);
    if (P > 0 && !groups) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (groups)", who);
    const int rows_out = src_rows ? M : P;
    {
        const float* in[5] = {xyz, rotations, scales, cov3d, sh_rest};
        float* out[5] = {xyz_out, rotations_out, scales_out, cov3d_out, sh_rest_out};
        const int width[5] = {3, 4, 3, 6, 3 * n_rest};
        const int64_t in_stride[5] = {3, 4, 3, 6, sh_stride}, out_stride[5] = {3, 4, 3, 6, sh_out_stride};
        for (int a = 0; a < 5; a++) {
            if (!in[a]) continue;
            if (!src_rows && in[a] == out[a]) {
                if (in_stride[a] != out_stride[a])
                    return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: in place with two different row strides", who);
                continue;
            }
            for (int b = 0; b < 5; b++)
                if (in[b] && overlap(span_of(in[b], P, in_stride[b], width[b]), span_of(out[a], rows_out, out_stride[a], width[a])))
                    return report_errorf(F3DGS_ERR_INVALID_ARGUMENT,
                                         "%s: an output overlaps an input (only the same array in place, without src_rows, is taken)", who);
        }
    }
    if (!scratch || scratch_bytes < f3dgs_transform_gaussians_scratch_bytes(G))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch of %zu bytes, %zu are needed", who, scratch ? scratch_bytes : (size_t)0,
                             f3dgs_transform_gaussians_scratch_bytes(G));
    if (reinterpret_cast<uintptr_t>(scratch) & 7u) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 8-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    Job job{};
    job.P = P, job.M = rows_out, job.G = G, job.linear = scale_mode == F3DGS_TRANSFORM_SCALES_LINEAR;
    job.groups = groups, job.src_rows = src_rows, job.status = status, job.table = static_cast<const double*>(scratch);
    job.xyz = xyz, job.rot = rotations, job.scales = scales, job.cov = cov3d, job.sh = sh_rest;
    job.xyz_out = xyz_out, job.rot_out = rotations_out, job.scales_out = scales_out, job.cov_out = cov3d_out, job.sh_out = sh_rest_out;
    job.sh_stride = sh_stride, job.sh_out_stride = sh_out_stride;
    hipLaunchKernelGGL(transform_table_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, G, quat, scale, translation, pivot,
                       static_cast<double*>(scratch), status);
    if (rows_out > 0 && P > 0) {
        const dim3 grid((unsigned)(((size_t)rows_out + ROWS - 1) / ROWS));
        switch (n_rest) {
            case 0: hipLaunchKernelGGL((transform_kernel<0>), grid, dim3(256), 0, st, job); break;
            case 3: hipLaunchKernelGGL((transform_kernel<3>), grid, dim3(256), 0, st, job); break;
            case 8: hipLaunchKernelGGL((transform_kernel<8>), grid, dim3(256), 0, st, job); break;
            default: hipLaunchKernelGGL((transform_kernel<15>), grid, dim3(256), 0, st, job); break;
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
