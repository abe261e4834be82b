// Language-guided editing: which Gaussians match a text prompt (gaussian_renderer/__init__.py:21-55 of the reference,
// calculate_selection_score / calculate_selection_score_delete), as ONE pass over the (P, C) feature table.
//
// The reference's arithmetic, step by step and in its number formats (the fp16 roundings decide which side of the threshold
// a row falls on, so they are the specification, not an approximation):
//   n = ||f||_2 and f^ = f / n in fp32 (optionally written back: the reference's `features /= ...`);
//   f^ and the fp32-normalised text rows rounded to fp16 (`.half()`);
//   s_k = f^ . t^_k rounded to fp16 (the half GEMM: exact fp16 products, fp32 accumulation in some order);
//   K > 1: softmax over the K fp16 scores (the reference evaluates it in fp32), every probability rounded to fp16;
// The two accumulations are carried in fp64 here and rounded to fp16 ONCE: the result is the fp16 neighbour of the exact
// value, the one point every fp32 evaluation order scatters around, and it does not depend on the lane layout.
//   the decision (include/f3dgs.h lists the branches), on the fp16 values.
//
// Shape: a GROUP of G lanes (a power of two, G >= K, G >= C/4 up to 64) owns a row, so a wave holds 64 / G rows.  Every lane
// keeps its float4 pieces of the row in registers between the norm and the contraction (the row is read from memory once;
// the next tile's row is requested before the current one is worked on).  The normalised fp16 text block sits in LDS.  The K
// dot products are exact fp32 products summed in fp64, reduced over the group with DPP (inside a row of 16 lanes) and
// ds_bpermute (across); after the reductions lane k of the group holds s_k, and softmax, the positive sum and the argmax
// are group reductions as well, so all rows of a wave are decided at once.  Rows with C % 4 != 0, unaligned pointers or
// C > 2048 take edit_generic_kernel: scalar loads, the row re-read per text row (from cache), same arithmetic.
#include <math.h>

#include <hip/hip_fp16.h>

#include "common.h"
#include "render_common.h"

namespace f3dgs {

namespace {

constexpr int ED_THREADS = 256;
constexpr int ED_MAX_BLOCKS = 2048;     // grid-stride beyond: 8 workgroups on each of 256 CUs

struct EditArgs {
    int P, C, K;
    int G;                   // lanes per row
    const float* features;
    float* normalized_out;   // nullptr, or may alias features
    const float* text;
    unsigned long long positive_mask;
    int first_positive;
    int is_delete, text_normalized, fill_unselected, has_threshold;
    float threshold;
    float* mask_out;
    float* score_out;        // nullptr
    const float* opacity_in; // nullptr
    float* opacity_out;
};

__device__ __forceinline__ float round_h(float x) { return __half2float(__float2half_rn(x)); }

// all-reduce over the G lanes of a group (G a power of two, groups aligned to G): DPP for the steps inside a row of 16 lanes,
// ds_bpermute for the two above.  Op must be commutative and associative.
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_mov(T x) {
    static_assert(sizeof(T) == 4, "one register");
    int i;
    __builtin_memcpy(&i, &x, 4);
    i = __builtin_amdgcn_update_dpp(0, i, CTRL, 0xF, 0xF, false);
    __builtin_memcpy(&x, &i, 4);
    return x;
}

template <typename T, typename Op>
__device__ __forceinline__ T group_reduce(T v, int G, Op op) {
    if (G >= 2) v = op(v, dpp_mov<0xB1>(v));     // quad_perm [1,0,3,2]
    if (G >= 4) v = op(v, dpp_mov<0x4E>(v));     // quad_perm [2,3,0,1]
    if (G >= 8) v = op(v, dpp_mov<0x141>(v));    // row_half_mirror
    if (G >= 16) v = op(v, dpp_mov<0x140>(v));   // row_mirror
    if (G >= 32) v = op(v, __shfl_xor(v, 16, 64));
    if (G >= 64) v = op(v, __shfl_xor(v, 32, 64));
    return v;
}

__device__ __forceinline__ float group_sum(float v, int G) {
    return group_reduce(v, G, [](float a, float b) { return a + b; });
}

template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double x) {
    int w[2];
    __builtin_memcpy(w, &x, 8);
    w[0] = __builtin_amdgcn_update_dpp(0, w[0], CTRL, 0xF, 0xF, false);
    w[1] = __builtin_amdgcn_update_dpp(0, w[1], CTRL, 0xF, 0xF, false);
    __builtin_memcpy(&x, w, 8);
    return x;
}

// the same all-reduce for an fp64 sum
__device__ __forceinline__ double group_sum_d(double v, int G) {
    if (G >= 2) v += dpp_mov_d<0xB1>(v);
    if (G >= 4) v += dpp_mov_d<0x4E>(v);
    if (G >= 8) v += dpp_mov_d<0x141>(v);
    if (G >= 16) v += dpp_mov_d<0x140>(v);
    if (G >= 32) v += __shfl_xor(v, 16, 64);
    if (G >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

// fp64 -> fp16, round to nearest even, as ONE rounding: the value goes to fp32 rounded to odd (truncate the magnitude, set the
// last bit if anything was lost), which the fp32 -> fp16 conversion then rounds as it would have rounded the fp64 value
__device__ __forceinline__ float round_h_d(double x) {
    float f = (float)x;
    const double d = (double)f;
    if (d != x) {
        uint32_t u = __float_as_uint(f);
        if (fabs(d) > fabs(x)) u -= 1;
        f = __uint_as_float(u | 1u);
    }
    return round_h(f);
}

__device__ __forceinline__ float half_bits_to_float(uint32_t bits) {
    const unsigned short u = (unsigned short)bits;
    _Float16 h;
    __builtin_memcpy(&h, &u, 2);
    return (float)h;
}

__device__ __forceinline__ uint32_t float_to_half_bits(float x) {      // round to nearest even
    const _Float16 h = (_Float16)x;
    unsigned short u;
    __builtin_memcpy(&u, &h, 2);
    return u;
}

// (fp16 value, column) packed in one register: the value's 16 bits above, the column below.  torch.argmax: NaN is the
// maximum, the lowest column wins among equals.
__device__ __forceinline__ uint32_t argmax_better(uint32_t a, uint32_t b) {
    const float va = half_bits_to_float(a >> 16), vb = half_bits_to_float(b >> 16);
    const uint32_t ia = a & 0xFFFFu, ib = b & 0xFFFFu;
    const bool an = va != va, bn = vb != vb;
    const bool a_wins = an ? (!bn || ia < ib) : (!bn && (va > vb || (va == vb && ia < ib)));
    return a_wins ? a : b;
}

// The decision for the rows of one wave.  Lane gl of a group holds s = s_gl (already rounded to fp16) for gl < K; every lane
// of the group returns the row's mask (0 or 1) and *decided.
__device__ __forceinline__ float decide(const EditArgs& a, int gl, float s, float* decided) {
    const int G = a.G, K = a.K;
    if (K == 1) {
        const float s0 = __shfl(s, 0, G);
        *decided = s0;
        return s0 >= a.threshold ? 1.f : 0.f;
    }
    const bool live = gl < K;
    // softmax over the fp16 scores: exp and the quotient are evaluated in fp64 and rounded to fp16 once, so that a probability
    // is the fp16 neighbour of its exact value (an fp32 evaluation lands on the other neighbour on about 1 row in 10^4, and
    // q2 below would carry that twice).  A NaN or +inf score makes every probability of the row NaN, whatever the maximum
    // does with NaN: exp(s - m) is NaN for that column and so is the sum.
    const float m = group_reduce(live ? s : -INFINITY, G, [](float x, float y) { return fmaxf(x, y); });
    const double e = live ? exp((double)(s - m)) : 0.0;          // s - m: a difference of fp16 values, exact
    const double sum = group_sum_d(e, G);
    const float p = round_h_d(e / sum);
    const bool pos = live && ((a.positive_mask >> gl) & 1ull);
    const float q = round_h_d(group_sum_d(pos ? (double)p : 0.0, G));
    if (!a.is_delete && a.has_threshold) {
        *decided = q;
        return q >= a.threshold ? 1.f : 0.f;
    }
    // column first_positive is replaced by q; the other positive columns stay: argmax over the K columns
    const float v = gl == a.first_positive ? q : p;
    // (v is an fp16 value: the conversion is exact); a lane beyond K: -inf in the last column, which never wins
    const uint32_t key = live ? (float_to_half_bits(v) << 16) | (uint32_t)gl : (0xFC00u << 16) | 0xFFFFu;
    const uint32_t best = group_reduce(key, G, [](uint32_t x, uint32_t y) { return argmax_better(x, y); });
    const bool in_pos = (a.positive_mask >> (best & 0xFFFFu)) & 1ull;
    if (a.is_delete && a.has_threshold) {
        // summed AFTER the replacement: the positives other than the first count twice (as the reference does)
        const float q2 = round_h_d(group_sum_d(pos ? (double)v : 0.0, G));
        *decided = q2;
        return (in_pos || q2 >= a.threshold) ? 1.f : 0.f;
    }
    *decided = q;
    return in_pos ? 1.f : 0.f;
}

__device__ __forceinline__ void write_row(const EditArgs& a, int row, float mask, float decided) {
    a.mask_out[row] = mask;
    if (a.score_out) a.score_out[row] = decided;
    if (a.opacity_out) {
        const bool fill = a.fill_unselected ? mask <= 0.5f : mask >= 0.5f;
        a.opacity_out[row] = fill ? 0.f : a.opacity_in[row];
    }
}

// the K x C text block into LDS as fp16, normalised in fp32 first unless the caller did that
__device__ __forceinline__ void stage_text(const EditArgs& a, __half* lds_text) {
    const int C = a.C, K = a.K;
    if (a.text_normalized) {
        for (int i = threadIdx.x; i < K * C; i += ED_THREADS) lds_text[i] = __float2half_rn(a.text[i]);
    } else {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int k = wave; k < K; k += ED_THREADS / 64) {
            const float* t = a.text + (size_t)k * C;
            float ss = 0.f;
            for (int c = lane; c < C; c += 64) ss = fmaf(t[c], t[c], ss);
            const float n = sqrtf(group_sum(ss, 64));
            for (int c = lane; c < C; c += 64) lds_text[k * C + c] = __float2half_rn(t[c] / n);
        }
    }
    __syncthreads();
}

// C % 4 == 0, C <= 256 * NV, 16-byte aligned rows: NV float4 per lane
template <int NV>
__global__ void __launch_bounds__(ED_THREADS) edit_rows_kernel(const EditArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __half* lds_text = reinterpret_cast<__half*>(lds_raw);
    stage_text(a, lds_text);

    const int G = a.G, C = a.C, K = a.K, C4 = C >> 2;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), r = lane / G, R = 64 / G;
    const int wave = blockIdx.x * (ED_THREADS / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (ED_THREADS / 64);
    const int ntiles = (a.P + R - 1) / R;

    auto load_tile = [&](int tile, float4 (&v)[NV]) {
        const int row = tile * R + r;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c4 = gl + G * j;
            v[j] = (tile < ntiles && row < a.P && c4 < C4)
                       ? reinterpret_cast<const float4*>(a.features + (size_t)row * C)[c4]
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    float4 nxt[NV];
    load_tile(wave, nxt);
    for (int tile = wave; tile < ntiles; tile += nwaves) {
        float4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] = nxt[j];
        load_tile(tile + nwaves, nxt);
        const int row = tile * R + r;
        const bool valid = row < a.P;

        // the order of torch's vectorised row reduction (one accumulator per float4 component, then x + y + z + w, then a
        // lane tree), so that the norm, and with it the written-back row, equals torch's bit for bit where measured
        float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            sx = fmaf(v[j].x, v[j].x, sx);
            sy = fmaf(v[j].y, v[j].y, sy);
            sz = fmaf(v[j].z, v[j].z, sz);
            sw = fmaf(v[j].w, v[j].w, sw);
        }
        // (rows shorter than 128: torch gives every element its own lane and adds neighbours pairwise)
        const float ss = C < 128 ? __fadd_rn(__fadd_rn(sx, sy), __fadd_rn(sz, sw)) : __fadd_rn(__fadd_rn(__fadd_rn(sx, sy), sz), sw);
        const float n = sqrtf(group_sum(ss, G));
        __half2 h[NV][2];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float4 f = make_float4(v[j].x / n, v[j].y / n, v[j].z / n, v[j].w / n);
            const int c4 = gl + G * j;
            if (a.normalized_out && valid && c4 < C4) reinterpret_cast<float4*>(a.normalized_out + (size_t)row * C)[c4] = f;
            h[j][0] = __halves2half2(__float2half_rn(f.x), __float2half_rn(f.y));
            h[j][1] = __halves2half2(__float2half_rn(f.z), __float2half_rn(f.w));
        }

        float s = 0.f;
        for (int k = 0; k < K; ++k) {
            // a product of two fp16 values is exact in fp32; the sum is carried in fp64 and rounded to fp16 once: the fp16
            // neighbour of the exact dot product, which every fp32 accumulation order approximates
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int c4 = gl + G * j;
                if (c4 < C4) {
                    const uint2 raw = *reinterpret_cast<const uint2*>(lds_text + (size_t)k * C + 4 * c4);
                    __half2 t0, t1;
                    __builtin_memcpy(&t0, &raw.x, 4);
                    __builtin_memcpy(&t1, &raw.y, 4);
                    acc += (double)__fmul_rn(__low2float(h[j][0]), __low2float(t0));
                    acc += (double)__fmul_rn(__high2float(h[j][0]), __high2float(t0));
                    acc += (double)__fmul_rn(__low2float(h[j][1]), __low2float(t1));
                    acc += (double)__fmul_rn(__high2float(h[j][1]), __high2float(t1));
                }
            }
            const double tot = group_sum_d(acc, G);
            if (gl == k) s = round_h_d(tot);
        }

        float decided;
        const float mask = decide(a, gl, s, &decided);
        if (valid && gl == 0) write_row(a, row, mask, decided);
    }
}

// any C >= 1, any alignment: scalar loads; the row is read once for the norm and once per text row (from cache, not HBM)
__global__ void __launch_bounds__(ED_THREADS) edit_generic_kernel(const EditArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __half* lds_text = reinterpret_cast<__half*>(lds_raw);
    stage_text(a, lds_text);

    const int G = a.G, C = a.C, K = a.K;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), r = lane / G, R = 64 / G;
    const int wave = blockIdx.x * (ED_THREADS / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (ED_THREADS / 64);
    const int ntiles = (a.P + R - 1) / R;

    for (int tile = wave; tile < ntiles; tile += nwaves) {
        const int row = tile * R + r;
        const bool valid = row < a.P;
        const float* f = a.features + (size_t)(valid ? row : 0) * C;
        float ss = 0.f;
        for (int c = gl; c < C; c += G) ss = fmaf(f[c], f[c], ss);
        const float n = sqrtf(group_sum(ss, G));
        float s = 0.f;
        for (int k = 0; k < K; ++k) {
            double acc = 0.0;
            for (int c = gl; c < C; c += G) {
                const float fh = round_h(f[c] / n);
                acc += (double)__fmul_rn(fh, __half2float(lds_text[(size_t)k * C + c]));
            }
            const double tot = group_sum_d(acc, G);
            if (gl == k) s = round_h_d(tot);
        }
        // after the last read of the row by this lane: normalized_out may alias features
        if (a.normalized_out && valid)
            for (int c = gl; c < C; c += G) a.normalized_out[(size_t)row * C + c] = f[c] / n;
        float decided;
        const float mask = decide(a, gl, s, &decided);
        if (valid && gl == 0) write_row(a, row, mask, decided);
    }
}

int pow2_at_least(int x) {
    int g = 1;
    while (g < x) g <<= 1;
    return g;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

int f3dgs_edit_select(int P, int C, int K, const float* features, float* normalized_out, const float* text,
                      uint64_t positive_mask, int first_positive, int variant, int has_threshold, float threshold,
                      float* mask_out, float* score_out, const float* opacity_in, float* opacity_out, void* stream) {
    if (P < 0 || P > (1 << 30) || C < 1 || K < 1)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: bad sizes P=%d C=%d K=%d", P, C, K);
    if (K > F3DGS_EDIT_MAX_TEXTS || (long long)K * C > F3DGS_EDIT_MAX_TEXT_ELEMENTS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: K=%d C=%d beyond the limit of %d text rows and K*C <= %d", K, C,
                   F3DGS_EDIT_MAX_TEXTS, F3DGS_EDIT_MAX_TEXT_ELEMENTS);
    const int known = F3DGS_EDIT_DELETE | F3DGS_EDIT_TEXT_NORMALIZED | F3DGS_EDIT_FILL_UNSELECTED;
    if (variant & ~known) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: unknown variant bits 0x%x", variant & ~known);
    if (positive_mask == 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: empty positive mask");
    if (K < 64 && (positive_mask >> K) != 0)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: positive mask has bits at or above K=%d", K);
    if (first_positive < 0 || first_positive >= K || !((positive_mask >> first_positive) & 1))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: first_positive=%d is not in the positive mask", first_positive);
    if (K == 1 && !has_threshold) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: K=1 needs a threshold");
    if ((opacity_in == nullptr) != (opacity_out == nullptr))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: opacity_in and opacity_out go together (both or neither)");
    if (P == 0) return F3DGS_OK;
    if (!features || !text || !mask_out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "edit_select: null pointer");

    EditArgs a;
    a.P = P; a.C = C; a.K = K;
    a.features = features; a.normalized_out = normalized_out; a.text = text;
    a.positive_mask = positive_mask; a.first_positive = first_positive;
    a.is_delete = (variant & F3DGS_EDIT_DELETE) ? 1 : 0;
    a.text_normalized = (variant & F3DGS_EDIT_TEXT_NORMALIZED) ? 1 : 0;
    a.fill_unselected = (variant & F3DGS_EDIT_FILL_UNSELECTED) ? 1 : 0;
    a.has_threshold = has_threshold ? 1 : 0;
    a.threshold = threshold;
    a.mask_out = mask_out; a.score_out = score_out; a.opacity_in = opacity_in; a.opacity_out = opacity_out;

    const bool vec = (C % 4 == 0) && C <= 2048 && aligned16(features) && (!normalized_out || aligned16(normalized_out));
    a.G = pow2_at_least(vec ? (C / 4 > K ? C / 4 : K) : (C > K ? C : K));
    if (a.G > 64) a.G = 64;
    const int R = 64 / a.G;
    const long long ntiles = ((long long)P + R - 1) / R;
    const long long want = (ntiles + ED_THREADS / 64 - 1) / (ED_THREADS / 64);
    const dim3 grid((unsigned)(want < ED_MAX_BLOCKS ? want : ED_MAX_BLOCKS)), block(ED_THREADS);
    const size_t lds = (size_t)K * C * sizeof(__half);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (!vec) {
        hipLaunchKernelGGL(edit_generic_kernel, grid, block, lds, s, a);
    } else {
        const int nv = (C / 4 + 63) / 64;
        if (nv <= 1) hipLaunchKernelGGL(edit_rows_kernel<1>, grid, block, lds, s, a);
        else if (nv <= 2) hipLaunchKernelGGL(edit_rows_kernel<2>, grid, block, lds, s, a);
        else if (nv <= 4) hipLaunchKernelGGL(edit_rows_kernel<4>, grid, block, lds, s, a);
        else hipLaunchKernelGGL(edit_rows_kernel<8>, grid, block, lds, s, a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "edit_select: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
