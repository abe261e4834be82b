// decoder_tile.h - the 1x1 CNN_decoder contraction y = X W^T + b on the fp32 matrix pipe, one copy for its three users: the
// feature-map loss and the decode (feature_loss.hip: fl_decoder_kernel, fl_decode_kernel) and the segmentation (segment.hip:
// seg_kernel, which promises the decode's values bit for bit).
//
// v_mfma_f32_32x32x2_f32: exact fp32, A/B one value per lane, A[i = l&31][k = l>>5], B[k = l>>5][n = l&31], D column l&31,
// rows (r&3)+8(r>>2)+4(l>>5).  A WAVE owns 32 pixels for all Cout, a workgroup = 4 waves = 128 pixels.  Everything per pixel
// stays in registers; the only shared data is the current 32-row tile of W (LDS, double-buffered).  With lane
// l = (px = l & 31, h = l >> 5) and the K index of an MFMA step s defined as c = h C/2 + s (any bijection of K works as long
// as both operands use it):
//   phase A   y^T[co][px] = W[co][:] . X[px][:]      A = W tile row (b128 LDS reads: four steps per read),
//                                                    B = this lane's half row of X, loaded ONCE into C/2 registers
// The result lies in D's layout: lane = column px, register r = row co(r, h) = co0 + mfma_row(r, h).  That IS the B layout of
// a second contraction over co in which step r contracts co(r, 0) with co(r, 1): the callers' phase B (g_x = g W in the loss,
// the text logits in the segmentation) takes the accumulator register r of phase A itself as its B operand - no transpose,
// no LDS round trip, no barrier between the phases.
//
// Which K index a step contracts, how the W tile lies in LDS and which register holds which output row are decided here and
// nowhere else; the callers keep their epilogues.  It is a header because the kernels are templates over C; feature_loss.o
// and segment.o are compiled with the same contraction flags, and the bit equality between them rests on that.
// Everything here is `__device__ __forceinline__`.
#pragma once

#include "common.h"

namespace f3dgs {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int mfma_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }   // 32x32 D layout

namespace decoder_tile {

template <int C>
constexpr int WS = C + 4;              // W tile row stride: 16-byte aligned rows, b128 reads of 32 rows hit all banks evenly
template <int C>
constexpr int LPT = (32 * C / 4) / 256;       // float4 loads per thread for one W tile (C = 32: 1, 64: 2, 128: 4)

// When the next W tile is requested.  Normally ahead of phase A: in flight during this tile's MFMAs.  C = 128: behind phase A
// instead (the callers' phase B alone is 4 k matrix-pipe cycles), so that its sixteen registers never live next to what the
// caller holds through phase A - in the loss the sixteen ground-truth values: together they put the kernel 21 registers above
// the 256 of two waves per SIMD (spills inside the tile loop)
template <int C>
constexpr bool LATE_W = C >= 128;

// this lane's half row of X[N][C]: channels h C/2 .. h C/2 + C/2 - 1 of pixel p (row 0 stands in beyond N; ZERO_PAST_N: as zeros)
template <int C, bool ZERO_PAST_N>
__device__ __forceinline__ void load_x(float (&xr)[C / 2], const float* X, int p, int N, int h) {
    constexpr int HC = C / 2;
    const bool p_ok = p < N;
    const float4* src = reinterpret_cast<const float4*>(X + (size_t)(p_ok ? p : 0) * C + h * HC);
#pragma unroll
    for (int k = 0; k < HC / 4; k++) {
        const float4 v = src[k];
        if constexpr (ZERO_PAST_N) {
            xr[4 * k] = p_ok ? v.x : 0.f; xr[4 * k + 1] = p_ok ? v.y : 0.f; xr[4 * k + 2] = p_ok ? v.z : 0.f; xr[4 * k + 3] = p_ok ? v.w : 0.f;
        } else {
            xr[4 * k] = v.x; xr[4 * k + 1] = v.y; xr[4 * k + 2] = v.z; xr[4 * k + 3] = v.w;
        }
    }
}

// W tile staging: thread t moves float4 #(t + 256 k) of the 32 x C tile of rows co0 .. co0 + 31 (zero rows past Cout).
// (Wd and, below, bias are taken by reference: the loads then go through the kernel's own pointer as they did when this
// text stood in the kernels, and the compiler forms the same addresses - by value it orders the first tile's loads otherwise.)
template <int C>
__device__ __forceinline__ void load_w(float4 (&v)[LPT<C>], const float* __restrict__ const& Wd, int Cout, int co0) {
#pragma unroll
    for (int k = 0; k < LPT<C>; k++) {
        const int e = (threadIdx.x + 256 * k) * 4, r = e / C, c = e - r * C;
        v[k] = co0 + r < Cout ? *reinterpret_cast<const float4*>(Wd + (size_t)(co0 + r) * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// &Ws[buf][r][c] of the double-buffered LDS image Ws[2][32][WS], which feature_loss.hip holds as that array and segment.hip
// as a pointer behind its text tiles.  One layout in two spellings, because the register allocation of each unit's kernels
// follows the spelling (32-bit array offsets / pointer arithmetic) and each keeps its register count only with its own.
template <int C>
__device__ __forceinline__ float* w_at(float (&Ws)[2][32][WS<C>], int buf, int r, int c) { return &Ws[buf][r][c]; }
template <int C>
__device__ __forceinline__ float* w_at(float* Ws, int buf, int r, int c) { return Ws + ((size_t)buf * 32 + r) * WS<C> + c; }

template <int C, class Tile>
__device__ __forceinline__ void store_w(Tile& Ws, int buf, const float4 (&v)[LPT<C>]) {
#pragma unroll
    for (int k = 0; k < LPT<C>; k++) {
        const int e = (threadIdx.x + 256 * k) * 4, r = e / C, c = e - r * C;
        *reinterpret_cast<float4*>(w_at<C>(Ws, buf, r, c)) = v[k];
    }
}

// the accumulator starts at the bias: y = W x + b.  bias_row: register r's start, the row co = co0 + mfma_row(r, h) (zero past Cout);
// WHOLE_TILES: the caller guarantees Cout % 32 == 0, no row is past Cout
template <bool WHOLE_TILES = false>
__device__ __forceinline__ float bias_row(const float* __restrict__ const& bias, int Cout, int co) {
    return WHOLE_TILES || co < Cout ? bias[co] : 0.f;
}

template <bool WHOLE_TILES = false>
__device__ __forceinline__ void bias_start(f32x16& acc, const float* __restrict__ const& bias, int Cout, int co0, int h) {
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = bias_row<WHOLE_TILES>(bias, Cout, co0 + mfma_row(r, h));
}

// ---- phase A over the tile in buffer `buf` (scheduling fences: without them every LDS read of the unrolled loop is hoisted
//      to the top and the loss kernel needs > 256 registers)
template <int C, class Tile>
__device__ __forceinline__ void phase_a(f32x16& acc, Tile& Ws, int buf, int li, int h, const float (&xr)[C / 2]) {
    constexpr int HC = C / 2;
    const float* wrow = w_at<C>(Ws, buf, li, h * HC);
#pragma unroll
    for (int s4 = 0; s4 < HC / 4; s4++) {
        const float4 a = *reinterpret_cast<const float4*>(wrow + 4 * s4);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xr[4 * s4 + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xr[4 * s4 + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xr[4 * s4 + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xr[4 * s4 + 3], acc, 0, 0, 0);
        if ((s4 & 1) == 1) __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace decoder_tile

}  // namespace f3dgs
