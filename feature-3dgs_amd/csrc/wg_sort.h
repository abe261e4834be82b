// wg_sort.h - what a radix pass inside ONE workgroup is made of: wave and workgroup scans, the ballot rank, the digit offsets and the
// whole 8-bit pass over pairs that live in registers and LDS.  Who uses what:
//   wave_incl_scan, block_excl_scan_256   every scan of binning.hip and preprocess.hip (lookback.h includes this file)
//   wave_digit_rank                       onesweep_pass_kernel, the streaming passes of depth_bucket_sort_kernel and, through
//                                         lds_radix_pass, the two in-LDS sorts (radix_scatter_kernel keeps the match written out)
//   digit_offsets                         lds_radix_pass (counters of NW waves) and the streaming passes (a plain histogram)
//   SortLds, lds_radix_pass               small_sort_kernel and the in-LDS path of depth_bucket_sort_kernel
#pragma once

#include "common.h"

namespace f3dgs {

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive scan of one value per thread across a 256-thread workgroup. `sh` holds >= 8 words.
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t* sh, uint32_t* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v, lane);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t s = sh[k];
        if (k < w) base += s;
    }
    if (total) *total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + inc - v;
}

// Rank of an item among the items of its digit d (`bits` wide) that the wave has seen so far in this pass: the lanes that hold the same
// digit are matched with one ballot per bit, the first of them moves the wave's counter vcnt[d] on (wave-ordered: no atomics).
// All 64 lanes call; vcnt = the wave's row of counters, lt_mask = the lanes below this one.
// `bits` is a reference to a constant at the call site, not a template parameter or a value: a helper is optimised on its own before
// it is inlined, and with a known width its bit loop is unrolled there, the kernel's passes then reorder the chain of ANDs, and every
// bit costs two instructions where the loop written out in the kernel costs one (v_bitop3_b32).  Unknown until inlined, it compiles
// like the written-out loop (profiles/wg_sort_core.md).
__device__ __forceinline__ uint32_t wave_digit_rank(bool valid, uint32_t d, const int& bits, volatile uint32_t* vcnt, unsigned long long lt_mask) {
    const unsigned long long vm = __ballot(valid);
    uint32_t p_lo = (uint32_t)vm, p_hi = (uint32_t)(vm >> 32);
#pragma unroll
    for (int b = 0; b < bits; b++) {
        // x: all ones where the lane's digit has bit b; a peer's bit equals it: peers &= ~(ballot ^ x) = ~ballot ^ x
        const uint32_t x = 0u - ((d >> b) & 1u);
        const unsigned long long nm = ~__ballot(x != 0u);
        p_lo &= (uint32_t)nm ^ x;
        p_hi &= (uint32_t)(nm >> 32) ^ x;
    }
    const unsigned long long peers = ((unsigned long long)p_hi << 32) | p_lo;
    const uint32_t before = __popcll(peers & lt_mask);
    const uint32_t old = vcnt[d];
    if (valid && before == 0) vcnt[d] = old + (uint32_t)__popcll(peers);
    return old + before;
}

// Exclusive scan over the 256 digits of one total per digit (thread d < 256 holds digit d's, every thread of the workgroup calls):
// the start of the digit, valid in the first 256 threads.  One barrier; wsum: four words.
__device__ __forceinline__ uint32_t digit_excl_scan(uint32_t tot, uint32_t* wsum) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t inc = wave_incl_scan(tot, lane);
    if (tid < 256 && lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    if (tid < 256) {
        base = inc - tot;
        for (int ww = 0; ww < w; ww++) base += wsum[ww];
    }
    return base;
}

// The digit offsets of a pass.  cnt[NW][256], what the NW waves counted, becomes where each wave's items of each digit start
// (digits in order, inside a digit the waves in order) ...
template <int NW>
__device__ __forceinline__ void digit_offsets(uint32_t (*cnt)[256], uint32_t* wsum) {
    const int tid = threadIdx.x;
    uint32_t tot = 0;
    if (tid < 256) {
#pragma unroll
        for (int ww = 0; ww < NW; ww++) tot += cnt[ww][tid];
    }
    uint32_t base = digit_excl_scan(tot, wsum);
    if (tid < 256) {
#pragma unroll
        for (int ww = 0; ww < NW; ww++) {
            const uint32_t c = cnt[ww][tid];
            cnt[ww][tid] = base;
            base += c;
        }
    }
}
// ... and a plain histogram of the 256 digits becomes their starts, in place.
__device__ __forceinline__ void digit_offsets(uint32_t* hist, uint32_t* wsum) {
    const int tid = threadIdx.x;
    const uint32_t base = digit_excl_scan(tid < 256 ? hist[tid] : 0u, wsum);
    if (tid < 256) hist[tid] = base;
}

// The LDS image of a sort inside one workgroup of THREADS threads: up to CAP pairs and the waves' digit counters.
template <int THREADS, int CAP>
struct SortLds {
    uint32_t key[CAP];
    uint32_t val[CAP];
    uint32_t cnt[THREADS / 64][256];
    uint32_t wsum[4];
};

// One stable 8-bit pass over n <= CAP pairs held in registers: rank per wave, digit offsets, scatter into the LDS image, and - unless
// this is the `last` pass, whose result the caller takes from L.key / L.val - back into the registers in the new order.  Three barriers.
// Item order: wave w owns [64 steps w, 64 steps (w + 1)), visited in `steps` = ceil(n / THREADS) <= ITEMS steps of 64 consecutive
// items (lane = item within the step): the items are spread evenly over the waves, the unused steps of a small problem are skipped.
// (`bits`: see wave_digit_rank; callers leave it alone.)
template <int THREADS, int ITEMS, int CAP>
__device__ __forceinline__ void lds_radix_pass(SortLds<THREADS, CAP>& L, uint32_t (&key)[ITEMS], uint32_t (&val)[ITEMS],
                                               uint32_t (&rank)[ITEMS], int steps, uint32_t n, int shift, bool last, const int& bits = 8) {
    constexpr int NW = THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t wbase = (uint32_t)(w * steps * 64 + lane);
    for (int d = tid; d < NW * 256; d += THREADS) (&L.cnt[0][0])[d] = 0;
    __syncthreads();       // counters cleared; the previous pass's read-back is complete
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        if (k >= steps) break;
        const uint32_t i = wbase + (uint32_t)(k * 64);
        rank[k] = wave_digit_rank(i < n, (key[k] >> shift) & 255u, bits, &L.cnt[w][0], lt_mask);
    }
    __syncthreads();
    digit_offsets<NW>(L.cnt, L.wsum);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t i = wbase + (uint32_t)(k * 64);
        if (k < steps && i < n) {
            const uint32_t pos = L.cnt[w][(key[k] >> shift) & 255u] + rank[k];
            L.key[pos] = key[k];
            L.val[pos] = val[k];
        }
    }
    __syncthreads();
    if (!last) {
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t i = wbase + (uint32_t)(k * 64);
            if (k < steps && i < n) { key[k] = L.key[i]; val[k] = L.val[i]; }
        }
    }
}

}  // namespace f3dgs
