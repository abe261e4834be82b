// binning.hip — scan, stable LSD radix sort, instance emission and tile ranges.
//
// What the reference does (R/cuda_rasterizer/rasterizer_impl.cu:279-320): prefix-sum tiles_touched,
// emit one (tile<<32 | depth_bits, gaussian_id) pair per overlapped tile in Gaussian-index order,
// stable-sort all N pairs on the 64-bit key with cub (6 passes at 1080p), find per-tile ranges.
//
// What this file does instead (same resulting order, far less traffic):
//   1. stable sort of the P Gaussians by their 32-bit depth key (4 LSD passes over P pairs - or one bucket pass and one launch
//      that sorts every bucket inside LDS: "depth sort by buckets" below);
//   2. prefix-sum of tiles_touched taken IN DEPTH ORDER;
//   3. emit instances (tile, id) in depth order;
//   4. stable sort of the N instances by tile id only (2 passes at <= 65536 tiles, digits as wide as the tile count needs).
// The last pass of 1 leaves every Gaussian's tile count at its place in the depth order (nobody reads that pass's keys), so 2 and
// 3 read the counts in a row.
// An LSD radix sort is "sort by low key, then stably by high key": steps 1+4 are exactly the
// reference's sort on (tile | depth) with ties broken by ascending Gaussian id, because the depth
// sort starts from id order and both sorts are stable (Q6 in SURVEY.md section 8a).
//
// Radix pass = 3 launches: per-workgroup digit histogram, per-digit row scan (grid = digits),
// stable scatter (wave-level match with ballots, wave-ordered LDS counters).  The bucket pass of the depth sort is the same three
// with its own layouts (template parameter BUCKET): the histogram matrix row-major with a column scan, the output as pairs.

#include <atomic>
#include "common.h"
#include "lookback.h"

namespace f3dgs {

namespace {

// ---------------- list offsets in depth order: two-level sums ------------------------------------------
// Two levels are kept: the sum of every run of 64 consecutive items (`sub`, 64 per workgroup chunk - one run is what
// one wave of the emit kernel owns) and the chunk totals.  An emit wave rebuilds its offset from the two (the totals of
// the chunks in front of its own, one 256-byte read of its chunk's runs, a wave scan), so no per-item offset array is
// written or read and the scan is ONE launch.
__global__ void __launch_bounds__(256) scan_reduce_kernel(const uint32_t* __restrict__ in,
                                                          const uint32_t* __restrict__ gather, size_t n,
                                                          uint32_t* __restrict__ block_sums, uint32_t* __restrict__ sub) {
    __shared__ uint32_t sh[8];
    const size_t base = (size_t)blockIdx.x * SCAN_CHUNK;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const size_t i = base + (size_t)k * 256 + threadIdx.x;
        v[k] = i < n ? (gather ? in[gather[i]] : in[i]) : 0u;
    }
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        uint32_t r = v[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) r += (uint32_t)__shfl_xor((int)r, d, 64);
        if (lane == 0) sub[(size_t)blockIdx.x * 64 + 4 * k + w] = r;       // items base + 256 k + 64 w .. + 63
        acc += v[k];
    }
    uint32_t tot;
    block_excl_scan_256(acc, sh, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}


// ---------------- radix sort pass -------------------------------------------------------------------
// Item order inside a workgroup chunk: wave w owns [w*1024, (w+1)*1024), visited in 16 steps of 64
// consecutive items (lane = item within the step).  BITS = digit width (8 for tile ids, 11 for the 32-bit
// depth keys: 3 passes instead of 4).  vals_in == nullptr means "value = item index" (first pass of the
// depth sort: saves an iota kernel and a key copy).
// `tj` (first pass of the depth sort only): workgroup 0 also adds up the per-workgroup instance counts of
// preprocess_kernel - both totals are known right after that kernel - and stores them to the device counters and
// straight into the host's pinned read-back words: no totals launch and no copy launch in front of the sort.
// `tj`: the per-workgroup instance counts of preprocess_kernel added up by ONE workgroup (all its THREADS threads call this) and
// stored to the device counters and straight into the host's pinned read-back words.
template <int THREADS>
__device__ __forceinline__ void run_totals_job(const TotalsJob& tj) {
    __shared__ uint32_t shc[3][THREADS / 64];
    uint32_t v = 0, u = 0, ar = 0;
    for (int i = threadIdx.x; i < tj.n_partial; i += THREADS) {
        v += tj.partial[i]; u += tj.partial[tj.n_partial + i]; ar = max(ar, tj.partial[2 * tj.n_partial + i]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        v += (uint32_t)__shfl_xor((int)v, d, 64);
        u += (uint32_t)__shfl_xor((int)u, d, 64);
        ar = max(ar, (uint32_t)__shfl_xor((int)ar, d, 64));
    }
    if ((threadIdx.x & 63) == 0) { shc[0][threadIdx.x >> 6] = v; shc[1][threadIdx.x >> 6] = u; shc[2][threadIdx.x >> 6] = ar; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t ref = 0, own = 0, arm = 0;
        for (int k = 0; k < THREADS / 64; k++) { ref += shc[0][k]; own += shc[1][k]; arm = max(arm, shc[2][k]); }
        // [0] entries of our lists, [1] the reference's count, [2] != 0: some visible Gaussian has a long axis (preprocess_kernel)
        tj.counters[0] = own; tj.counters[1] = ref; tj.counters[2] = arm; tj.counters[3] = 0u;    // ([3]: the emit kernel, later in the frame)
        if (tj.host) {
            __hip_atomic_store(&tj.host[0], own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&tj.host[1], ref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&tj.host[2], arm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __threadfence_system();
        }
    }
}

// BUCKET (the bucket pass of the depth sort, common.h): the digit of a key is its bucket, (key - kmin) >> s, the last bin for the
// culled keys.  kmin / kmax are the extremes of preprocess_kernel's per-workgroup partials (tj.partial: the fourth and fifth
// run), which EVERY workgroup reduces for itself - a few KB out of L2, behind its keys' requests - so that no launch stands
// between preprocess and this one; workgroup 0 leaves kmin and s in ctl[0 .. 1] for the two launches that follow.
__device__ __forceinline__ uint32_t depth_bucket_of(uint32_t key, uint32_t kmin, uint32_t s, uint32_t culled_bin) {
    return key == 0xFFFFFFFFu ? culled_bin : (key - kmin) >> s;
}
template <int BITS, int ITEMS, bool BUCKET = false>
__global__ void __launch_bounds__(SORT_THREADS) radix_hist_kernel(const uint32_t* __restrict__ keys, size_t n,
                                                                  int shift, uint32_t nb,
                                                                  uint32_t* __restrict__ hist, TotalsJob tj,
                                                                  const uint32_t* __restrict__ n_dev, uint32_t bucket_count,
                                                                  uint32_t* __restrict__ ctl) {
    constexpr int BINS = 1 << BITS;
    constexpr int CHUNK = SORT_THREADS * ITEMS;
    __shared__ __attribute__((aligned(BUCKET ? 16 : 4))) uint32_t h[BINS];       // (BUCKET: read back 16 bytes at a time)
    // n_dev (sync-free forward): the launch is sized by a CAPACITY n, the item count is the device's word; workgroups behind the
    // last item write their zero column of the histogram matrix and nothing else.  A count above the capacity reads as ZERO: the
    // emit kernel stored nothing for such a frame (the arrays hold what the allocator left there), the tile ranges stay empty
    if (n_dev) { const size_t nd = *n_dev; n = nd <= n ? nd : 0; }     // (a frame that does not fit is void: nothing was emitted)
    // every key of the thread is requested before anything else, as in the scatter kernel: written as load-and-count per item,
    // the compiled loop waited for each key in front of its LDS atomic - ITEMS memory round trips one behind the other
    const size_t base = (size_t)blockIdx.x * CHUNK;
    uint32_t key[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const size_t i = base + (size_t)k * SORT_THREADS + threadIdx.x;
        key[k] = i < n ? keys[i] : 0u;
    }
    if (tj.partial && blockIdx.x == 0) run_totals_job<SORT_THREADS>(tj);
    uint32_t kmin = 0, bshift = 0;
    if constexpr (BUCKET) {
        __shared__ uint32_t shk[2][SORT_THREADS / 64];
        uint32_t lo = 0xFFFFFFFFu, hi = 0u;
        // (the loop compiles to two steps a round trip, eight in a row at c3; all its loads in one run, and no reduction at all -
        // a stale range, timing only - both left the stage where it was: profiles/depth_bucket_sort.md 8)
        for (int i = threadIdx.x; i < tj.n_partial; i += SORT_THREADS) {
            lo = min(lo, tj.partial[3 * tj.n_partial + i]);
            hi = max(hi, tj.partial[4 * tj.n_partial + i]);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
            hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
        }
        if ((threadIdx.x & 63) == 0) { shk[0][threadIdx.x >> 6] = lo; shk[1][threadIdx.x >> 6] = hi; }
        __syncthreads();
        lo = min(min(shk[0][0], shk[0][1]), min(shk[0][2], shk[0][3]));
        hi = max(max(shk[1][0], shk[1][1]), max(shk[1][2], shk[1][3]));
        kmin = lo;
        bshift = depth_bucket_shift(lo, hi, bucket_count);
        if (blockIdx.x == 0 && threadIdx.x == 0) { ctl[0] = kmin; ctl[1] = bshift; }
    }
    for (int d = threadIdx.x; d < BINS; d += SORT_THREADS) h[d] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const size_t i = base + (size_t)k * SORT_THREADS + threadIdx.x;
        const uint32_t d = BUCKET ? depth_bucket_of(key[k], kmin, bshift, BINS - 1) : (key[k] >> shift) & (BINS - 1);
        if (i < n) atomicAdd(&h[d], 1u);
    }
    __syncthreads();
    if constexpr (BUCKET) {
        // row-major, hist[block * BINS + d]: the workgroup's counts are one contiguous row, written with 16-byte stores (digit-major,
        // every one of its 1,024 words went out alone, 4 nb bytes from the next); radix_colscan_kernel scans the columns
        static_assert(BINS % (4 * SORT_THREADS) == 0, "whole 16-byte stores per thread");
        uint4* const row = reinterpret_cast<uint4*>(hist + (size_t)blockIdx.x * BINS);
        const uint4* const h4 = reinterpret_cast<const uint4*>(h);
        for (int q = threadIdx.x; q < BINS / 4; q += SORT_THREADS) row[q] = h4[q];
    } else {
        for (int d = threadIdx.x; d < BINS; d += SORT_THREADS) hist[(size_t)d * nb + blockIdx.x] = h[d];  // digit-major
    }
}

// The bucket pass's scan: exclusive prefixes over the workgroups (rows) of every bin (column) of the row-major matrix, in place,
// and the column totals to totals[d].  A workgroup owns COLSCAN_BINS = 16 bins - one 64-byte sector of every row; thread (bin lane,
// row lane) owns a run of up to COLSCAN_RUN consecutive rows: all its loads are requested before the first add, the 16 run totals
// of a bin meet in LDS behind one barrier.  c3 (489 rows) is one sweep of 16 x 31 rows; longer matrices (c4 under option 1: 977
// rows) go on in further sweeps of up to COLSCAN_SWEEP_ROWS rows, the columns' sums so far carried along.
__global__ void __launch_bounds__(COLSCAN_BINS * COLSCAN_ROW_LANES)
radix_colscan_kernel(uint32_t* __restrict__ hist, uint32_t nb, uint32_t bins, uint32_t* __restrict__ totals) {
    __shared__ uint32_t part[COLSCAN_ROW_LANES][COLSCAN_BINS];
    const uint32_t bl = threadIdx.x % COLSCAN_BINS, rl = threadIdx.x / COLSCAN_BINS;
    const uint32_t d = blockIdx.x * COLSCAN_BINS + bl;        // (bins is a multiple of COLSCAN_BINS: every thread owns a column)
    uint32_t carry = 0;
    for (uint32_t row0 = 0; row0 < nb; row0 += COLSCAN_SWEEP_ROWS) {
        const uint32_t rows = min(nb - row0, (uint32_t)COLSCAN_SWEEP_ROWS);
        const uint32_t run = (rows + COLSCAN_ROW_LANES - 1) / COLSCAN_ROW_LANES;      // rows a row lane owns in this sweep
        const uint32_t first = row0 + rl * run, end = min(first + run, row0 + rows);   // (first >= end: a row lane behind the last row)
        uint32_t v[COLSCAN_RUN];
#pragma unroll
        for (int k = 0; k < COLSCAN_RUN; k++) {
            const uint32_t r = first + (uint32_t)k;
            const uint32_t x = hist[(size_t)(r < end ? r : row0) * bins + d];        // (unconditional loads: one run of requests, one wait)
            v[k] = r < end ? x : 0u;
        }
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < COLSCAN_RUN; k++) {
            const uint32_t x = v[k];
            v[k] = sum;                  // exclusive inside the run
            sum += x;
        }
        part[rl][bl] = sum;
        __syncthreads();
        uint32_t before = carry, tot = 0;
#pragma unroll
        for (int j = 0; j < COLSCAN_ROW_LANES; j++) {
            const uint32_t t = part[j][bl];
            before += (uint32_t)j < rl ? t : 0u;
            tot += t;
        }
#pragma unroll
        for (int k = 0; k < COLSCAN_RUN; k++) {
            const uint32_t r = first + (uint32_t)k;
            if (r < end) hist[(size_t)r * bins + d] = before + v[k];
        }
        carry += tot;
        __syncthreads();                 // every total read before the next sweep's are written
    }
    if (rl == 0) totals[d] = carry;
}

// One workgroup per digit: exclusive scan of that digit's per-workgroup counts, total to totals[d].
// The first ROWSCAN_GROUPS x 256 columns (c3: the whole row, 489 / 1289 columns) are requested at once and scanned behind ONE
// barrier - wave scans in registers, the 4 x ROWSCAN_GROUPS wave totals through LDS; a loop of load, scan (two barriers), store
// per 256 columns was as many memory round trips one behind the other.  Longer rows (c5) go on in that loop.
constexpr int ROWSCAN_GROUPS = 8;
__global__ void __launch_bounds__(256) radix_rowscan_kernel(uint32_t* __restrict__ hist, uint32_t nb,
                                                            uint32_t* __restrict__ totals) {
    __shared__ uint32_t sh[8];
    __shared__ uint4 wtot[ROWSCAN_GROUPS];        // [group] = totals of its four waves
    uint32_t* row = hist + (size_t)blockIdx.x * nb;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t v[ROWSCAN_GROUPS], inc[ROWSCAN_GROUPS];
#pragma unroll
    for (int k = 0; k < ROWSCAN_GROUPS; k++) {
        const uint32_t i = (uint32_t)k * 256 + threadIdx.x;
        const uint32_t r = row[i < nb ? i : 0u];        // (unconditional loads: one run of requests, one wait)
        v[k] = i < nb ? r : 0u;
    }
#pragma unroll
    for (int k = 0; k < ROWSCAN_GROUPS; k++) {
        inc[k] = (uint32_t)k * 256 < nb ? wave_incl_scan(v[k], lane) : 0u;       // (uniform: groups behind the row are zero)
        if (lane == 63) (&wtot[k].x)[w] = inc[k];
    }
    __syncthreads();
    uint32_t carry = 0;
#pragma unroll
    for (int k = 0; k < ROWSCAN_GROUPS; k++) {
        const uint4 t = wtot[k];
        const uint32_t before = carry + (w > 0 ? t.x : 0u) + (w > 1 ? t.y : 0u) + (w > 2 ? t.z : 0u);
        const uint32_t i = (uint32_t)k * 256 + threadIdx.x;
        if (i < nb) row[i] = before + inc[k] - v[k];
        carry += t.x + t.y + t.z + t.w;
    }
    for (uint32_t base = ROWSCAN_GROUPS * 256; base < nb; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? row[i] : 0;
        uint32_t tot;
        const uint32_t ex = block_excl_scan_256(v, sh, &tot);
        if (i < nb) row[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// RANGES (final tile pass only, needs REORDER): the keys are whole tile ids and the output is fully sorted, so the
// range of a tile is [min, max + 1) of the output positions of its entries.  Inside the LDS-sorted chunk the entries
// of one tile are adjacent and so are their output positions: two atomicMin per (workgroup, tile) segment on the
// all-ones preset of BinState::ranges_enc - a few dozen per workgroup, spread over all tiles.  This replaces a
// separate pass over the sorted keys.
__device__ __forceinline__ void record_range(uint2* ranges_enc, uint32_t tile, bool first, bool last, uint32_t pos) {
    if (first) atomicMin(&ranges_enc[tile].x, pos);
    if (last) atomicMin(&ranges_enc[tile].y, 0xFFFFFFFFu - (pos + 1u));
}

// COUNTS (final pass of the depth sort): nobody reads that pass's sorted keys, so an item's slot of keys_out receives
// payload[value] instead - the Gaussian's tile count at its place in the depth order (GeomState::key_a), gathered here, where
// the id is in a register anyway, rather than by the two kernels that walk the order afterwards.  The same stores, no more LDS.
// BUCKET (see radix_hist_kernel; never with REORDER): the digit is the key's bucket by ctl[0 .. 1], and workgroup 0 leaves every
// bucket's first position in bucket_offs for the launch that sorts the buckets.  `hist` is row-major (the workgroup's row, scanned
// by radix_colscan_kernel) and keys_out is the B side's run of 2n words, which receives (key, id) PAIRS; vals_out is not used.
template <int BITS, int ITEMS, bool REORDER, bool RANGES, bool COUNTS = false, bool BUCKET = false>
__global__ void __launch_bounds__(SORT_THREADS)
radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                     uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out, size_t n, int shift,
                     uint32_t nb, const uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals,
                     uint2* __restrict__ ranges_enc, const uint32_t* __restrict__ n_dev,
                     const uint32_t* __restrict__ payload, const uint32_t* __restrict__ ctl, uint32_t* __restrict__ bucket_offs) {
    constexpr int BINS = 1 << BITS;
    constexpr int CHUNK = SORT_THREADS * ITEMS;
    static_assert(!(BUCKET && (REORDER || RANGES || COUNTS)), "the bucket pass is a plain scatter of keys and ids");
    const uint32_t bk_min = BUCKET ? ctl[0] : 0u, bk_shift = BUCKET ? ctl[1] : 0u;
    auto digit_of = [&](uint32_t key) -> uint32_t {
        if constexpr (BUCKET) return depth_bucket_of(key, bk_min, bk_shift, BINS - 1);
        else return (key >> shift) & (BINS - 1);
    };
    // bins per thread in the offset phase; fewer bins than threads (digits of 4 ... 7 bits): the first BINS threads own one each
    constexpr int BPT = BINS >= SORT_THREADS ? BINS / SORT_THREADS : 1;
    static_assert(BINS >= SORT_THREADS ? BINS % SORT_THREADS == 0 : true, "whole bins per thread");
    if (n_dev) {        // (see radix_hist_kernel) a launch sized by a capacity: the workgroups behind the last item have nothing to move
        const size_t nd = *n_dev;
        n = nd <= n ? nd : 0;
        if ((size_t)blockIdx.x * CHUNK >= n) return;
    }
    __shared__ uint32_t cnt[4][BINS];
    __shared__ uint32_t sh[8];
    // REORDER: the chunk is first sorted inside LDS so that the global stores of a wave run over consecutive
    // addresses per digit (16 items per digit on average) instead of 64 unrelated 4-byte scatters.
    __shared__ uint32_t gbase[REORDER ? BINS : 1];     // global offset of this workgroup's run of digit d
    __shared__ uint32_t lstart[REORDER ? BINS : 1];    // start of digit d inside the LDS-sorted chunk
    __shared__ uint32_t skey[REORDER ? CHUNK : 1];
    __shared__ uint32_t sval[REORDER ? CHUNK : 1];
    volatile uint32_t* vcnt = &cnt[0][0];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = threadIdx.x; d < 4 * BINS; d += SORT_THREADS) (&cnt[0][0])[d] = 0;
    __syncthreads();

    const size_t wbase = (size_t)blockIdx.x * CHUNK + (size_t)w * (ITEMS * 64);
    uint32_t key[ITEMS];
    constexpr bool VAL_FIRST = REORDER || COUNTS;
    uint32_t val[VAL_FIRST ? ITEMS : 1];
    uint32_t rank[ITEMS];
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    // every request of the chunk goes out first (the values are only needed by the LDS reorder - and by the gather of COUNTS:
    // their latency hides behind the ranking)
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const size_t i = wbase + (size_t)k * 64 + lane;
        key[k] = i < n ? keys_in[i] : 0xFFFFFFFFu;
        if constexpr (VAL_FIRST) val[k] = (vals_in && i < n) ? vals_in[i] : (uint32_t)i;
    }
    // BUCKET: the matrix is row-major (radix_hist_kernel) - a thread's BPT bins are BPT consecutive words of the workgroup's row,
    // requested here with 16-byte loads behind the keys and needed only in the offset phase (digit-major they were BPT single
    // words 4 nb bytes apart, requested there)
    uint32_t hrow[BUCKET ? BPT : 1];
    (void)hrow;
    if constexpr (BUCKET) {
        static_assert(BPT % 4 == 0, "whole 16-byte loads per thread");
        const uint4* const row = reinterpret_cast<const uint4*>(hist + (size_t)blockIdx.x * BINS + (size_t)threadIdx.x * BPT);
#pragma unroll
        for (int q = 0; q < BPT / 4; q++) {
            const uint4 t = row[q];
            hrow[4 * q] = t.x; hrow[4 * q + 1] = t.y; hrow[4 * q + 2] = t.z; hrow[4 * q + 3] = t.w;
        }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const size_t i = wbase + (size_t)k * 64 + lane;
        const bool valid = i < n;
        const uint32_t d = digit_of(key[k]);
        const unsigned long long vm = __ballot(valid);
        uint32_t p_lo = (uint32_t)vm, p_hi = (uint32_t)(vm >> 32);
#pragma unroll
        for (int b = 0; b < BITS; b++) {
            // (wave_digit_rank, wg_sort.h, written out: through the helper the 4- and 6-bit instantiations come out one and two
            // instructions longer, profiles/wg_sort_core.md 2)
            const uint32_t x = 0u - ((d >> b) & 1u);
            const unsigned long long nm = ~__ballot(x != 0u);
            p_lo &= (uint32_t)nm ^ x;
            p_hi &= (uint32_t)(nm >> 32) ^ x;
        }
        const unsigned long long peers = ((unsigned long long)p_hi << 32) | p_lo;
        const uint32_t before = __popcll(peers & lt_mask);
        const uint32_t old = vcnt[w * BINS + d];
        if (valid && before == 0) vcnt[w * BINS + d] = old + (uint32_t)__popcll(peers);
        rank[k] = old + before;
    }
    // COUNTS without the LDS reorder: a lane stores its own items, so their payloads are requested here, one more register per
    // item, and arrive behind the offset phase
    uint32_t pay[(COUNTS && !REORDER) ? ITEMS : 1];
    (void)pay;
    if constexpr (COUNTS && !REORDER) {
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const size_t i = wbase + (size_t)k * 64 + lane;
            pay[k] = payload[i < n ? val[k] : 0u];      // (unconditional: one run of loads, one wait)
        }
    }
    __syncthreads();
    // thread t owns digits [t*BPT, (t+1)*BPT) - where there are fewer digits than threads, digit t or none: turn per-wave
    // counts into offsets (every thread takes part in the scans)
    {
        uint32_t tot[BPT], run = 0, blk[BPT], brun = 0;
#pragma unroll
        for (int q = 0; q < BPT; q++) {
            const uint32_t d = threadIdx.x * BPT + q;
            const bool own = BINS >= SORT_THREADS || d < (uint32_t)BINS;
            tot[q] = own ? totals[d] : 0u;
            run += tot[q];
            blk[q] = own ? cnt[0][d] + cnt[1][d] + cnt[2][d] + cnt[3][d] : 0u;
            brun += blk[q];
        }
        uint32_t digit_base = block_excl_scan_256(run, sh, nullptr);
        uint32_t local_base = REORDER ? block_excl_scan_256(brun, sh, nullptr) : 0;
#pragma unroll
        for (int q = 0; q < BPT; q++) {
            const uint32_t d = threadIdx.x * BPT + q;
            if (BINS < SORT_THREADS && d >= (uint32_t)BINS) break;
            const uint32_t g = digit_base + (BUCKET ? hrow[BUCKET ? q : 0] : hist[(size_t)d * nb + blockIdx.x]);
            if (BUCKET && blockIdx.x == 0) bucket_offs[d] = digit_base;
            if (REORDER) { gbase[d] = g; lstart[d] = local_base; }
            uint32_t r2 = REORDER ? local_base : g;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t c = cnt[k][d];
                cnt[k][d] = r2;
                r2 += c;
            }
            digit_base += tot[q];
            local_base += blk[q];
        }
    }
    __syncthreads();
    if (REORDER) {
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const size_t i = wbase + (size_t)k * 64 + lane;
            if (i < n) {
                const uint32_t d = digit_of(key[k]);
                const uint32_t lp = cnt[w][d] + rank[k];
                skey[lp] = key[k];
                if constexpr (REORDER) sval[lp] = val[k];
            }
        }
        __syncthreads();
        const size_t cbase = (size_t)blockIdx.x * CHUNK;
        const uint32_t have = (uint32_t)min((size_t)CHUNK, n - cbase);
        if constexpr (COUNTS) {
            // the ids come out of the LDS image in their new order: all of a thread's gathers go out before its first store (one
            // memory latency for the ITEMS of them), and nothing is staged through LDS.  (Gathered before the ranking and staged
            // through 8 KB more of LDS instead, the c3 pass took 13.9 us against 14.4: inside the run-to-run spread.  Either way the
            // pass is 6 us longer than one that stores keys - a million 4-byte reads all over a 4 MB table cost that wherever
            // they are issued; scan_reduce_kernel is 6 us shorter without them, and the emit kernel 7 us.)
            static_assert(!RANGES, "the depth sort records no ranges");
            // (the gathers are unconditional - a slot behind the chunk's items reads item 0's, the chunk holds one at least - so
            // that they compile to one straight run of loads with a single wait in front of the stores)
            uint32_t pos[ITEMS], id[ITEMS], c[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t j = (uint32_t)k * SORT_THREADS + threadIdx.x;
                const uint32_t jj = j < have ? j : 0u;
                const uint32_t d = (skey[jj] >> shift) & (BINS - 1);
                pos[k] = gbase[d] + (jj - lstart[d]);
                id[k] = sval[jj];
                c[k] = payload[id[k]];
            }
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t j = (uint32_t)k * SORT_THREADS + threadIdx.x;
                if (j < have) {
                    keys_out[pos[k]] = c[k];
                    vals_out[pos[k]] = id[k];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t j = (uint32_t)k * SORT_THREADS + threadIdx.x;
                if (j < have) {
                    const uint32_t kk = skey[j];
                    const uint32_t d = (kk >> shift) & (BINS - 1);
                    const uint32_t pos = gbase[d] + (j - lstart[d]);
                    keys_out[pos] = kk;
                    vals_out[pos] = sval[j];
                    if (RANGES) record_range(ranges_enc, kk, j == 0 || skey[j - 1] != kk, j + 1 == have || skey[j + 1] != kk, pos);
                }
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const size_t i = wbase + (size_t)k * 64 + lane;
            if (i < n) {
                const uint32_t d = digit_of(key[k]);
                const uint32_t pos = cnt[w][d] + rank[k];
                if constexpr (COUNTS) {
                    keys_out[pos] = pay[k];
                    vals_out[pos] = val[k];
                } else if constexpr (BUCKET) {
                    // the B side as pairs: keys_out is its 2P-word run, ONE 8-byte store an item where two 4-byte stores to unrelated
                    // lines went out (a workgroup's 2,048 keys fall into hundreds of buckets: no run of neighbours to merge)
                    reinterpret_cast<uint2*>(keys_out)[pos] = make_uint2(key[k], (uint32_t)i);
                } else {
                    keys_out[pos] = key[k];
                    vals_out[pos] = vals_in ? vals_in[i] : (uint32_t)i;
                }
            }
        }
    }
}


// =====================================================================================================
// Single-pass ("onesweep") radix passes with decoupled look-back.
//
// One launch per 8-bit digit.  The global digit histograms of ALL passes of a sort are produced up front in
// a single read of the keys (depth keys: sort_prologue_kernel; tile ids: derived from the per-tile counts by
// the last workgroup of emit_scan_kernel), so a pass is: take a ticket (virtual workgroup id = arrival order,
// which makes "every predecessor is resident or done" true whatever the hardware's dispatch order is), rank the
// chunk's items per digit, publish the chunk's 256 digit counts, look back over the predecessors' published
// counts (one thread per digit) until an inclusive prefix is found, scatter through an LDS-sorted image of
// the chunk (helpers: lookback.h).
template <int ITEMS, bool WRITE_KEYS, bool RANGES>
__global__ void __launch_bounds__(SORT_THREADS)
onesweep_pass_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                     uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out, size_t n, int shift,
                     const uint32_t* __restrict__ digit_totals, uint32_t* __restrict__ status,
                     uint32_t* __restrict__ ticket, uint2* __restrict__ ranges) {
    constexpr int BINS = 256;
    constexpr int CHUNK = SORT_THREADS * ITEMS;
    __shared__ uint32_t cnt[4][BINS];
    __shared__ uint32_t sh[8];
    __shared__ uint32_t gbase[BINS];     // global offset of this workgroup's run of digit d
    __shared__ uint32_t lstart[BINS];    // start of digit d inside the LDS-sorted chunk
    __shared__ uint32_t skey[CHUNK];
    __shared__ uint32_t sval[CHUNK];
    __shared__ uint32_t s_vb;
    volatile uint32_t* vcnt = &cnt[0][0];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_vb = atomicAdd(ticket, 1u);
    for (int d = threadIdx.x; d < 4 * BINS; d += SORT_THREADS) (&cnt[0][0])[d] = 0;
    __syncthreads();
    const uint32_t vb = s_vb;

    const size_t cbase = (size_t)vb * CHUNK;
    const size_t wbase = cbase + (size_t)w * (ITEMS * 64);
    uint32_t key[ITEMS];
    uint32_t rank[ITEMS];
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const size_t i = wbase + (size_t)k * 64 + lane;
        const bool valid = i < n;
        key[k] = valid ? keys_in[i] : 0xFFFFFFFFu;
        rank[k] = wave_digit_rank(valid, (key[k] >> shift) & (BINS - 1), 8, &vcnt[w * BINS], lt_mask);
    }
    __syncthreads();
    {   // thread d owns digit d
        const uint32_t d = threadIdx.x;
        const uint32_t blk = cnt[0][d] + cnt[1][d] + cnt[2][d] + cnt[3][d];
        const uint32_t total = digit_totals[d];
        const uint32_t digit_base = block_excl_scan_256(total, sh, nullptr);
        const uint32_t local_base = block_excl_scan_256(blk, sh, nullptr);
        const uint32_t before_me = lookback(status + d, BINS, vb, blk);
        gbase[d] = digit_base + before_me;
        lstart[d] = local_base;
        uint32_t r2 = local_base;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t c = cnt[k][d];
            cnt[k][d] = r2;
            r2 += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const size_t i = wbase + (size_t)k * 64 + lane;
        if (i < n) {
            const uint32_t d = (key[k] >> shift) & (BINS - 1);
            const uint32_t lp = cnt[w][d] + rank[k];
            skey[lp] = key[k];
            sval[lp] = vals_in ? vals_in[i] : (uint32_t)i;
        }
    }
    __syncthreads();
    const uint32_t have = (uint32_t)min((size_t)CHUNK, n - cbase);
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t j = (uint32_t)k * SORT_THREADS + threadIdx.x;
        if (j < have) {
            const uint32_t kk = skey[j];
            const uint32_t d = (kk >> shift) & (BINS - 1);
            const uint32_t pos = gbase[d] + (j - lstart[d]);
            if (WRITE_KEYS) keys_out[pos] = kk;
            vals_out[pos] = sval[j];
            if (RANGES) record_range(ranges, kk, j == 0 || skey[j - 1] != kk, j + 1 == have || skey[j + 1] != kk, pos);
        }
    }
}

// Before the depth sort: the four digit histograms of the depth keys in one read, the two instance totals
// (sum of the per-workgroup partials of preprocess_kernel; the host reads them back while the sort runs) and
// the zero-fill of every look-back status word the forward pass will use from the geometry buffer.
__global__ void __launch_bounds__(256)
sort_prologue_kernel(const uint32_t* __restrict__ keys, size_t n, uint32_t* __restrict__ depth_hist,
                     const uint32_t* __restrict__ partial, int n_partial, uint32_t* __restrict__ counters,
                     uint32_t* __restrict__ zero_words, size_t n_zero) {
    __shared__ uint32_t h[4][256];
    __shared__ uint32_t shc[2][4];
    for (int d = threadIdx.x; d < 1024; d += 256) (&h[0][0])[d] = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_zero; i += (size_t)gridDim.x * 256) zero_words[i] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * SCAN_CHUNK;
    uint32_t culled = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const size_t i = base + (size_t)k * 256 + threadIdx.x;
        if (i < n) {
            const uint32_t kk = keys[i];
            if (kk == 0xFFFFFFFFu) { culled++; continue; }      // culled Gaussians: one shared bin per digit
            atomicAdd(&h[0][kk & 255], 1u);
            atomicAdd(&h[1][(kk >> 8) & 255], 1u);
            atomicAdd(&h[2][(kk >> 16) & 255], 1u);
            atomicAdd(&h[3][kk >> 24], 1u);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) culled += (uint32_t)__shfl_xor((int)culled, d, 64);
    if ((threadIdx.x & 63) == 0 && culled)
        for (int p = 0; p < 4; p++) atomicAdd(&h[p][255], culled);
    __syncthreads();
    for (int p = 0; p < 4; p++) {
        const uint32_t c = h[p][threadIdx.x];
        if (c) atomicAdd(&depth_hist[p * 256 + threadIdx.x], c);
    }
    if (blockIdx.x == 0) {   // counters[0] = instances in our lists, counters[1] = the reference's count
        uint32_t v = 0, u = 0;
        for (int i = threadIdx.x; i < n_partial; i += 256) { v += partial[i]; u += partial[n_partial + i]; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            v += (uint32_t)__shfl_xor((int)v, d, 64);
            u += (uint32_t)__shfl_xor((int)u, d, 64);
        }
        if ((threadIdx.x & 63) == 0) { shc[0][threadIdx.x >> 6] = v; shc[1][threadIdx.x >> 6] = u; }
        __syncthreads();
        if (threadIdx.x == 0) {
            counters[1] = shc[0][0] + shc[0][1] + shc[0][2] + shc[0][3];
            counters[0] = shc[1][0] + shc[1][1] + shc[1][2] + shc[1][3];
            counters[3] = 0u;      // "carved for exactly counters[0] entries" (f3dgs_debug_read; the three-kernel flavour: run_totals_job)
        }
    }
}

__global__ void __launch_bounds__(256) iota_kernel(uint32_t* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (uint32_t)i;
}

}  // namespace

void launch_offset_sums(const uint32_t* in, const uint32_t* gather, size_t n, uint32_t* chunk_sums, uint32_t* sub,
                        hipStream_t s) {
    const size_t nb = scan_blocks(n);
    if (nb == 0) return;
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(256), 0, s, in, gather, n, chunk_sums, sub);
}

// =====================================================================================================
// Small problems (up to SMALL_SORT_MAX pairs: config c1, early training, inference on small scenes): the WHOLE stable sort in
// one launch of one workgroup, resident in LDS.  A multi-launch pass costs ~20 us of dependent launches whatever the size (c1:
// nine launches = 0.060 ms for 10,000 depth keys, three = 0.024 ms for 16,076 instances); here every 8-bit pass (lds_radix_pass,
// wg_sort.h) is: rank the thread's 16 items per wave (the ballot match of radix_scatter_kernel, wave-ordered LDS counters), turn the
// 16 x 256 counters into offsets, scatter the pairs into the LDS image, read them back in the new order - three barriers, no global
// round trip.
// The pairs live in registers between passes; the LDS image is written out once at the end (with the tile ranges, RANGES).
// (A first version of this idea - round 4, removed - ping-ponged the pairs through global memory behind fences: slower than the
// launches it replaced.)
// (SMALL_SORT_MAX = 16384: common.h)
constexpr int SMALL_SORT_THREADS = 1024;
constexpr int SMALL_SORT_ITEMS = SMALL_SORT_MAX / SMALL_SORT_THREADS;     // 16
using SmallSortLds = SortLds<SMALL_SORT_THREADS, SMALL_SORT_MAX>;
template <bool RANGES>
__global__ void __launch_bounds__(SMALL_SORT_THREADS)
small_sort_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t* __restrict__ keys_out,
                  uint32_t* __restrict__ vals_out, uint32_t n, int passes, TotalsJob tj, uint2* __restrict__ ranges_enc,
                  const uint32_t* __restrict__ n_dev, OffsetSumsJob os) {
    extern __shared__ __attribute__((aligned(16))) char small_sort_smem[];
    SmallSortLds& L = *reinterpret_cast<SmallSortLds*>(small_sort_smem);
    constexpr int ITEMS = SMALL_SORT_ITEMS;
    if (n_dev) { const uint32_t nd = *n_dev; n = nd <= n ? nd : 0u; }       // (sync-free forward) n is a capacity, the item count is the device's word; a frame that does not fit is void
    if (tj.partial) run_totals_job<SMALL_SORT_THREADS>(tj);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // item order: lds_radix_pass's (wg_sort.h), in `steps` <= 16 steps
    const int steps = (int)((n + SMALL_SORT_THREADS - 1) / SMALL_SORT_THREADS);
    const uint32_t wbase = (uint32_t)(w * steps * 64 + lane);
    uint32_t key[ITEMS], val[ITEMS], rank[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t i = wbase + (uint32_t)(k * 64);
        const bool mine = k < steps && i < n;
        key[k] = mine ? keys_in[i] : 0xFFFFFFFFu;
        val[k] = (vals_in && mine) ? vals_in[i] : i;
    }
    for (int pass = 0; pass < passes; pass++)
        lds_radix_pass<SMALL_SORT_THREADS, ITEMS>(L, key, val, rank, steps, n, 8 * pass, pass + 1 >= passes);
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const uint32_t j = (uint32_t)(k * SMALL_SORT_THREADS + tid);
        if (j < n) {
            const uint32_t kk = L.key[j];
            if (keys_out) keys_out[j] = kk;
            vals_out[j] = L.val[j];
            if (RANGES) record_range(ranges_enc, kk, j == 0 || L.key[j - 1] != kk, j + 1 == n || L.key[j + 1] != kk, j);
        }
    }
    if (os.tiles_touched) {
        // The list offsets in the NEW order (scan_reduce_kernel's two levels), from the sorted ids still in LDS: step k of wave w
        // covers items 1024 k + 64 w .. + 63 = run 16 k + w of the order, and a chunk of SCAN_CHUNK items is 64 consecutive runs.
        static_assert(SCAN_CHUNK == 64 * 64 && SMALL_SORT_THREADS == 1024, "run = item / 64, chunk = run / 64");
        const uint32_t nchunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
        uint32_t* const runs = &L.cnt[0][0];          // (the counters are done with: the last pass's barriers are behind us)
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t j = (uint32_t)(k * SMALL_SORT_THREADS + tid);
            uint32_t r = j < n ? os.tiles_touched[L.val[j]] : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) r += (uint32_t)__shfl_xor((int)r, d, 64);
            const uint32_t run = (uint32_t)(16 * k + w);
            if (lane == 0) {
                runs[run] = r;
                if (run < 64u * nchunks) os.sub[run] = r;
            }
        }
        __syncthreads();
        if ((uint32_t)tid < nchunks) {
            uint32_t t = 0;
            for (int q = 0; q < 64; q++) t += runs[64 * tid + q];
            os.chunk_sums[tid] = t;
        }
    }
}

__global__ void __launch_bounds__(256) totals_kernel(TotalsJob tj) { run_totals_job<256>(tj); }

// A kernel whose dynamic LDS is above the default limit: raised once per device (refused: the caller's other path takes over).
template <auto KERNEL>
bool raise_lds_limit(size_t bytes) {
    constexpr int MAX_DEV = 64;
    static std::atomic<int> state[MAX_DEV];      // 0: not asked yet, 1: usable, -1: refused (the ABI is re-entrant across threads)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return false;
    if (state[dev].load(std::memory_order_acquire) == 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) (void)hipGetLastError();
        state[dev].store(e == hipSuccess ? 1 : -1, std::memory_order_release);
    }
    return state[dev].load(std::memory_order_acquire) > 0;
}
// The one-launch sort's LDS image is 144 KB (refused: the multi-launch passes take over).
template <bool RANGES>
bool small_sort_usable() { return raise_lds_limit<&small_sort_kernel<RANGES>>(sizeof(SmallSortLds)); }

// =====================================================================================================
// Depth sort by buckets, second half (common.h: depth sort by buckets): behind the bucket pass - histogram, column scan and stable
// scatter on the bucket index, into the B side - every bucket is one contiguous run of (key, id) pairs in id order (pair_b: one
// uint2 an item, stored and loaded 8 bytes at a time), and ONE launch
// sorts them all, one workgroup per bucket, with the passes of small_sort_kernel (lds_radix_pass, wg_sort.h: ballot ranking,
// wave-ordered LDS counters, three barriers a pass, stable).  Inside a bucket the order of two keys is the order of the low s bits of key - kmin (the bits above
// are the bucket index), so a workgroup sorts those, and of those only the ones in which its keys differ: two 8-bit passes where
// the LSD sort of whole keys takes four.  The ids go to val_a and, in their place beside them in key_a, the tile counts
// payload[id] - what the LSD sort's last scatter hands on (COUNTS).
// The culled bucket (last bin) needs no sort - the stable scatter left it in id order - and is moved by DEPTH_BUCKET_COPY_GROUPS
// workgroups of their own.  A bucket above DEPTH_BUCKET_CAP pairs (every Gaussian at one depth, say) owns the same index range on
// both sides; its workgroup sorts it alone, in streaming LSD passes from one side to the other: slow, correct for any input, and
// no workgroup ever waits for another.
struct BucketSortLds : SortLds<DEPTH_BUCKET_THREADS, DEPTH_BUCKET_CAP> {
    uint32_t red[2][DEPTH_BUCKET_THREADS / 64];
};
static_assert(2 * sizeof(BucketSortLds) <= 160 * 1024, "two workgroups per CU");
static_assert(DEPTH_BUCKET_CAP >= 512, "the streaming passes keep their digit offsets in the key image");

// OR of v over the workgroup's threads (all of them call), in every thread; red: one word per wave
__device__ __forceinline__ uint32_t bucket_block_or(uint32_t v, uint32_t* red) {
    constexpr int NW = DEPTH_BUCKET_THREADS / 64;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) r |= red[k];
    return r;
}

// A bucket above the capacity: streaming LSD passes B -> A -> B -> ... over its own index range, an odd number of them.  The B side
// holds the bucket as n pairs, pair_b[off .. off + n): the first pass reads them as pairs; from then on those 2n words are the
// workgroup's private scratch, cut into a key half and an id half like the A side (sk / sv and dk / dv point at item 0 of the
// bucket on either side), so the later passes are the ping-pong of two arrays they always were.
__device__ __forceinline__ void depth_bucket_stream_sort(BucketSortLds& L, uint2* pair_b, uint32_t* key_a, uint32_t* val_a,
                                                      uint32_t off, uint32_t n, uint32_t kmin, uint32_t low, uint32_t rel0,
                                                      const uint32_t* __restrict__ payload) {
    constexpr int THREADS = DEPTH_BUCKET_THREADS, ITEMS = 8, NW = THREADS / 64;       // (chunks of eight items a thread: fewer registers than the in-LDS path holds)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    volatile uint32_t* vcnt = &L.cnt[w][0];
    const uint2* const pairs = pair_b + off;
    uint32_t diff = 0;
    for (uint32_t j = tid; j < n; j += THREADS) diff |= ((pairs[j].x - kmin) & low) ^ rel0;
    diff = bucket_block_or(diff, L.red[0]);
    int passes = (32 - __clz((int)diff) + 7) / 8;
    if ((passes & 1) == 0) passes++;          // (a pass on bits in which no two keys differ is a stable copy)
    uint32_t* const gbase = L.key;            // [256] next position of every digit
    uint32_t* const scratch = reinterpret_cast<uint32_t*>(pair_b + off);        // (2n words, 8-byte aligned whatever off and n are)
    uint32_t *sk = scratch, *sv = scratch + n, *dk = key_a + off, *dv = val_a + off;
    for (int pass = 0; pass < passes; pass++) {
        const int shift = 8 * pass;
        const bool last = pass + 1 == passes;
        const bool first = pass == 0;         // (the source is the pairs, not sk / sv)
        auto digit_of = [&](uint32_t kk) -> uint32_t { return shift < 32 ? (((kk - kmin) & low) >> shift) & 255u : 0u; };
        __syncthreads();
        if (tid < 256) gbase[tid] = 0;
        __syncthreads();
        for (uint32_t j = tid; j < n; j += THREADS) atomicAdd(&gbase[digit_of(first ? pairs[j].x : sk[j])], 1u);
        __syncthreads();
        digit_offsets(gbase, L.wsum);
        for (uint32_t c0 = 0; c0 < n; c0 += THREADS * ITEMS) {
            // chunk of THREADS x ITEMS items in order: wave w owns 64 ITEMS consecutive ones
            for (int d = tid; d < NW * 256; d += THREADS) (&L.cnt[0][0])[d] = 0;
            __syncthreads();       // counters cleared, gbase final
            const uint32_t wbase = c0 + (uint32_t)(w * ITEMS * 64 + lane);
            uint32_t key[ITEMS], val[ITEMS], rank[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t i = wbase + (uint32_t)(k * 64);
                const uint32_t ii = i < n ? i : 0u;
                if (first) { const uint2 p = pairs[ii]; key[k] = p.x; val[k] = p.y; }
                else { key[k] = sk[ii]; val[k] = sv[ii]; }
            }
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t i = wbase + (uint32_t)(k * 64);
                rank[k] = wave_digit_rank(i < n, digit_of(key[k]), 8, vcnt, lt_mask);
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t base = gbase[tid];
#pragma unroll
                for (int ww = 0; ww < NW; ww++) {
                    const uint32_t c = L.cnt[ww][tid];
                    L.cnt[ww][tid] = base;
                    base += c;
                }
                gbase[tid] = base;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t i = wbase + (uint32_t)(k * 64);
                if (i < n) {
                    const uint32_t pos = L.cnt[w][digit_of(key[k])] + rank[k];
                    dk[pos] = last ? payload[val[k]] : key[k];
                    dv[pos] = val[k];
                }
            }
            __syncthreads();       // every offset read before the next chunk clears the counters
        }
        // this pass's stores are read by the next one - by other waves of this workgroup: written back in front of the barrier, the
        // CU's cache dropped behind it
        __threadfence();
        __syncthreads();
        __threadfence();
        uint32_t* t = sk; sk = dk; dk = t;
        t = sv; sv = dv; dv = t;
    }
}

// (the three arrays are read AND written by the streaming passes: no __restrict__, no const)
__global__ void __launch_bounds__(DEPTH_BUCKET_THREADS, 4)      // (four waves per SIMD: two workgroups per CU)
depth_bucket_sort_kernel(uint2* pair_b, uint32_t* key_a, uint32_t* val_a, uint32_t bins,
                         const uint32_t* __restrict__ totals, const uint32_t* __restrict__ offs, uint32_t* __restrict__ ctl,
                         const uint32_t* __restrict__ payload, uint32_t* __restrict__ stats_host) {
    extern __shared__ __attribute__((aligned(16))) char bucket_sort_smem[];
    BucketSortLds& L = *reinterpret_cast<BucketSortLds*>(bucket_sort_smem);
    constexpr int THREADS = DEPTH_BUCKET_THREADS, ITEMS = DEPTH_BUCKET_ITEMS, NW = THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // The buckets are taken from the FAR end: the keys are float bits, a logarithmic scale, so a far bucket spans more depth and holds
    // more keys (c3: about 980 in the nearest octave's, 3,900 in the farthest's), and the 576 non-empty workgroups run on 512 slots - in
    // index order the longest sorts started last, behind everything else (0.0621 -> 0.0584 ms for the stage at c3)
    const uint32_t b = blockIdx.x < bins - 1u ? bins - 2u - blockIdx.x : blockIdx.x;
    if (b >= bins - 1u) {
        // the culled bucket: ids in id order already, moved to the A side with their tile counts
        const uint32_t off = offs[bins - 1u], n = totals[bins - 1u];
        for (uint32_t j = (b - (bins - 1u)) * THREADS + tid; j < n; j += DEPTH_BUCKET_COPY_GROUPS * THREADS) {
            const uint32_t id = pair_b[off + j].y;
            val_a[off + j] = id;
            key_a[off + j] = payload[id];
        }
        if (b == bins - 1u) {
            // the frame's largest sorted bucket and how many are above the capacity (f3dgs_depth_sort_info)
            uint32_t mx = 0, over = 0;
            for (uint32_t d = tid; d < bins - 1u; d += THREADS) {
                const uint32_t t = totals[d];
                mx = max(mx, t);
                over += t > (uint32_t)DEPTH_BUCKET_CAP ? 1u : 0u;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
                over += (uint32_t)__shfl_xor((int)over, d, 64);
            }
            if (lane == 0) { L.red[0][w] = mx; L.red[1][w] = over; }
            __syncthreads();
            if (tid == 0) {
                mx = 0; over = 0;
                for (int k = 0; k < NW; k++) { mx = max(mx, L.red[0][k]); over += L.red[1][k]; }
                ctl[2] = mx; ctl[3] = over;
                if (stats_host) {
                    __hip_atomic_store(&stats_host[0], mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(&stats_host[1], over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __threadfence_system();
                }
            }
        }
        return;
    }
    const uint32_t n = totals[b];
    if (n == 0) return;
    const uint32_t off = offs[b];
    const uint32_t kmin = ctl[0], bshift = ctl[1];
    const uint32_t low = (1u << bshift) - 1u;             // (the shift is 29 at most: depth_bucket_shift)
    const uint32_t rel0 = (pair_b[off].x - kmin) & low;

    if (n <= (uint32_t)DEPTH_BUCKET_CAP) {
        // item order: lds_radix_pass's, in `steps` steps
        const int steps = (int)((n + THREADS - 1) / THREADS);
        const uint32_t wbase = (uint32_t)(w * steps * 64 + lane);
        uint32_t key[ITEMS], val[ITEMS], rank[ITEMS];
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < ITEMS; k++) {
            const uint32_t i = wbase + (uint32_t)(k * 64);
            const bool mine = k < steps && i < n;
            const uint32_t ii = mine ? off + i : off;         // (unconditional: one run of requests)
            const uint2 p = pair_b[ii];                       // one 8-byte load an item
            val[k] = p.y;
            key[k] = mine ? (p.x - kmin) & low : rel0;
            diff |= key[k] ^ rel0;
        }
        diff = bucket_block_or(diff, L.red[0]);
        const int passes = (32 - __clz((int)diff) + 7) / 8;       // (diff == 0: __clz gives 32, no pass)
        if (passes == 0) {
            // one key throughout: the bucket is in order as it stands
#pragma unroll
            for (int k = 0; k < ITEMS; k++) {
                const uint32_t i = wbase + (uint32_t)(k * 64);
                if (k < steps && i < n) {
                    val_a[off + i] = val[k];
                    key_a[off + i] = payload[val[k]];
                }
            }
            return;
        }
        for (int pass = 0; pass < passes; pass++)
            lds_radix_pass<THREADS, ITEMS>(L, key, val, rank, steps, n, 8 * pass, pass + 1 >= passes);
        // out in the new order, eight items of a thread at a time: their gathers all go out before the first store
        constexpr int HALF = ITEMS / 2;
        for (int h = 0; h < 2; h++) {
            if ((uint32_t)(h * HALF * THREADS) >= n) break;
            uint32_t id[HALF], c[HALF];
#pragma unroll
            for (int k = 0; k < HALF; k++) {
                const uint32_t j = (uint32_t)((h * HALF + k) * THREADS + tid);
                id[k] = L.val[j < n ? j : 0u];
                c[k] = payload[id[k]];
            }
#pragma unroll
            for (int k = 0; k < HALF; k++) {
                const uint32_t j = (uint32_t)((h * HALF + k) * THREADS + tid);
                if (j < n) {
                    val_a[off + j] = id[k];
                    key_a[off + j] = c[k];
                }
            }
        }
        return;
    }

    depth_bucket_stream_sort(L, pair_b, key_a, val_a, off, n, kmin, low, rel0, payload);
}

bool depth_bucket_sort_usable() { return raise_lds_limit<&depth_bucket_sort_kernel>(sizeof(BucketSortLds)); }

// ITEMS = keys per thread: 8 for the depth sort (2048-key workgroups: P = 1M gives 489 workgroups, about two per CU;
// with 16 there are fewer workgroups than CUs and every pass is one latency chain: 0.116 -> 0.097 ms at c3), 16 for
// the tile sort (twice the instances, and the LDS reorder pays more on longer runs: 0.119 vs 0.128 ms with 8).
template <int BITS, int ITEMS>
static hipError_t radix_pass(const uint32_t* ki, const uint32_t* vi, uint32_t* ko, uint32_t* vo, size_t n, int shift,
                             uint32_t* hist, hipStream_t s, uint2* ranges_enc = nullptr, const TotalsJob* tj = nullptr,
                             const uint32_t* n_dev = nullptr, const uint32_t* payload = nullptr) {
    // `payload` (the depth sort's final pass): ko receives payload[value] instead of the key (radix_scatter_kernel, COUNTS)
    hipError_t rc = hipSuccess;
    constexpr int BINS = 1 << BITS;
    static_assert(ITEMS >= SORT_ITEMS, "the histogram buffers are sized for SORT_ITEMS keys per thread");
    const uint32_t nb = (uint32_t)((n + SORT_THREADS * ITEMS - 1) / (SORT_THREADS * ITEMS));
    uint32_t* totals = hist + (size_t)BINS * nb;
    hipLaunchKernelGGL((radix_hist_kernel<BITS, ITEMS>), dim3(nb), dim3(SORT_THREADS), 0, s, ki, n, shift, nb, hist,
                       tj ? *tj : TotalsJob{nullptr, 0, nullptr, nullptr}, n_dev, 0u, (uint32_t*)nullptr);
    if (tj && tj->ready) rc = hipEventRecord(tj->ready, s);        // the totals are final behind this launch
    hipLaunchKernelGGL(radix_rowscan_kernel, dim3(BINS), dim3(256), 0, s, hist, nb, totals);
    const uint32_t* const no_payload = nullptr;
    const uint32_t* const no_ctl = nullptr;
    uint32_t* const no_offs = nullptr;
    if constexpr (ITEMS == SORT_ITEMS && (BITS == RADIX_BITS || BITS == DEPTH_RADIX_BITS)) {        // the depth sort's shapes
        if (payload) {
            hipLaunchKernelGGL((radix_scatter_kernel<BITS, ITEMS, (BITS <= 8), false, true>), dim3(nb), dim3(SORT_THREADS), 0, s, ki,
                               vi, ko, vo, n, shift, nb, hist, totals, (uint2*)nullptr, n_dev, payload, no_ctl, no_offs);
            return rc;
        }
    }
    if (ranges_enc && BITS <= 8)
        hipLaunchKernelGGL((radix_scatter_kernel<BITS, ITEMS, true, true>), dim3(nb), dim3(SORT_THREADS), 0, s, ki, vi, ko, vo, n,
                           shift, nb, hist, totals, ranges_enc, n_dev, no_payload, no_ctl, no_offs);
    else
        hipLaunchKernelGGL((radix_scatter_kernel<BITS, ITEMS, (BITS <= 8), false>), dim3(nb), dim3(SORT_THREADS), 0, s, ki, vi, ko,
                           vo, n, shift, nb, hist, totals, (uint2*)nullptr, n_dev, no_payload, no_ctl, no_offs);
    return rc;
}

// The bucket pass of the depth sort, BITS = log2 of its bins: histogram (with the totals job and the key range), column scan, stable
// scatter of (key, id) pairs.  key_b / val_b: the B side, one run of 2n words (val_b = key_b + n) that receives the pairs; hist: the
// row-major matrix of nb rows; totals, offs, ctl: where the caller carved them behind it.
template <int BITS>
static hipError_t launch_bucket_pass(const uint32_t* keys, uint32_t* key_b, uint32_t* val_b, size_t n, uint32_t nb, uint32_t* hist,
                                     uint32_t* totals, uint32_t* offs, uint32_t* ctl, const TotalsJob& tj, uint32_t count,
                                     hipStream_t s) {
    constexpr uint32_t bins = 1u << BITS;
    const uint32_t* const none = nullptr;
    hipLaunchKernelGGL((radix_hist_kernel<BITS, SORT_ITEMS, true>), dim3(nb), dim3(SORT_THREADS), 0, s, keys, n, 0, nb, hist, tj, none,
                       count, ctl);
    hipError_t rc = hipSuccess;
    if (tj.ready) rc = hipEventRecord(tj.ready, s);        // the totals are final behind this launch
    hipLaunchKernelGGL(radix_colscan_kernel, dim3(bins / COLSCAN_BINS), dim3(COLSCAN_BINS * COLSCAN_ROW_LANES), 0, s, hist, nb, bins,
                       totals);
    hipLaunchKernelGGL((radix_scatter_kernel<BITS, SORT_ITEMS, false, false, false, true>), dim3(nb), dim3(SORT_THREADS), 0, s, keys,
                       none, key_b, val_b, n, 0, nb, hist, totals, (uint2*)nullptr, none, none, (const uint32_t*)ctl, offs);
    return rc;
}

// A tile-sort pass of `bits` bits (tile_digit_split: 4 ... 8; a single pass of fewer bits ranks 4, the upper ones are zero)
static void tile_radix_pass(int bits, const uint32_t* ki, const uint32_t* vi, uint32_t* ko, uint32_t* vo, size_t n, int shift,
                            uint32_t* hist, hipStream_t s, uint2* ranges_enc, const uint32_t* n_dev) {
    switch (bits) {
        case 8: (void)radix_pass<8, 16>(ki, vi, ko, vo, n, shift, hist, s, ranges_enc, nullptr, n_dev); break;
        case 7: (void)radix_pass<7, 16>(ki, vi, ko, vo, n, shift, hist, s, ranges_enc, nullptr, n_dev); break;
        case 6: (void)radix_pass<6, 16>(ki, vi, ko, vo, n, shift, hist, s, ranges_enc, nullptr, n_dev); break;
        case 5: (void)radix_pass<5, 16>(ki, vi, ko, vo, n, shift, hist, s, ranges_enc, nullptr, n_dev); break;
        default: (void)radix_pass<4, 16>(ki, vi, ko, vo, n, shift, hist, s, ranges_enc, nullptr, n_dev); break;
    }
}

void launch_radix_sort_pairs(uint32_t* key_a, uint32_t* val_a, uint32_t* key_b, uint32_t* val_b, size_t n, int nbits,
                             uint32_t* hist, bool result_in_a, uint2* ranges_enc, hipStream_t s, const uint32_t* n_dev) {
    // n_dev (sync-free forward, api.hip): `n` is the CAPACITY the buffers were carved for and every launch is sized by it; the
    // kernels take the item count from the device word (clamped to n)
    // Input is expected in A when (#passes even) == result_in_a, else in B; the caller arranges that.
    const int passes = (nbits + RADIX_BITS - 1) / RADIX_BITS;
    if (n == 0 || passes == 0) return;
    bool in_a = (passes % 2 == 0) ? result_in_a : !result_in_a;
    if (n <= (size_t)SMALL_SORT_MAX && (ranges_enc ? small_sort_usable<true>() : small_sort_usable<false>())) {
        // input where the caller put it for `passes` hops, result on the side it asked for - in one launch
        const uint32_t* ki = in_a ? key_a : key_b;
        const uint32_t* vi = in_a ? val_a : val_b;
        uint32_t* ko = result_in_a ? key_a : key_b;
        uint32_t* vo = result_in_a ? val_a : val_b;
        const TotalsJob none = {nullptr, 0, nullptr, nullptr};
        if (ranges_enc)
            hipLaunchKernelGGL(small_sort_kernel<true>, dim3(1), dim3(SMALL_SORT_THREADS), sizeof(SmallSortLds), s, ki, vi, ko, vo,
                               (uint32_t)n, passes, none, ranges_enc, n_dev, OffsetSumsJob{nullptr, nullptr, nullptr});
        else
            hipLaunchKernelGGL(small_sort_kernel<false>, dim3(1), dim3(SMALL_SORT_THREADS), sizeof(SmallSortLds), s, ki, vi, ko, vo,
                               (uint32_t)n, passes, none, (uint2*)nullptr, n_dev, OffsetSumsJob{nullptr, nullptr, nullptr});
        return;
    }
    // the multi-launch passes: the same number of them, digits as wide as the key needs (tile_digit_split, common.h); the one-launch
    // sort above keeps its 8-bit steps
    const DigitSplit split = tile_digit_split(nbits);
    for (int p = 0; p < passes; p++) {
        uint32_t* ki = in_a ? key_a : key_b;
        uint32_t* vi = in_a ? val_a : val_b;
        uint32_t* ko = in_a ? key_b : key_a;
        uint32_t* vo = in_a ? val_b : val_a;
        tile_radix_pass(split.width[p], ki, vi, ko, vo, n, split.shift[p], hist, s, p == passes - 1 ? ranges_enc : nullptr, n_dev);
        in_a = !in_a;
    }
}

// Depth sort of the Gaussians: 32-bit keys in `keys` (read-only), values = indices.  Up to SMALL_SORT_MAX keys: one launch; beyond,
// with `buckets`: one bucket pass and one launch that sorts the buckets (four launches); else three passes of 11/11/10 bits or,
// above 200,000 keys, four of 8.  The sorted ids end in val_a, and in key_a the sorted keys - or, given `counts_in_a`, what the
// frame reads next in that order: the tile counts (common.h).
hipError_t launch_depth_sort(const uint32_t* keys, uint32_t* key_a, uint32_t* val_a, uint32_t* key_b, uint32_t* val_b, size_t n,
                             uint32_t* hist, const TotalsJob* tj, hipStream_t s, const OffsetSumsJob* sums, bool* sums_done,
                             bool* counts_in_a, bool buckets, uint32_t* stats_host, DepthSortInfo* info) {
    if (sums_done) *sums_done = false;
    if (counts_in_a) *counts_in_a = false;
    if (info) *info = DepthSortInfo{F3DGS_DEPTH_SORT_NONE, 0u, 0u};
    if (n == 0) return hipSuccess;
    if (n <= (size_t)SMALL_SORT_MAX && small_sort_usable<false>()) {
        // the totals the host waits for go out in a launch of their own, in FRONT of the sort: behind it the host would sit out the
        // whole sort (0.04 ms) before it can enqueue the emit - and small scenes are bound by the host's enqueue time
        hipError_t rc = hipSuccess;
        // (no event to record = a call inside a graph capture: nobody waits on the host, the totals ride in the sort's launch -
        // one node less, ~4.5 us of a replayed c1 step)
        const bool apart = tj && tj->partial && tj->ready;
        if (apart) {
            hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(256), 0, s, *tj);
            rc = hipEventRecord(tj->ready, s);
        }
        hipLaunchKernelGGL(small_sort_kernel<false>, dim3(1), dim3(SMALL_SORT_THREADS), sizeof(SmallSortLds), s, keys, (const uint32_t*)nullptr,
                           key_a, val_a, (uint32_t)n, 4, (tj && tj->partial && !apart) ? *tj : TotalsJob{nullptr, 0, nullptr, nullptr},
                           (uint2*)nullptr, (const uint32_t*)nullptr, sums ? *sums : OffsetSumsJob{nullptr, nullptr, nullptr});
        if (sums && sums_done) *sums_done = true;
        if (info) info->path = F3DGS_DEPTH_SORT_ONE_LAUNCH;
        return rc;
    }
    // the last pass hands the tile counts on in the new order instead of the keys, where the caller can take them
    const uint32_t* const payload = (counts_in_a && sums) ? sums->tiles_touched : nullptr;
    // (the B side as one run of 2n words, 8-byte aligned: GeomState::carve)
    const bool b_is_one_run = val_b == key_b + n && (reinterpret_cast<uintptr_t>(key_b) & 7u) == 0;
    if (buckets && payload && tj && tj->partial && n < (1ull << 31) && b_is_one_run && depth_bucket_sort_usable()) {
        // four launches: the bucket pass into the B side (histogram - with the totals job and the key range -, column scan, stable
        // scatter of pairs), then every bucket sorted inside LDS into the A side (depth_bucket_sort_kernel)
        const uint32_t count = depth_bucket_count(n);
        const uint32_t nb = (uint32_t)((n + SORT_THREADS * SORT_ITEMS - 1) / (SORT_THREADS * SORT_ITEMS));
        const bool wide = depth_bucket_bits(n) == DEPTH_BUCKET_BITS_WIDE;
        const uint32_t bins = 1u << depth_bucket_bits(n);
        uint32_t* const totals = hist + (size_t)bins * nb;
        uint32_t* const offs = totals + bins;
        uint32_t* const ctl = offs + bins;
        const hipError_t rc = wide
            ? launch_bucket_pass<DEPTH_BUCKET_BITS_WIDE>(keys, key_b, val_b, n, nb, hist, totals, offs, ctl, *tj, count, s)
            : launch_bucket_pass<DEPTH_BUCKET_BITS>(keys, key_b, val_b, n, nb, hist, totals, offs, ctl, *tj, count, s);
        hipLaunchKernelGGL(depth_bucket_sort_kernel, dim3(bins - 1u + DEPTH_BUCKET_COPY_GROUPS), dim3(DEPTH_BUCKET_THREADS),
                           sizeof(BucketSortLds), s, reinterpret_cast<uint2*>(key_b), key_a, val_a, bins, (const uint32_t*)totals,
                           (const uint32_t*)offs, ctl,
                           payload, stats_host);
        *counts_in_a = true;
        if (info) *info = DepthSortInfo{F3DGS_DEPTH_SORT_BUCKETS, count, (uint32_t)DEPTH_BUCKET_CAP};
        return rc;
    }
    if (info) info->path = F3DGS_DEPTH_SORT_PASSES;
    if (n > 200000) {
        // large P: four 8-bit passes are faster than three 11-bit ones (measured at 1M: 0.105 vs 0.148 ms);
        // small P is launch-bound and prefers fewer passes.  Result must end in (key_a, val_a): A <- keys, then
        // A -> B -> A -> ... needs an odd number of remaining hops, so the first pass writes into B.
        const hipError_t rc = radix_pass<RADIX_BITS, SORT_ITEMS>(keys, nullptr, key_b, val_b, n, 0, hist, s, nullptr, tj);
        (void)radix_pass<RADIX_BITS, SORT_ITEMS>(key_b, val_b, key_a, val_a, n, 8, hist, s);
        (void)radix_pass<RADIX_BITS, SORT_ITEMS>(key_a, val_a, key_b, val_b, n, 16, hist, s);
        (void)radix_pass<RADIX_BITS, SORT_ITEMS>(key_b, val_b, key_a, val_a, n, 24, hist, s, nullptr, nullptr, nullptr, payload);
        if (payload) *counts_in_a = true;
        return rc;
    }
    const hipError_t rc = radix_pass<DEPTH_RADIX_BITS, SORT_ITEMS>(keys, nullptr, key_a, val_a, n, 0, hist, s, nullptr, tj);
    (void)radix_pass<DEPTH_RADIX_BITS, SORT_ITEMS>(key_a, val_a, key_b, val_b, n, DEPTH_RADIX_BITS, hist, s);
    (void)radix_pass<DEPTH_RADIX_BITS, SORT_ITEMS>(key_b, val_b, key_a, val_a, n, 2 * DEPTH_RADIX_BITS, hist, s, nullptr, nullptr, nullptr,
                                                   payload);
    if (payload) *counts_in_a = true;
    return rc;
}


void launch_sort_prologue(const GeomState& g, size_t P, hipStream_t s) {
    const size_t nb = scan_blocks(P);
    if (nb == 0) return;
    hipLaunchKernelGGL(sort_prologue_kernel, dim3(nb), dim3(256), 0, s, g.depth_key, P, g.depth_hist, g.ref_partial,
                       (int)((P + 255) / 256), g.counters, g.lb_words, g.n_lb_words);
}

// Depth sort, onesweep flavour: four 8-bit passes, one launch each; ids end in val_a (keys are not written by the
// last pass: nothing reads them).
void launch_depth_sort_onesweep(const GeomState& g, size_t n, hipStream_t s) {
    if (n == 0) return;
    const uint32_t nb = (uint32_t)depth_sort_blocks(n);
    uint32_t* st = g.depth_status;
    const size_t st_stride = (size_t)nb * 256;
    uint2* const no_ranges = nullptr;
    hipLaunchKernelGGL((onesweep_pass_kernel<DEPTH_SORT_ITEMS, true, false>), dim3(nb), dim3(SORT_THREADS), 0, s, g.depth_key,
                       (const uint32_t*)nullptr, g.key_b, g.val_b, n, 0, g.depth_hist, st, g.tickets + 0, no_ranges);
    hipLaunchKernelGGL((onesweep_pass_kernel<DEPTH_SORT_ITEMS, true, false>), dim3(nb), dim3(SORT_THREADS), 0, s, g.key_b,
                       g.val_b, g.key_a, g.val_a, n, 8, g.depth_hist + 256, st + st_stride, g.tickets + 1, no_ranges);
    hipLaunchKernelGGL((onesweep_pass_kernel<DEPTH_SORT_ITEMS, true, false>), dim3(nb), dim3(SORT_THREADS), 0, s, g.key_a,
                       g.val_a, g.key_b, g.val_b, n, 16, g.depth_hist + 512, st + 2 * st_stride, g.tickets + 2, no_ranges);
    hipLaunchKernelGGL((onesweep_pass_kernel<DEPTH_SORT_ITEMS, false, false>), dim3(nb), dim3(SORT_THREADS), 0, s, g.key_b,
                       g.val_b, g.key_a, g.val_a, n, 24, g.depth_hist + 768, st + 3 * st_stride, g.tickets + 3, no_ranges);
}

// Tile sort, onesweep flavour (ids only travel with their tile ids; `passes` = 1 or 2 digits of 8 bits).
// Input in (tile_tmp, id_tmp) for an odd number of passes, in (tile_sorted, point_list) for an even one; the
// result lands in (tile_sorted, point_list).
void launch_tile_sort_onesweep(const GeomState& g, const BinState& b, size_t n, int passes, uint2* ranges, hipStream_t s) {
    if (n == 0) return;
    const uint32_t nb = (uint32_t)sort_blocks(n);
    const size_t st_stride = (size_t)nb * 256;
    if (passes == 1) {
        hipLaunchKernelGGL((onesweep_pass_kernel<SORT_ITEMS, true, true>), dim3(nb), dim3(SORT_THREADS), 0, s, b.tile_tmp,
                           b.id_tmp, b.tile_sorted, b.point_list, n, 0, g.tile_hist, b.tile_status, g.tickets + 5, ranges);
        return;
    }
    hipLaunchKernelGGL((onesweep_pass_kernel<SORT_ITEMS, true, false>), dim3(nb), dim3(SORT_THREADS), 0, s, b.tile_sorted,
                       b.point_list, b.tile_tmp, b.id_tmp, n, 0, g.tile_hist, b.tile_status, g.tickets + 5, (uint2*)nullptr);
    hipLaunchKernelGGL((onesweep_pass_kernel<SORT_ITEMS, true, true>), dim3(nb), dim3(SORT_THREADS), 0, s, b.tile_tmp,
                       b.id_tmp, b.tile_sorted, b.point_list, n, 8, g.tile_hist + 256, b.tile_status + st_stride,
                       g.tickets + 6, ranges);
}

// Stable sort of (keys[i], i) on key bits [0, nbits): the sorted indices end in val_a (8-bit passes; `keys` is only read).
void launch_radix_sort_keys_to_order(const uint32_t* keys, uint32_t* key_a, uint32_t* val_a, uint32_t* key_b, uint32_t* val_b,
                                     size_t n, int nbits, uint32_t* hist, hipStream_t s) {
    const int passes = (nbits + RADIX_BITS - 1) / RADIX_BITS;
    if (n == 0 || passes == 0) return;
    bool to_a = (passes % 2) == 1;        // the last pass must write the A side
    const uint32_t* ki = keys;
    const uint32_t* vi = nullptr;
    for (int p = 0; p < passes; p++) {
        uint32_t* ko = to_a ? key_a : key_b;
        uint32_t* vo = to_a ? val_a : val_b;
        (void)radix_pass<RADIX_BITS, SORT_ITEMS>(ki, vi, ko, vo, n, p * RADIX_BITS, hist, s);
        ki = ko; vi = vo;
        to_a = !to_a;
    }
}

void launch_iota(uint32_t* dst, size_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(iota_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, n);
}

}  // namespace f3dgs
