// mask_regions.hip - small-region removal on bit-packed masks (include/f3dgs.h: f3dgs_mask_regions*): the reference's
// utils/amg.py:remove_small_regions (8-connected labelling, holes filled and islands dropped below an area) where the masks lie,
// without a dense label image.
//
// The graph's nodes are the maximal vertical RUNS of the polarity that is labelled (set bits for islands, clear bits of rows
// < FH for holes), cut at column ends and found from the packed words by shift-and-compare.  Per run four integers: its rows
// (y0 | y1 << 16), its parent, its area and its tie key y0 FW + x.  Run [a, b] of column x and run [c, d] of column x + 1 touch
// iff c <= b + 1 && d >= a - 1 (8-connectivity).  Kernels, one launch each:
//   regions_count_kernel    one workgroup per mask: the runs of every column and their exclusive prefix within the mask
//   regions_base_kernel     one workgroup: the masks' prefix (the first run of every mask), the total, the per-mask state cleared
//   regions_emit_kernel     one thread per (mask, column): the runs, every run its own parent
//   regions_link_kernel     one thread per (mask, pair of adjacent columns): a two-pointer walk down both run lists, a union for
//                           every touching pair.  A union links the LARGER root to the smaller by compare-and-swap: a parent is
//                           only ever lowered, a walk to the root visits strictly decreasing indices, and the root of a
//                           component is its smallest run.  Agent-scope atomics on both sides: other workgroups' links are seen.
//                           (find_root and unite live in union_find.h, shared with components.hip.)
//   regions_flatten_kernel  every run finds its root, points at it, and adds its area / lowers the root's key (integer atomics)
//   regions_decide_kernel   every root: the mask's components, its small ones, and the largest (ties: the smallest key) by one
//                           64-bit atomicMax of size << 32 | ~key
//   regions_rewrite_kernel  one workgroup per mask: `changed`, the new words (padding rows zero), and - from the words as they
//                           are written - the area and batched_mask_to_box's box
// Every loop is bounded by construction (a run list, a column, a grid stride); the walks of the union-find carry a cap of the
// number of runs besides, and a walk that reaches it sets the error word that f3dgs_mask_regions returns as F3DGS_ERR_HIP.  No
// workgroup waits for another: the stages are launches.  Integers only: two calls give the same bits.

#include <limits.h>
#include <string.h>

#include "common.h"
#include "union_find.h"

namespace f3dgs {

namespace {

constexpr int HDR = 4;                  // int32 words in front of the scratch: total runs (int64), error word, unused
constexpr int MAX_MASKS = 65535;        // grid.y
constexpr int MAX_EDGE = 32768;         // a row fits 15 bits: two of them in a word

struct Shape {
    int K, FH, FW, NW;
};

struct MaskState {
    int32_t n_comp, n_small;            // components of the labelled polarity; those below the threshold
    unsigned long long best;            // max over components of size << 32 | ~key
};

struct Runs {
    int32_t* hdr;
    MaskState* ms;                      // K
    int32_t* base;                      // K + 1: the first run of every mask; base[K] the total
    int32_t* local;                     // K x FW: the first run of a column, within its mask
    uint32_t* span;                     // per run: y0 | y1 << 16
    int32_t* parent;
    int32_t* area;
    int32_t* key;                       // y0 FW + x, lowered onto the root
    int32_t capacity;
};

__device__ __forceinline__ const uint32_t* mask_of(const uint32_t* packed, const int32_t* index, int k, int FW, int NW) {
    return packed + (size_t)(index ? index[k] : k) * FW * NW;
}

__device__ __forceinline__ uint32_t valid_bits(int wy, int FH) {
    const int nb = min(32, FH - 32 * wy);
    return nb == 32 ? 0xffffffffu : ((1u << nb) - 1u);
}

// the labelled polarity of word (x, wy): rows >= FH are neither foreground nor background
__device__ __forceinline__ uint32_t work_word(const uint32_t* __restrict__ pm, int x, int wy, int NW, int FH, int holes) {
    const uint32_t w = pm[(size_t)x * NW + wy];
    return (holes ? ~w : w) & valid_bits(wy, FH);
}

__device__ __forceinline__ long long total_runs(const int32_t* hdr) { return *reinterpret_cast<const long long*>(hdr); }

__device__ __forceinline__ int col_begin(const Runs& r, const Shape& s, int k, int x) { return r.base[k] + r.local[(size_t)k * s.FW + x]; }
__device__ __forceinline__ int col_end(const Runs& r, const Shape& s, int k, int x) { return x + 1 < s.FW ? col_begin(r, s, k, x + 1) : r.base[k + 1]; }

__global__ void __launch_bounds__(256) regions_count_kernel(Shape s, const uint32_t* __restrict__ packed, const int32_t* __restrict__ index,
                                                            int holes, int32_t* __restrict__ local, int32_t* __restrict__ totals) {
    __shared__ int s_w[4];
    const int k = blockIdx.x;
    const uint32_t* const pm = mask_of(packed, index, k, s.FW, s.NW);
    int run = 0;
    for (int x0 = 0; x0 < s.FW; x0 += 256) {
        const int x = x0 + threadIdx.x;
        int n = 0;
        if (x < s.FW) {
            uint32_t prev = 0u;
            for (int wy = 0; wy < s.NW; wy++) {
                const uint32_t v = work_word(pm, x, wy, s.NW, s.FH, holes);
                n += __popc(v & ~((v << 1) | prev));                      // the run starts
                prev = v >> 31;
            }
        }
        int total;
        const int before = block_scan(n, s_w, total);
        if (x < s.FW) local[(size_t)k * s.FW + x] = run + before;
        run += total;
    }
    if (threadIdx.x == 0) totals[k] = run;
}

// base[k] = the runs of the masks before k (in place over the totals), base[K] and hdr = the total; the state of every mask cleared
__global__ void __launch_bounds__(256) regions_base_kernel(int K, Runs r) {
    __shared__ long long s_w[4];
    long long run = 0;
    for (int k0 = 0; k0 < K; k0 += 256) {
        const int k = k0 + threadIdx.x;
        const long long n = k < K ? r.base[k] : 0;
        long long total;
        const long long before = block_scan(n, s_w, total);
        if (k < K) {
            r.base[k] = (int32_t)min(run + before, (long long)INT_MAX);      // (beyond the capacity nothing reads it)
            r.ms[k] = MaskState{0, 0, 0ull};
        }
        run += total;
    }
    if (threadIdx.x == 0) {
        r.base[K] = (int32_t)min(run, (long long)INT_MAX);
        *reinterpret_cast<long long*>(r.hdr) = run;
        r.hdr[2] = 0;
        r.hdr[3] = 0;
    }
}

__global__ void __launch_bounds__(256) regions_emit_kernel(Shape s, const uint32_t* __restrict__ packed, const int32_t* __restrict__ index,
                                                           int holes, Runs r) {
    if (total_runs(r.hdr) > r.capacity) return;                            // (the caller sees the total and comes again with room)
    const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (x >= s.FW) return;
    const uint32_t* const pm = mask_of(packed, index, k, s.FW, s.NW);
    int at = col_begin(r, s, k, x);
    int open = -1;                                                         // the first row of a run that began in an earlier word
    uint32_t prev = 0u;
    uint32_t v = work_word(pm, x, 0, s.NW, s.FH, holes);
    for (int wy = 0; wy < s.NW; wy++) {
        const uint32_t next = wy + 1 < s.NW ? work_word(pm, x, wy + 1, s.NW, s.FH, holes) : 0u;
        uint32_t starts = v & ~((v << 1) | prev);
        uint32_t ends = v & ~((v >> 1) | (next << 31));
        for (; ends; ends &= ends - 1u) {
            const int y1 = 32 * wy + (int)__builtin_ctz(ends);
            int y0 = open;
            if (open >= 0) {
                open = -1;
            } else {
                y0 = 32 * wy + (int)__builtin_ctz(starts);
                starts &= starts - 1u;
            }
            if (at < r.capacity) {                                         // (always: the bound guards the stores)
                r.span[at] = (uint32_t)y0 | ((uint32_t)y1 << 16);
                r.parent[at] = at;
                r.area[at] = y1 - y0 + 1;
                r.key[at] = y0 * s.FW + x;
            }
            at++;
        }
        if (starts) open = 32 * wy + (int)__builtin_ctz(starts);            // (at most one start is left: the run goes on)
        prev = v >> 31;
        v = next;
    }
}

__global__ void __launch_bounds__(256) regions_link_kernel(Shape s, Runs r) {
    const long long total = total_runs(r.hdr);
    if (total > r.capacity) return;
    const int x = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (x + 1 >= s.FW) return;
    int i = col_begin(r, s, k, x);
    const int i_end = col_begin(r, s, k, x + 1);
    int j = i_end;
    const int j_end = col_end(r, s, k, x + 1);
    const int steps = (i_end - i) + (j_end - j);
    for (int it = 0; it < steps && i < i_end && j < j_end; it++) {
        const uint32_t si = r.span[i], sj = r.span[j];
        const int a = (int)(si & 0xffffu), b = (int)(si >> 16), c = (int)(sj & 0xffffu), d = (int)(sj >> 16);
        if (c <= b + 1 && d >= a - 1) unite(r.parent, i, j, (int)total, r.hdr + 2);
        if (b <= d) i++;                                                   // (the run that ends first can touch nothing further down)
        else j++;
    }
}

__global__ void __launch_bounds__(256) regions_flatten_kernel(Runs r) {
    const long long total = total_runs(r.hdr);
    if (total > r.capacity) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (int)total; i += gridDim.x * 256) {
        const int root = find_root(r.parent, i, (int)total, r.hdr + 2);
        if (root < 0 || root == i) continue;
        atomicAdd(r.area + root, r.area[i]);                               // (a run that is no root receives nothing)
        atomicMin(r.key + root, r.key[i]);
        __hip_atomic_store(r.parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(256) regions_decide_kernel(int K, double area_thresh, Runs r) {
    const long long total = total_runs(r.hdr);
    if (total > r.capacity) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < (int)total; i += gridDim.x * 256) {
        if (r.parent[i] != i) continue;
        int lo = 0, hi = K;                                                // the mask of run i: the last k with base[k] <= i
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (r.base[mid] <= i) lo = mid;
            else hi = mid;
        }
        const int size = r.area[i];
        atomicAdd(&r.ms[lo].n_comp, 1);
        if ((double)size < area_thresh) atomicAdd(&r.ms[lo].n_small, 1);
        atomicMax(&r.ms[lo].best, ((unsigned long long)(uint32_t)size << 32) | (uint32_t)~(uint32_t)r.key[i]);
    }
}

__global__ void __launch_bounds__(256) regions_rewrite_kernel(Shape s, const uint32_t* __restrict__ packed, const int32_t* __restrict__ index,
                                                              int holes, double area_thresh, Runs r, uint32_t* __restrict__ out,
                                                              unsigned char* __restrict__ changed, int32_t* __restrict__ area,
                                                              int32_t* __restrict__ box) {
    __shared__ int s_area, s_x0, s_y0, s_x1, s_y1;
    if (total_runs(r.hdr) > r.capacity) return;
    const int k = blockIdx.x;
    const uint32_t* const pm = mask_of(packed, index, k, s.FW, s.NW);
    uint32_t* const po = out + (size_t)k * s.FW * s.NW;
    const MaskState ms = r.ms[k];
    const bool edit = ms.n_small > 0;
    const bool all_small = !holes && ms.n_small == ms.n_comp;              // islands, every one small: the largest stays
    const int best_size = (int)(ms.best >> 32), best_key = (int)~(uint32_t)ms.best;
    if (threadIdx.x == 0) {
        s_area = 0;
        s_x0 = s_y0 = INT_MAX;
        s_x1 = s_y1 = -1;
        changed[k] = edit ? 1 : 0;
    }
    __syncthreads();
    int n = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int x = threadIdx.x; x < s.FW; x += 256) {
        int at = edit ? col_begin(r, s, k, x) : 0;
        const int at_end = edit ? col_end(r, s, k, x) : 0;
        for (int wy = 0; wy < s.NW; wy++) {
            uint32_t w = pm[(size_t)x * s.NW + wy] & valid_bits(wy, s.FH);
            const int lo = 32 * wy, hi = lo + 31;
            while (at < at_end) {                                          // the runs that reach into this word
                const uint32_t sp = r.span[at];
                const int a = (int)(sp & 0xffffu), b = (int)(sp >> 16);
                if (a > hi) break;
                const int root = r.parent[at];
                const int size = r.area[root];
                const bool hit = all_small ? !(size == best_size && r.key[root] == best_key) : (double)size < area_thresh;
                if (hit) {
                    const int b0 = max(a, lo) - lo, len = min(b, hi) - lo - b0 + 1;
                    const uint32_t m = (len == 32 ? 0xffffffffu : ((1u << len) - 1u)) << b0;
                    w = holes ? (w | m) : (w & ~m);
                }
                if (b > hi) break;                                         // (it goes on in the next word)
                at++;
            }
            po[(size_t)x * s.NW + wy] = w;
            if (w) {
                n += __popc(w);
                x0 = min(x0, x);
                x1 = max(x1, x);
                y0 = min(y0, lo + (int)__builtin_ctz(w));
                y1 = max(y1, hi - (int)__builtin_clz(w));
            }
        }
    }
    if (n) {
        atomicAdd(&s_area, n);
        atomicMin(&s_x0, x0);
        atomicMin(&s_y0, y0);
        atomicMax(&s_x1, x1);
        atomicMax(&s_y1, y1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool any = s_area > 0;                                       // batched_mask_to_box: [0, 0, 0, 0] for an empty mask
        area[k] = s_area;
        box[4 * k + 0] = any ? s_x0 : 0;
        box[4 * k + 1] = any ? s_y0 : 0;
        box[4 * k + 2] = any ? s_x1 : 0;
        box[4 * k + 3] = any ? s_y1 : 0;
    }
}

size_t scratch_ints(int K, int FW, int64_t capacity) {
    return (size_t)HDR + 4 * (size_t)K + ((size_t)K + 1) + (size_t)K * FW + 4 * (size_t)capacity;
}

int check_shape(const char* who, int K, int FH, int FW, int64_t capacity) {
    if (K < 0 || FH < 1 || FW < 1 || capacity < 0)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: bad sizes K=%d FH=%d FW=%d run_capacity=%lld", who, K, FH, FW, (long long)capacity);
    if (K > MAX_MASKS) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: K=%d masks: up to %d per call are supported", who, K, MAX_MASKS);
    if (FH > MAX_EDGE || FW > MAX_EDGE || (size_t)FH * FW > 0x3fffffffull)
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: frames of %d x %d pixels: edges up to %d and up to 2^30 pixels are supported", who, FH, FW, MAX_EDGE);
    if (capacity > INT_MAX) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: run_capacity %lld: up to 2^31 - 1 runs are supported", who, (long long)capacity);
    return F3DGS_OK;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_mask_regions_scratch_bytes(int K, int FW, int64_t run_capacity) {
    if (K < 1 || K > MAX_MASKS || FW < 1 || FW > MAX_EDGE || run_capacity < 0 || run_capacity > INT_MAX) return 0;
    return scratch_ints(K, FW, run_capacity) * sizeof(int32_t);
}

int f3dgs_mask_regions(int K, int FH, int FW, const uint32_t* packed, const int32_t* index, int holes, double area_thresh,
                       int64_t run_capacity, uint32_t* out, unsigned char* changed, int32_t* area, int32_t* box, int64_t* runs,
                       void* scratch, void* stream) {
    if (const int rc = check_shape("mask_regions", K, FH, FW, run_capacity)) return rc;
    if (!(area_thresh >= 0.0) || area_thresh > 1e300)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_regions: area_thresh %g: a finite number >= 0 expected", area_thresh);
    if (!runs) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_regions: null pointer");
    *runs = 0;
    if (K == 0) return F3DGS_OK;
    if (!packed || !out || !changed || !area || !box || !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_regions: null pointer");
    if (reinterpret_cast<uintptr_t>(scratch) & 7u) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_regions: scratch must be 8-byte aligned");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Shape s{K, FH, FW, (FH + 31) / 32};
    int32_t* const w = static_cast<int32_t*>(scratch);
    Runs r;
    r.hdr = w;
    r.ms = reinterpret_cast<MaskState*>(w + HDR);
    r.base = w + HDR + 4 * (size_t)K;
    r.local = r.base + K + 1;
    r.span = reinterpret_cast<uint32_t*>(r.local + (size_t)K * FW);
    r.parent = reinterpret_cast<int32_t*>(r.span) + run_capacity;
    r.area = r.parent + run_capacity;
    r.key = r.area + run_capacity;
    r.capacity = (int32_t)run_capacity;
    const int hl = holes ? 1 : 0;
    const unsigned col_blocks = (unsigned)((FW + 255) / 256);
    const unsigned run_blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((run_capacity + 255) / 256, 1), 4096);
    hipLaunchKernelGGL(regions_count_kernel, dim3(K), dim3(256), 0, st, s, packed, index, hl, r.local, r.base);
    hipLaunchKernelGGL(regions_base_kernel, dim3(1), dim3(256), 0, st, K, r);
    hipLaunchKernelGGL(regions_emit_kernel, dim3(col_blocks, K), dim3(256), 0, st, s, packed, index, hl, r);
    if (FW > 1) hipLaunchKernelGGL(regions_link_kernel, dim3((unsigned)((FW - 1 + 255) / 256), K), dim3(256), 0, st, s, r);
    hipLaunchKernelGGL(regions_flatten_kernel, dim3(run_blocks), dim3(256), 0, st, r);
    hipLaunchKernelGGL(regions_decide_kernel, dim3(run_blocks), dim3(256), 0, st, K, area_thresh, r);
    hipLaunchKernelGGL(regions_rewrite_kernel, dim3(K), dim3(256), 0, st, s, packed, index, hl, area_thresh, r, out, changed, area, box);
    hipError_t e = hipGetLastError();
    int32_t hdr[HDR] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(hdr, r.hdr, sizeof(hdr), hipMemcpyDeviceToHost, st);      // the host read: total and error word
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "mask_regions: %s", hipGetErrorString(e));
    long long total;
    memcpy(&total, hdr, sizeof(total));
    *runs = total;
    if (hdr[2]) return report_errorf(F3DGS_ERR_HIP, "mask_regions: a union-find walk reached its bound of %lld runs (error word %d)", total, hdr[2]);
    return F3DGS_OK;
}

}  // extern "C"
