// components.hip - connected components of the points over their K-nearest-neighbour lists (include/f3dgs.h:
// f3dgs_knn_components, f3dgs_component_filter): what turns the lists of neighbors.hip into a graph.
//
// Slot s of row i is a directed edge i -> j = idx[i, s] when 0 <= j < P, j != i, both ends are active (labels NULL or >= 0) and
// carry the same label, and - with a finite max_dist2 - dist2[i, s] <= max_dist2 (the mode filter's comparison: a NaN gives no
// edge).  The graph is undirected: {i, j} is an edge if either direction holds, with `mutual` only if both do, each judged on its
// own slot.  Kernels, one launch each:
//   comp_init_kernel      every node its own parent, -1 if inactive; its count 0; the status word 0
//   comp_link_slot_kernel a union per edge, one thread per (node, slot): the shape f3dgs_knn_components runs, the faster one at every
//                         K measured (profiles/components_bench.md).  comp_link_kernel, one thread per node with its row in
//                         registers, stays behind f3dgs_debug_knn_components_shape.  The union-find is union_find.h's, shared with
//                         mask_regions.hip
//   comp_flatten_kernel   every node finds its root, points at it, and is counted at the root: ONE atomicAdd per distinct root per
//                         wave (a ballot loop over the distinct roots among the 64 lanes) - a scene without labels is one
//                         component, and a million adds on one word are what this loop avoids
//   comp_spread_kernel    size[i] = the count at root[i]
//   dense ids             comp_count_kernel (roots per block of 1024 nodes), comp_scan_kernel (one workgroup: the exclusive prefix
//                         of the block sums, n_comp), comp_rank_kernel (the prefix within the block: comp and comp_root of the
//                         roots, -1 behind n_comp), comp_ids_kernel (comp of everybody else)
//   filter                filter_clear_kernel, filter_best_kernel (roots only: a 64-bit atomicMax of size << 32 | ~root per
//                         label), filter_apply_kernel
// `root` IS the parent array and `size` IS the count array: the graph stage needs no table of its own.  No workgroup waits for
// another; every loop is bounded by construction or by the cap of P of the union-find's walks.  Integers only: two calls give
// the same bits.

#include <limits.h>
#include <math.h>

#include "common.h"
#include "union_find.h"

namespace f3dgs {

namespace {

constexpr int SCAN_ROUNDS = 4;                       // a block of the dense ids: 4 rounds of 256 nodes
constexpr int SCAN_BLOCK = 256 * SCAN_ROUNDS;

struct Graph {
    int P, K;
    const int32_t* idx;
    const float* dist2;                              // read only when `limited`
    float max_dist2;
    const int32_t* labels;                           // or NULL: every node active, label 0
    bool limited, mutual;
};

__global__ void __launch_bounds__(256) comp_init_kernel(int P, const int32_t* __restrict__ labels, int32_t* __restrict__ root,
                                                        int32_t* __restrict__ size, int32_t* __restrict__ n_comp,
                                                        int32_t* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        *status = 0;
        if (n_comp) *n_comp = 0;
    }
    if (i >= P) return;
    root[i] = (!labels || labels[i] >= 0) ? i : -1;
    size[i] = 0;
}

// does row j hold i in a slot that is an edge by its own distance?  (the labels are symmetric: the caller has compared them)
__device__ __forceinline__ bool points_back(const Graph& g, int j, int i) {
    bool back = false;
    for (int t = 0; t < g.K; t++) {
        const size_t at = (size_t)j * g.K + t;
        back = back || (g.idx[at] == i && (!g.limited || g.dist2[at] <= g.max_dist2));
    }
    return back;
}

// slot `at` of row i (label li >= 0) as an edge: its other end, or -1
__device__ __forceinline__ int edge_of(const Graph& g, int i, int li, int j, size_t at) {
    if (j < 0 || j >= g.P || j == i) return -1;                              // idx is the caller's: nothing is read out of bounds
    if (g.limited && !(g.dist2[at] <= g.max_dist2)) return -1;
    if (g.labels && g.labels[j] != li) return -1;
    if (g.mutual && (j < i || !points_back(g, j, i))) return -1;            // (a mutual edge is seen from both ends: the lower one links)
    return j;
}

// one thread per node, the LS slots of its row loaded before the first union
template <int LS>
__global__ void __launch_bounds__(256) comp_link_kernel(Graph g, int32_t* __restrict__ parent, int32_t* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.P) return;
    const int li = g.labels ? g.labels[i] : 0;
    if (li < 0) return;
    int nb[LS];
#pragma unroll
    for (int s = 0; s < LS; s++) nb[s] = s < g.K ? g.idx[(size_t)i * g.K + s] : -1;
#pragma unroll
    for (int s = 0; s < LS; s++) {
        const int j = edge_of(g, i, li, nb[s], (size_t)i * g.K + s);
        if (j >= 0) unite(parent, i, j, g.P, status);
    }
}

// one thread per (node, slot)
__global__ void __launch_bounds__(256) comp_link_slot_kernel(Graph g, int32_t* __restrict__ parent, int32_t* __restrict__ status) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)g.P * g.K) return;
    const int i = (int)(at / g.K);
    const int li = g.labels ? g.labels[i] : 0;
    if (li < 0) return;
    const int j = edge_of(g, i, li, g.idx[at], at);
    if (j >= 0) unite(parent, i, j, g.P, status);
}

__global__ void __launch_bounds__(256) comp_flatten_kernel(int P, int32_t* __restrict__ root, int32_t* __restrict__ size,
                                                           int32_t* __restrict__ status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int r = -1;
    if (i < P && load_agent(root + i) >= 0) {
        r = find_root(root, i, P, status);
        if (r >= 0 && r != i) __hip_atomic_store(root + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the count: every distinct root among the lanes once.  At most 64 rounds, one to three where neighbours share components.
    bool pending = r >= 0;
    for (int round = 0; round < 64; round++) {
        const unsigned long long left = __ballot(pending);
        if (!left) break;
        const int leader = __ffsll((long long)left) - 1;
        const int lr = __shfl(r, leader);
        const bool same = pending && r == lr;
        const unsigned long long members = __ballot(same);
        if (lane == leader) atomicAdd(size + lr, __popcll(members));
        pending = pending && !same;
    }
}

__global__ void __launch_bounds__(256) comp_spread_kernel(int P, const int32_t* __restrict__ root, int32_t* __restrict__ size) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = root[i];
    if (r >= 0 && r < i) size[i] = size[r];                                  // (a root keeps its count; nobody writes a root's)
}

__global__ void __launch_bounds__(256) comp_count_kernel(int P, const int32_t* __restrict__ root, int32_t* __restrict__ sums) {
    __shared__ int s_w[4];
    int n = 0;
    for (int k = 0; k < SCAN_ROUNDS; k++) {
        const int i = blockIdx.x * SCAN_BLOCK + k * 256 + threadIdx.x;
        n += (i < P && root[i] == i) ? 1 : 0;
    }
    int total;
    block_scan(n, s_w, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the block sums become their exclusive prefix, in place; n_comp the total
__global__ void __launch_bounds__(256) comp_scan_kernel(int n_blocks, int32_t* __restrict__ sums, int32_t* __restrict__ n_comp) {
    __shared__ int s_w[4];
    int run = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int n = b < n_blocks ? sums[b] : 0;
        int total;
        const int before = block_scan(n, s_w, total);
        if (b < n_blocks) sums[b] = run + before;
        run += total;
    }
    if (threadIdx.x == 0) *n_comp = run;
}

__global__ void __launch_bounds__(256) comp_rank_kernel(int P, const int32_t* __restrict__ root, const int32_t* __restrict__ sums,
                                                        const int32_t* __restrict__ n_comp, int32_t* __restrict__ comp,
                                                        int32_t* __restrict__ comp_root) {
    __shared__ int s_w[4];
    const int n = *n_comp;
    int run = sums[blockIdx.x];
    for (int k = 0; k < SCAN_ROUNDS; k++) {
        const int i = blockIdx.x * SCAN_BLOCK + k * 256 + threadIdx.x;
        const bool is_root = i < P && root[i] == i;
        int total;
        const int before = block_scan(is_root ? 1 : 0, s_w, total);
        if (is_root) {
            const int c = run + before;                                      // < n_comp <= P
            comp[i] = c;
            comp_root[c] = i;
        }
        if (i < P && i >= n) comp_root[i] = -1;                              // (the roots write in front of n_comp only)
        run += total;
    }
}

__global__ void __launch_bounds__(256) comp_ids_kernel(int P, const int32_t* __restrict__ root, int32_t* __restrict__ comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = root[i];
    if (r < 0) comp[i] = -1;
    else if (r < i) comp[i] = comp[r];                                       // (a root's was written by the launch before)
}

__device__ __forceinline__ unsigned long long best_key(int size, int root) {
    return ((unsigned long long)(uint32_t)size << 32) | (uint32_t)~(uint32_t)root;
}

__global__ void __launch_bounds__(256) filter_clear_kernel(int num_labels, unsigned long long* __restrict__ best) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < num_labels) best[l] = 0ull;
}

__global__ void __launch_bounds__(256) filter_best_kernel(int P, const int32_t* __restrict__ labels, const int32_t* __restrict__ root,
                                                          const int32_t* __restrict__ size, int num_labels,
                                                          unsigned long long* __restrict__ best) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P || root[i] != i) return;
    const int l = labels ? labels[i] : 0;
    if (l >= 0 && l < num_labels) atomicMax(best + l, best_key(size[i], i));
}

__global__ void __launch_bounds__(256) filter_apply_kernel(int P, const int32_t* labels, const int32_t* __restrict__ root,
                                                           const int32_t* __restrict__ size, int min_size, bool largest, int num_labels,
                                                           const unsigned long long* __restrict__ best, int32_t* labels_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int l = labels ? labels[i] : 0;                                    // (labels_out may be labels: read before the store)
    bool keep = l >= 0 && size[i] >= min_size;
    if (keep && largest) keep = l < num_labels && best[l] == best_key(size[i], root[i]);
    labels_out[i] = keep ? l : -1;
}

unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

size_t best_bytes(int num_labels) { return (size_t)(num_labels > 0 ? num_labels : 0) * sizeof(unsigned long long); }

int check_lists(const char* who, int P, int K) {
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (K < 1 || K > F3DGS_KNN_MAX_NEIGHBORS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: K = %d neighbours, 1 .. %d are taken", who, K, F3DGS_KNN_MAX_NEIGHBORS);
    if (P > (1 << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
    return F3DGS_OK;
}

// shape: 0 one thread per node, 1 one thread per (node, slot), 2 no link at all (the floor of the other stages, for measurements)
int run_components(const char* who, int P, int K, const int32_t* idx, const float* dist2, float max_dist2, const int32_t* labels,
                   int mutual, int shape, int32_t* root, int32_t* size, int32_t* comp, int32_t* comp_root, int32_t* n_comp,
                   int32_t* status, void* scratch, void* stream) {
    if (const int rc = check_lists(who, P, K)) return rc;
    if (!(max_dist2 >= 0.f)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: max_dist2 is negative or NaN", who);
    if (!status) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (P > 0) {
        if (!idx || !root || !size) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
        if (root == size) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: root is size: two outputs need two arrays", who);
        if (max_dist2 < INFINITY && !dist2) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a finite max_dist2 needs dist2", who);
        if (comp) {
            if (!comp_root || !n_comp || !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (comp goes with comp_root, n_comp and scratch)", who);
            if (comp == root || comp == size || comp_root == root || comp_root == size || comp_root == comp)
                return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: comp and comp_root need arrays of their own", who);
            if (reinterpret_cast<uintptr_t>(scratch) & 7u) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 8-byte aligned", who);
        }
    }
    const unsigned nodes = std::max(blocks_of((size_t)P, 256), 1u);
    hipLaunchKernelGGL(comp_init_kernel, dim3(nodes), dim3(256), 0, st, P, labels, root, size, (comp || P == 0) ? n_comp : nullptr, status);
    if (P > 0) {
        Graph g{P, K, idx, dist2, max_dist2, labels, max_dist2 < INFINITY, mutual != 0};
        if (shape == 1)
            hipLaunchKernelGGL(comp_link_slot_kernel, dim3(blocks_of((size_t)P * K, 256)), dim3(256), 0, st, g, root, status);
        else if (shape == 0 && K <= 4)
            hipLaunchKernelGGL(comp_link_kernel<4>, dim3(nodes), dim3(256), 0, st, g, root, status);
        else if (shape == 0 && K <= 8)
            hipLaunchKernelGGL(comp_link_kernel<8>, dim3(nodes), dim3(256), 0, st, g, root, status);
        else if (shape == 0)
            hipLaunchKernelGGL(comp_link_kernel<16>, dim3(nodes), dim3(256), 0, st, g, root, status);
        hipLaunchKernelGGL(comp_flatten_kernel, dim3(nodes), dim3(256), 0, st, P, root, size, status);
        hipLaunchKernelGGL(comp_spread_kernel, dim3(nodes), dim3(256), 0, st, P, root, size);
        if (comp) {
            const unsigned n_blocks = blocks_of((size_t)P, SCAN_BLOCK);
            int32_t* const sums = static_cast<int32_t*>(scratch);
            hipLaunchKernelGGL(comp_count_kernel, dim3(n_blocks), dim3(256), 0, st, P, root, sums);
            hipLaunchKernelGGL(comp_scan_kernel, dim3(1), dim3(256), 0, st, (int)n_blocks, sums, n_comp);
            hipLaunchKernelGGL(comp_rank_kernel, dim3(n_blocks), dim3(256), 0, st, P, root, sums, n_comp, comp, comp_root);
            hipLaunchKernelGGL(comp_ids_kernel, dim3(nodes), dim3(256), 0, st, P, root, comp);
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // namespace

static_assert(F3DGS_KNN_MAX_NEIGHBORS == 16, "the link templates end at 16");

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_knn_components_scratch_bytes(int P, int num_labels) {
    const size_t blocks = blocks_of((size_t)(P > 0 ? P : 0), SCAN_BLOCK);
    return std::max(blocks * sizeof(int32_t), best_bytes(num_labels)) + 8;   // (never 0: an allocation of its own for every call)
}

int f3dgs_knn_components(int P, int K, const int32_t* idx, const float* dist2, float max_dist2, const int32_t* labels, int mutual,
                         int32_t* root, int32_t* size, int32_t* comp, int32_t* comp_root, int32_t* n_comp, int32_t* status,
                         void* scratch, void* stream) {
    return run_components("f3dgs_knn_components", P, K, idx, dist2, max_dist2, labels, mutual, 1, root, size, comp, comp_root, n_comp,
                          status, scratch, stream);
}

int f3dgs_debug_knn_components_shape(int P, int K, const int32_t* idx, const float* dist2, float max_dist2, const int32_t* labels,
                                     int mutual, int shape, int32_t* root, int32_t* size, int32_t* status, void* stream) {
    const char* who = "f3dgs_debug_knn_components_shape";
    if (shape < 0 || shape > 2) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: shape %d: 0, 1 or 2 expected", who, shape);
    return run_components(who, P, K, idx, dist2, max_dist2, labels, mutual, shape, root, size, nullptr, nullptr, nullptr, status, nullptr,
                          stream);
}

int f3dgs_component_filter(int P, const int32_t* labels, const int32_t* root, const int32_t* size, int min_size, int largest,
                           int num_labels, int32_t* labels_out, void* scratch, void* stream) {
    const char* who = "f3dgs_component_filter";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (P > (1 << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
    if (largest && num_labels < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: num_labels = %d with largest", who, num_labels);
    if (P == 0) return F3DGS_OK;
    if (!root || !size || !labels_out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (labels_out == root || labels_out == size)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: labels_out is root or size: only labels may be filtered in place", who);
    const bool table = largest && num_labels > 0;
    if (table && !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (largest needs scratch)", who);
    if (table && (reinterpret_cast<uintptr_t>(scratch) & 7u))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 8-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* const best = static_cast<unsigned long long*>(scratch);
    const unsigned nodes = blocks_of((size_t)P, 256);
    if (table) {
        hipLaunchKernelGGL(filter_clear_kernel, dim3(blocks_of((size_t)num_labels, 256)), dim3(256), 0, st, num_labels, best);
        hipLaunchKernelGGL(filter_best_kernel, dim3(nodes), dim3(256), 0, st, P, labels, root, size, num_labels, best);
    }
    hipLaunchKernelGGL(filter_apply_kernel, dim3(nodes), dim3(256), 0, st, P, labels, root, size, min_size, largest != 0,
                       table ? num_labels : 0, best, labels_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
