// neighbors.hip - the K nearest neighbours of every point WITH their indices, and a mode filter of per-point labels over them.
//
// knn.hip answers one number per point (the mean of three squared distances) and throws the neighbours away; this unit keeps them.
// The front end is knn.hip's, as it stands (launch_knn_sort: bounds, 30-bit Morton codes, the library's radix sort, the gather
// into float4 {x, y, z, index}, boxes of leaves of 256 sorted points).  What is new:
//
//   knn_list_kernel     one WAVE owns 64 consecutive sorted points.  Every lane keeps its best (distance, index) pairs in
//                       registers, sorted, in a list of LS = 4 / 8 / 16 slots of which K are in use, and inserts through a
//                       compare-exchange chain with static indices.  It seeds the list from its own leaf and then walks the
//                       other leaves: a leaf is visited if ANY lane's K-th best distance reaches its box (wave-uniform ballot:
//                       the leaf's points are read once per wave as broadcasts).
//   mode_filter_kernel  one thread per point: the point and its K neighbours vote with their labels, weighted.
//
// The result of the search is a function of the inputs alone: row i holds the K points j != i with the smallest (dist2, j) in
// lexicographic order.  Two things make that hold.  Every distance is ((dx*dx) + (dy*dy)) + (dz*dz) with dx = candidate - query,
// one fp32 rounding per operation - this unit is built with -ffp-contract=off.  And the leaf test is MONOTONE with the candidate
// distance: the box distance is formed here from the same uncontracted operations - subtraction, squaring and addition are each
// monotone, so the bound of a box never exceeds the computed distance of a point inside it - and a leaf is visited at
// bound <= K-th best (not <), so that a neighbour at exactly the K-th distance with a lower index is never pruned.

#include <float.h>
#include <math.h>

#include "common.h"
#include "leaf_walk.h"

namespace f3dgs {

namespace {

constexpr int LEAF = KNN_LEAF;
constexpr int NO_INDEX = 0x7FFFFFFF;      // an empty slot: behind every real index at the distance +inf
// (finite3 and box_bound: leaf_walk.h, shared with outliers.hip)

// A lane's best (distance, index) pairs in LS slots, ascending in that order.  Every index below is a compile-time constant after
// unrolling: the list lives in registers (a runtime-indexed private array would go to scratch memory).
template <int LS>
struct BestList {
    float d[LS];
    int id[LS];
    // K <= LS pairs are wanted: the first LS - K slots are filled with pairs that sort in front of every real one and never move,
    // so that the K-th best is ALWAYS slot LS - 1 - a static index (picking slot K - 1 at run time would put the list in memory)
    __device__ __forceinline__ void clear(int K) {
#pragma unroll
        for (int s = 0; s < LS; s++) {
            d[s] = s < LS - K ? -INFINITY : INFINITY;
            id[s] = s < LS - K ? -1 : NO_INDEX;
        }
    }
    // does (dist, index) come in front of the last pair?  dist < inf: a distance that overflowed, or a NaN, is nobody's neighbour
    __device__ __forceinline__ bool takes(float dist, int index) const {
        return dist < INFINITY && (dist < d[LS - 1] || (dist == d[LS - 1] && index < id[LS - 1]));
    }
    __device__ __forceinline__ void insert(float dist, int index) {      // takes(dist, index) holds
        d[LS - 1] = dist;
        id[LS - 1] = index;
#pragma unroll
        for (int s = LS - 1; s >= 1; s--) {
            const bool up = d[s] < d[s - 1] || (d[s] == d[s - 1] && id[s] < id[s - 1]);
            const float td = d[s - 1];
            const int ti = id[s - 1];
            d[s - 1] = up ? d[s] : td;
            id[s - 1] = up ? id[s] : ti;
            d[s] = up ? td : d[s];
            id[s] = up ? ti : id[s];
        }
    }
    __device__ __forceinline__ float kth() const { return d[LS - 1]; }
};

// The candidates of one leaf against the wave's 64 queries.  Candidate points are wave-uniform (scalar loads).
template <int LS>
__device__ __forceinline__ void scan_leaf(const float4* __restrict__ sorted, int begin, int end, int self, bool want, float qx, float qy,
                                          float qz, BestList<LS>& best) {
    for (int c = begin; c < end; c++) {
        const float4 p = sorted[c];                       // same address in every lane
        const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
        const float dist = ((dx * dx) + (dy * dy)) + (dz * dz);
        const int index = (int)__float_as_uint(p.w);
        if (want && c != self && best.takes(dist, index)) best.insert(dist, index);
    }
}

template <int LS, bool OUTWARD>
__global__ void __launch_bounds__(64) knn_list_kernel(int P, int K, const float4* __restrict__ sorted, const KnnBox* __restrict__ leaf_box,
                                                      int n_leaf, int* __restrict__ idx, float* __restrict__ dist2) {
    const int lane = threadIdx.x;
    const int j = blockIdx.x * 64 + lane;
    const bool have = j < P;
    const float4 q = sorted[have ? j : P - 1];
    // a point with a non-finite coordinate has no neighbours: it takes no part in any ballot
    const bool ask = have && finite3(q.x, q.y, q.z);
    BestList<LS> best;
    best.clear(K);
    const int home = (blockIdx.x * 64) / LEAF;
    scan_leaf<LS>(sorted, home * LEAF, min(P, (home + 1) * LEAF), j, ask, q.x, q.y, q.z, best);
    float bound = best.kth();
    // One loop body for both orders (the list stays in registers only while everything around it is inlined in one place).
    // OUTWARD: t = 1, 2, 3, 4, ... is home - 1, home + 1, home - 2, home + 2, ...: the Morton neighbours first, they tighten the
    // bound early; the steps that fall off either end of the leaves are skipped.
    const int n_steps = OUTWARD ? 2 * max(home, n_leaf - 1 - home) : n_leaf - 1;
    for (int t = 1; t <= n_steps; t++) {
        const int b = OUTWARD ? ((t & 1) ? home - ((t + 1) >> 1) : home + (t >> 1)) : (t <= home ? t - 1 : t);
        if (b < 0 || b >= n_leaf) continue;
        const KnnBox bx = leaf_box[b];
        const bool want = ask && box_bound(bx, q.x, q.y, q.z) <= bound;
        if (__ballot(want) == 0) continue;
        scan_leaf<LS>(sorted, b * LEAF, min(P, (b + 1) * LEAF), j, want, q.x, q.y, q.z, best);
        bound = best.kth();
    }
    if (!have) return;
    const size_t row = (size_t)__float_as_uint(q.w) * (size_t)K;
#pragma unroll
    for (int s = 0; s < LS; s++) {
        const int o = s - (LS - K);      // the wanted pairs are the last K slots
        if (o >= 0) {
            const bool empty = best.id[s] == NO_INDEX;
            idx[row + o] = empty ? -1 : best.id[s];
            if (dist2) dist2[row + o] = empty ? FLT_MAX : best.d[s];
        }
    }
}

// One Jacobi step of the mode filter: thread i reads the OLD labels of i and of idx[i, 0 .. K-1].  LS + 1 voters in registers.
template <int LS>
__global__ void __launch_bounds__(256) mode_filter_kernel(int P, int K, const int* __restrict__ labels, const float* __restrict__ weight,
                                                          const int* __restrict__ idx, const float* __restrict__ dist2, float max_dist2,
                                                          bool limited, bool fill, int* __restrict__ labels_out,
                                                          float* __restrict__ share_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    constexpr int V = LS + 1;
    int lab[V];
    float w[V];
    const int own = labels[i];
#pragma unroll
    for (int v = 0; v < V; v++) {
        int j = -1;
        if (v == 0) {
            j = i;
        } else if (v - 1 < K) {
            j = idx[(size_t)i * K + (v - 1)];
            if (limited && !(dist2[(size_t)i * K + (v - 1)] <= max_dist2)) j = -1;
        }
        lab[v] = -1;
        w[v] = 0.f;
        if (j >= 0 && j < P) {                      // idx is the caller's: nothing is read out of bounds
            const int l = labels[j];
            const float wj = weight ? weight[j] : 1.f;
            if (l >= 0 && wj > 0.f && wj < INFINITY) { lab[v] = l; w[v] = wj; }
        }
    }
    float total = 0.f, top = 0.f;
    int winner = -1;
#pragma unroll
    for (int a = 0; a < V; a++) {
        if (lab[a] >= 0) total = total + w[a];      // the voters' total, in voter order
        float score = 0.f;
#pragma unroll
        for (int b = 0; b < V; b++) score = (lab[b] >= 0 && lab[b] == lab[a]) ? score + w[b] : score;      // in voter order
        const bool first = winner < 0;
        const bool tie = score == top && (lab[a] == own || (winner != own && lab[a] < winner));
        if (lab[a] >= 0 && (first || score > top || tie)) { top = score; winner = lab[a]; }
    }
    if (!fill && own < 0) winner = -1;
    labels_out[i] = winner;
    if (share_out) share_out[i] = winner >= 0 ? top / total : 0.f;
}

template <bool OUTWARD>
void launch_lists(int P, int K, const float4* sorted, const KnnBox* leaf_box, int n_leaf, int* idx, float* dist2, hipStream_t s) {
    const dim3 grid((P + 63) / 64), block(64);
    if (K <= 4)
        hipLaunchKernelGGL((knn_list_kernel<4, OUTWARD>), grid, block, 0, s, P, K, sorted, leaf_box, n_leaf, idx, dist2);
    else if (K <= 8)
        hipLaunchKernelGGL((knn_list_kernel<8, OUTWARD>), grid, block, 0, s, P, K, sorted, leaf_box, n_leaf, idx, dist2);
    else
        hipLaunchKernelGGL((knn_list_kernel<16, OUTWARD>), grid, block, 0, s, P, K, sorted, leaf_box, n_leaf, idx, dist2);
}

static_assert(F3DGS_KNN_MAX_NEIGHBORS == 16, "the list templates end at 16");

hipError_t launch_knn_neighbors(int P, int K, const float* points, int* idx, float* dist2, char* scratch, bool outward, hipStream_t s) {
    float4* sorted;
    KnnBox* leaf_box;
    int n_leaf;
    launch_knn_sort(P, points, scratch, &sorted, &leaf_box, &n_leaf, s);
    if (outward)
        launch_lists<true>(P, K, sorted, leaf_box, n_leaf, idx, dist2, s);
    else
        launch_lists<false>(P, K, sorted, leaf_box, n_leaf, idx, dist2, s);
    return hipGetLastError();
}

hipError_t launch_label_mode_filter(int P, int K, const int* labels, const float* weight, const int* idx, const float* dist2,
                                    float max_dist2, bool fill, int* labels_out, float* share_out, hipStream_t s) {
    const dim3 grid((P + 255) / 256), block(256);
    const bool limited = max_dist2 < INFINITY;
    if (K <= 4)
        hipLaunchKernelGGL((mode_filter_kernel<4>), grid, block, 0, s, P, K, labels, weight, idx, dist2, max_dist2, limited, fill, labels_out,
                           share_out);
    else if (K <= 8)
        hipLaunchKernelGGL((mode_filter_kernel<8>), grid, block, 0, s, P, K, labels, weight, idx, dist2, max_dist2, limited, fill, labels_out,
                           share_out);
    else
        hipLaunchKernelGGL((mode_filter_kernel<16>), grid, block, 0, s, P, K, labels, weight, idx, dist2, max_dist2, limited, fill,
                           labels_out, share_out);
    return hipGetLastError();
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_knn_neighbors_scratch_bytes(int P, int K) {
    (void)K;      // the lists live in registers: the scratch is the front end's (sort buffers, sorted points, leaf boxes)
    return knn_scratch_bytes((size_t)(P > 0 ? P : 0));
}

int f3dgs_knn_neighbors(int P, int K, const float* points, int32_t* idx, float* dist2, void* scratch, void* stream) {
    const char* who = "f3dgs_knn_neighbors";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (K < 1 || K > F3DGS_KNN_MAX_NEIGHBORS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: K = %d neighbours, 1 .. %d are taken", who, K, F3DGS_KNN_MAX_NEIGHBORS);
    if (P == 0) return F3DGS_OK;
    if (P > (1 << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
    if (!points || !idx || !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (!aligned16(scratch)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
    HIP_TRY(launch_knn_neighbors(P, K, points, idx, dist2, static_cast<char*>(scratch), options().knn_outward != 0,
                                 static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_label_mode_filter(int P, int K, const int32_t* labels, const float* weight, const int32_t* idx, const float* dist2,
                            float max_dist2, int fill, int32_t* labels_out, float* share_out, void* stream) {
    const char* who = "f3dgs_label_mode_filter";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (K < 1 || K > F3DGS_KNN_MAX_NEIGHBORS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: K = %d neighbours, 1 .. %d are taken", who, K, F3DGS_KNN_MAX_NEIGHBORS);
    if (!(max_dist2 >= 0.f)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: max_dist2 is negative or NaN", who);
    if (P == 0) return F3DGS_OK;
    if (!labels || !idx || !labels_out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (labels_out == labels) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: labels_out is labels: a Jacobi step cannot run in place", who);
    if (max_dist2 < INFINITY && !dist2) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a finite max_dist2 needs dist2", who);
    HIP_TRY(launch_label_mode_filter(P, K, labels, weight, idx, dist2, max_dist2, fill != 0, labels_out, share_out,
                                     static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

}  // extern "C"
