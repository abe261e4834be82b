// outliers.hip - the two density tests of a point cloud (include/f3dgs.h: f3dgs_radius_count, f3dgs_knn_outliers): how many points
// lie within a radius of every point, and which points' mean neighbour distance stands out of their group's.
//
// The front end of the count is knn.hip's, as it stands (launch_knn_sort: Morton order, float4 {x, y, z, index}, boxes of leaves of
// 256 sorted points).  What is new:
//
//   radius_gather_labels_kernel  the labels into sorted order, once: the walk then reads a candidate's label at the same uniform
//                                address as its position
//   radius_count_kernel          one WAVE owns 64 consecutive sorted points, as in knn_list_kernel.  A lane wants a leaf iff it asks,
//                                its count is below the cap and the leaf's box_bound is <= radius2; the wave skips a leaf on an empty
//                                ballot, and the leaf's points are read once per wave as broadcasts.  The bound never tightens, so
//                                the walk order decides nothing: the leaves are walked in storage order.  No LDS, a handful of
//                                registers.  The wave leaves the walk once every lane has reached the cap
//   outlier_clear_kernel         the per-group sums to zero
//   outlier_score_kernel         one thread per point: the fp64 mean of the square roots of its valid slots, rounded once; then the
//                                first sums (n, sum of scores) per group
//   outlier_spread_kernel        the second sums: (score - mean)^2 about the device's own fp64 mean
//   outlier_apply_kernel         every thread forms its group's {n, mean, std, threshold} from the sums (the same operations on the
//                                same words: the same bits in every thread), thread g < G stores row g of `stats`, thread i decides
//                                keep[i].  No workgroup waits for another
// The group sums meet in fp64 atomics, ONE per distinct group per wave (comp_flatten_kernel's ballot loop over the distinct values
// among the 64 lanes): without labels the cloud is one group, and a million adds on one word are what the loop avoids.
//
// The count is an integer function of the inputs alone: every distance is ((dx*dx) + (dy*dy)) + (dz*dz) with dx = candidate - query,
// one fp32 rounding per operation, and the leaf test is monotone with it (leaf_walk.h) - this unit is built with -ffp-contract=off.
// The scores are a function of the inputs alone as well; the group sums arrive in a varying order, so mean, std and threshold are
// reproducible to the error of an fp64 sum only.

#include <limits.h>
#include <math.h>

#include "common.h"
#include "leaf_walk.h"

namespace f3dgs {

namespace {

constexpr int LEAF = KNN_LEAF;

// finite3 on a candidate's bits: a candidate is wave-uniform, and integer tests of uniform words stay on the scalar unit
__device__ __forceinline__ bool finite_bits(float x, float y, float z) {
    const uint32_t e = 0x7F800000u;
    return (__float_as_uint(x) & e) != e && (__float_as_uint(y) & e) != e && (__float_as_uint(z) & e) != e;
}

__global__ void __launch_bounds__(256) radius_gather_labels_kernel(int P, const float4* __restrict__ sorted, const int32_t* __restrict__ labels,
                                                                   int32_t* __restrict__ sorted_labels) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < P) sorted_labels[j] = labels[__float_as_uint(sorted[j].w)];
}

template <bool LABELLED>
__global__ void __launch_bounds__(64) radius_count_kernel(int P, const float4* __restrict__ sorted, const KnnBox* __restrict__ leaf_box,
                                                          int n_leaf, const int32_t* __restrict__ sorted_labels, float radius2, int limit,
                                                          int32_t* __restrict__ count) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    const bool have = j < P;
    const float4 q = sorted[have ? j : P - 1];
    const int own = LABELLED ? sorted_labels[have ? j : P - 1] : 0;
    // a point with a non-finite coordinate or a negative label counts nobody: it takes no part in any ballot
    const bool ask = have && finite3(q.x, q.y, q.z) && own >= 0;
    int n = 0;
    for (int b = 0; b < n_leaf; b++) {
        const KnnBox bx = leaf_box[b];
        const bool want = ask && n < limit && box_bound(bx, q.x, q.y, q.z) <= radius2;
        if (__ballot(want) == 0) continue;
        const int end = min(P, (b + 1) * LEAF);
        for (int c = b * LEAF; c < end; c++) {
            const float4 p = sorted[c];                       // same address in every lane
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float dist = ((dx * dx) + (dy * dy)) + (dz * dz);
            // (a NaN distance fails the comparison; with radius2 = +inf an infinite candidate would pass it: finite_bits)
            bool hit = want && c != j && dist <= radius2 && finite_bits(p.x, p.y, p.z);
            if (LABELLED) hit = hit && sorted_labels[c] == own;
            n += hit ? 1 : 0;
        }
        if (__ballot(ask && n < limit) == 0) break;           // every lane has reached the cap
    }
    if (have) count[__float_as_uint(q.w)] = min(n, limit);
}

// ---- the scores over the neighbour lists -----------------------------------------------------------------------------------

struct GroupSums {
    double* sum;      // G   sum of the finite scores
    double* sq;       // G   sum of (score - mean)^2
    int32_t* n;       // G   members with a finite score
};

__host__ __device__ inline GroupSums carve_sums(void* scratch, int G) {
    GroupSums t;
    t.sum = static_cast<double*>(scratch);
    t.sq = t.sum + G;
    t.n = reinterpret_cast<int32_t*>(t.sq + G);
    return t;
}

// v of the lanes with `active`, summed per distinct g among them and added to word[g] (and the lanes counted into n[g], where
// given) by one lane per distinct g.  Every lane of the wave calls this.  At most 64 rounds, one without labels.
__device__ __forceinline__ void add_per_group(bool active, int g, double v, double* __restrict__ word, int32_t* __restrict__ n) {
    const int lane = threadIdx.x & 63;
    bool pending = active;
    for (int round = 0; round < 64; round++) {
        const unsigned long long left = __ballot(pending);
        if (!left) break;
        const int leader = __ffsll((long long)left) - 1;
        const int lg = __shfl(g, leader);
        const bool same = pending && g == lg;
        const unsigned long long members = __ballot(same);
        const double total = wave_sum(same ? v : 0.0);
        if (lane == leader) {
            atomicAdd(word + lg, total);
            if (n) atomicAdd(n + lg, __popcll(members));
        }
        pending = pending && !same;
    }
}

__global__ void __launch_bounds__(256) outlier_clear_kernel(int G, GroupSums t) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < G) { t.sum[g] = 0.0; t.sq[g] = 0.0; t.n[g] = 0; }
}

__global__ void __launch_bounds__(256) outlier_score_kernel(int P, int K, const int32_t* __restrict__ idx, const float* __restrict__ dist2,
                                                            const int32_t* __restrict__ labels, int G, float* __restrict__ score,
                                                            GroupSums t) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int g = -1;
    float sc = INFINITY;
    if (i < P) {
        g = labels ? labels[i] : 0;
        if (g < 0 || g >= G) g = -1;
        if (g >= 0) {
            double sum = 0.0;
            int valid = 0;
            for (int s = 0; s < K; s++) {
                const size_t at = (size_t)i * K + s;
                const int j = idx[at];
                if (j < 0 || j >= P || j == i) continue;                     // idx is the caller's: nothing is read out of bounds
                if (labels && labels[j] != g) continue;
                const float d = dist2[at];
                if (!(d < INFINITY)) continue;                               // (a NaN is not valid)
                sum = sum + sqrt((double)d);
                valid++;
            }
            if (valid > 0) sc = (float)(sum / (double)valid);
        }
        score[i] = sc;
    }
    add_per_group(g >= 0 && sc < INFINITY, g, (double)sc, t.sum, t.n);
}

__global__ void __launch_bounds__(256) outlier_spread_kernel(int P, const int32_t* __restrict__ labels, int G, const float* __restrict__ score,
                                                             GroupSums t) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int g = -1;
    double dev2 = 0.0;
    bool counted = false;
    if (i < P) {
        g = labels ? labels[i] : 0;
        const float sc = score[i];
        counted = g >= 0 && g < G && sc < INFINITY;
        if (counted) {
            const double mean = t.sum[g] / (double)t.n[g];                   // (n >= 1: this point is one of them)
            const double d = (double)sc - mean;
            dev2 = d * d;
        }
    }
    add_per_group(counted, g, dev2, t.sq, nullptr);
}

struct GroupLine {
    double n, mean, std, threshold;
};

__device__ __forceinline__ GroupLine group_line(const GroupSums& t, int g, float ratio) {
    GroupLine l = {0.0, 0.0, 0.0, 0.0};
    const int n = t.n[g];
    if (n < 1) return l;
    l.n = (double)n;
    l.mean = t.sum[g] / l.n;
    l.std = n < 2 ? 0.0 : sqrt(t.sq[g] / (double)(n - 1));
    l.threshold = l.mean + (double)ratio * l.std;
    return l;
}

__global__ void __launch_bounds__(256) outlier_apply_kernel(int P, const int32_t* __restrict__ labels, int G, float ratio,
                                                            const float* __restrict__ score, GroupSums t, double* __restrict__ stats,
                                                            uint8_t* __restrict__ keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < G) {
        const GroupLine l = group_line(t, i, ratio);
        stats[4 * (size_t)i + 0] = l.n;
        stats[4 * (size_t)i + 1] = l.mean;
        stats[4 * (size_t)i + 2] = l.std;
        stats[4 * (size_t)i + 3] = l.threshold;
    }
    if (i >= P) return;
    const int g = labels ? labels[i] : 0;
    const float sc = score[i];
    bool k = false;
    if (g >= 0 && g < G && sc < INFINITY) k = (double)sc <= group_line(t, g, ratio).threshold;
    keep[i] = k ? 1 : 0;
}

unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

size_t labels_offset(size_t P) { return knn_scratch_bytes(P); }       // (a multiple of the carving alignment)

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_radius_count_scratch_bytes(int P) {
    const size_t n = (size_t)(P > 0 ? P : 0);
    return labels_offset(n) + ((n * sizeof(int32_t) + ALIGN - 1) & ~(ALIGN - 1));      // the front end's, and P labels in sorted order
}

int f3dgs_radius_count(int P, const float* points, float radius2, const int32_t* labels, int cap, int32_t* count, void* scratch,
                       void* stream) {
    const char* who = "f3dgs_radius_count";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (!(radius2 >= 0.f)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: radius2 is negative or NaN", who);
    if (cap < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: cap = %d: 0 (no cap) or a positive count expected", who, cap);
    if (P == 0) return F3DGS_OK;
    if (P > (1 << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
    if (!points || !count || !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (!aligned16(scratch)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    float4* sorted;
    KnnBox* leaf_box;
    int n_leaf;
    launch_knn_sort(P, points, static_cast<char*>(scratch), &sorted, &leaf_box, &n_leaf, st);
    const int limit = cap > 0 ? cap : INT_MAX;      // (a count stays below 2^30)
    const dim3 grid((P + 63) / 64), block(64);
    if (labels) {
        int32_t* const sorted_labels = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + labels_offset((size_t)P));
        hipLaunchKernelGGL(radius_gather_labels_kernel, dim3(blocks_of((size_t)P, 256)), dim3(256), 0, st, P, sorted, labels, sorted_labels);
        hipLaunchKernelGGL(radius_count_kernel<true>, grid, block, 0, st, P, sorted, leaf_box, n_leaf, sorted_labels, radius2, limit, count);
    } else {
        hipLaunchKernelGGL(radius_count_kernel<false>, grid, block, 0, st, P, sorted, leaf_box, n_leaf, nullptr, radius2, limit, count);
    }
    HIP_TRY(hipGetLastError());
    return F3DGS_OK;
}

size_t f3dgs_knn_outliers_scratch_bytes(int num_groups) {
    const size_t G = (size_t)(num_groups > 0 ? num_groups : 0);
    return G * (2 * sizeof(double) + sizeof(int32_t)) + 8;      // (never 0: an allocation of its own for every call)
}

int f3dgs_knn_outliers(int P, int K, const int32_t* idx, const float* dist2, const int32_t* labels, int num_groups, float ratio,
                       float* score, double* stats, uint8_t* keep, void* scratch, void* stream) {
    const char* who = "f3dgs_knn_outliers";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (K < 1 || K > F3DGS_KNN_MAX_NEIGHBORS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: K = %d neighbours, 1 .. %d are taken", who, K, F3DGS_KNN_MAX_NEIGHBORS);
    if (num_groups < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: num_groups = %d: at least one group expected", who, num_groups);
    if (!labels && num_groups != 1)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: num_groups = %d without labels: every point is in group 0", who, num_groups);
    if (!(ratio >= 0.f && ratio < INFINITY)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: ratio is negative or not finite", who);
    if (P > (1 << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
    if (!stats || !scratch) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (P > 0 && (!idx || !dist2 || !score || !keep)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (reinterpret_cast<uintptr_t>(scratch) & 7u) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 8-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const GroupSums t = carve_sums(scratch, num_groups);
    const unsigned nodes = blocks_of((size_t)P, 256);
    hipLaunchKernelGGL(outlier_clear_kernel, dim3(blocks_of((size_t)num_groups, 256)), dim3(256), 0, st, num_groups, t);
    if (P > 0) {
        hipLaunchKernelGGL(outlier_score_kernel, dim3(nodes), dim3(256), 0, st, P, K, idx, dist2, labels, num_groups, score, t);
        hipLaunchKernelGGL(outlier_spread_kernel, dim3(nodes), dim3(256), 0, st, P, labels, num_groups, score, t);
    }
    hipLaunchKernelGGL(outlier_apply_kernel, dim3(blocks_of(std::max((size_t)P, (size_t)num_groups), 256)), dim3(256), 0, st, P, labels,
                       num_groups, ratio, score, t, stats, keep);
    HIP_TRY(hipGetLastError());
    return F3DGS_OK;
}

}  // extern "C"
