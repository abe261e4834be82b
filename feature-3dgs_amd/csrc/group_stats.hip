// group_stats.hip - statistics of the Gaussians per group id (include/f3dgs.h: f3dgs_group_stats) and the merge of adjacent groups
// whose mean features agree (f3dgs_group_merge): what says something about a class, an instance or a component as a whole.
//
// f3dgs_group_stats is a segmented reduction of P x (C + 10) values under arbitrary, unsorted ids, every sum in fp64.  A million
// fp64 atomics on the C + 10 words of one giant group are the worst shape there is (comp_flatten_kernel, components.hip, says the
// same of its count), so nothing reaches global memory before it has been aggregated.  ONE shape, for every (G, C):
//   group_clear_kernel     the table of sums in `scratch` zeroed, the boxes preset to (max key, min key)
//   group_pass_kernel<0>   a workgroup takes a chunk of ROWS consecutive rows: the member test, (x, y, z, w) of every row into LDS,
//                          one 32-bit key (id << LOG_ROWS | row of the chunk) per member, a bitonic sort of the keys in LDS.  The
//                          sorted members are cut into contiguous segments, one per sub-group of lanes, and a sub-group walks its
//                          segment with a RUN of equal ids in registers: one atomic per run, not per row (and the last runs of a
//                          wave's sub-groups are added by shuffles where they hold the same id).  The moments take 16
//                          lanes a sub-group (lane 0 the mass, 1-3 w x, 4-6 the box minimum, 7-9 its maximum, 10 the count), the
//                          feature rows 16 to 64 lanes ACROSS the channels, so that a row is read in one coalesced piece
//                          (float4 a lane where C, the stride and the pointer allow it), four rows in flight per sub-group
//   group_center_kernel    the fp64 centroids (only with cov)
//   group_pass_kernel<1>   the same chunk, sort and walk over d = x - centroid in fp64: the six sums w d_a d_b (only with cov)
//   group_finish_kernel, group_finish_features_kernel   every output the fp64 quotient rounded once to fp32; the empty values
// A privatised LDS table (G (C + 10) doubles per workgroup) was the alternative for small G: it flushes G (C + 10) atomics per
// workgroup whatever the chunk holds, the runs flush (distinct ids of the chunk) x (C + 10) - never more, and fewer wherever
// the ids are coherent - and need no second code path with its threshold on (G, C).  DESIGN.md 3.22 has the numbers.
// The atomics arrive in a varying order: the float outputs are not bit-reproducible between runs; count and aabb are.
//
// f3dgs_group_merge: merge_init_kernel (the G x G bit matrix cleared, every group its own parent), merge_adjacency_kernel (one
// thread per (node, slot): the bit (min, max) of the two ids, the word read first - nearly every edge repeats a pair already
// there), merge_unite_kernel (one wave per row: the three dot products in fp64 with the lanes across the channels, union_find.h's
// unite), merge_flatten_kernel, merge_gather_kernel.  Integers out.

#include <limits.h>
#include <math.h>

#include "common.h"
#include "group_sums.h"
#include "union_find.h"

namespace f3dgs {

namespace {

constexpr int LOG_ROWS = 11;
constexpr int ROWS = 1 << LOG_ROWS;                  // rows of a workgroup's chunk
constexpr int RPT = ROWS / 256;                      // rows a thread loads
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;             // a row that is no member: behind every member in the sorted chunk
constexpr int MOMENT_LANES = 16;                     // lanes of a sub-group of the moment walk
constexpr int IN_FLIGHT = 4;                         // rows a sub-group of the feature walk loads before it adds them
static_assert(((uint64_t)(F3DGS_GROUP_MAX_GROUPS - 1) << LOG_ROWS | (ROWS - 1)) < NO_KEY, "an id and a row of the chunk share 32 bits");
static_assert(F3DGS_GROUP_MERGE_MAX_GROUPS <= F3DGS_GROUP_MAX_GROUPS, "the merge takes f3dgs_group_stats' ids");

enum : uint32_t { ROLE_MASS = 1u << 0, ROLE_SUM = 7u << 1, ROLE_BOX = 63u << 4, ROLE_COUNT = 1u << 10 };

// the sums of the call, in `scratch`
struct Table {
    double* mass;      // G
    double* sum;       // G x 3   sum w x
    double* center;    // G x 3   sum / mass
    double* cov;       // G x 6   sum w d d^T
    double* feat;      // G x C   sum w f
    uint32_t* count;   // G
    uint32_t* box;     // G x 6   order keys: min xyz, max xyz
};

size_t table_doubles(int G, int C) { return (size_t)G * (size_t)(13 + C); }
size_t table_bytes(int G, int C) { return table_doubles(G, C) * sizeof(double) + (size_t)G * 7 * sizeof(uint32_t); }

Table carve_table(void* scratch, int G, int C) {
    Table t;
    double* d = static_cast<double*>(scratch);
    t.mass = d;
    t.sum = d + (size_t)G;
    t.center = d + (size_t)G * 4;
    t.cov = d + (size_t)G * 7;
    t.feat = d + (size_t)G * 13;
    t.count = reinterpret_cast<uint32_t*>(d + table_doubles(G, C));
    t.box = t.count + G;
    return t;
}

struct Job {
    int P, G, C;
    const int32_t* groups;
    const float* xyz;
    const float* weight;
    const float* features;
    int64_t stride;
    Table t;
    uint32_t roles;        // the lanes of the moment walk whose sums somebody wants
    int lanes_per_row;     // of the feature walk; 0: no feature walk
};

// the order-preserving map of a float's bits onto unsigned integers: -inf < ... < -0 < +0 < ... < +inf
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

__global__ void __launch_bounds__(256) group_clear_kernel(int G, size_t doubles, Table t) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < doubles; i += step) t.mass[i] = 0.0;      // (mass is the table's first word)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)G * 6; i += step) t.box[i] = (i % 6) < 3 ? NO_KEY : 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)G; i += step) t.count[i] = 0u;
}

// ascending bitonic sort of the chunk's keys: 66 steps of ROWS / 2 compare-exchanges
__device__ __forceinline__ void sort_keys(uint32_t* s_key) {
    for (int k = 2; k <= ROWS; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < ROWS / 2; t += 256) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const uint32_t a = s_key[lo], b = s_key[hi];
                if ((a > b) == ((lo & k) == 0)) {
                    s_key[lo] = b;
                    s_key[hi] = a;
                }
            }
        }
    }
    __syncthreads();
}

// the members of the sorted chunk: the first position that holds NO_KEY (a binary search by every thread: no word of LDS for it)
__device__ __forceinline__ int count_members(const uint32_t* s_key) {
    int lo = 0, hi = ROWS;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_key[mid] != NO_KEY) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool is_member(int g, int G, float x, float y, float z, float w) {
    return g >= 0 && g < G && fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY && w > 0.f && w < INFINITY;
}

__device__ __forceinline__ void flush_moments(const Job& job, int g, int role, double acc, uint32_t box, uint32_t cnt) {
    if (g < 0 || !((job.roles >> role) & 1u)) return;
    if (role == 0) atomicAdd(job.t.mass + g, acc);
    else if (role < 4) atomicAdd(job.t.sum + (size_t)g * 3 + (role - 1), acc);
    else if (role < 7) atomicMin(job.t.box + (size_t)g * 6 + (role - 4), box);
    else if (role < 10) atomicMax(job.t.box + (size_t)g * 6 + (role - 4), box);
    else if (role == 10) atomicAdd(job.t.count + g, cnt);
}

// sub-groups of 16 lanes over the sorted members; lane `role` of a sub-group keeps one quantity of the run
__device__ __forceinline__ void walk_moments(const Job& job, int n, const uint32_t* s_key, const float4* s_pt) {
    const int sub = threadIdx.x / MOMENT_LANES, role = threadIdx.x % MOMENT_LANES, subs = 256 / MOMENT_LANES;
    const int begin = n * sub / subs, end = n * (sub + 1) / subs;
    const uint32_t box0 = role < 7 ? NO_KEY : 0u;
    double acc = 0.0;
    uint32_t box = box0, cnt = 0;
    int cur = -1;
    for (int pos = begin; pos < end; pos++) {
        const uint32_t key = s_key[pos];
        const int g = (int)(key >> LOG_ROWS);
        const float4 p = s_pt[key & (ROWS - 1)];
        if (g != cur) {
            flush_moments(job, cur, role, acc, box, cnt);
            cur = g;
            acc = 0.0;
            box = box0;
            cnt = 0;
        }
        const float c = role % 3 == 1 ? p.x : (role % 3 == 2 ? p.y : p.z);      // roles 1, 4, 7: x; 2, 5, 8: y; 3, 6, 9: z
        acc += role == 0 ? (double)p.w : (double)p.w * (double)c;                // (exact products: 24 x 24 bits)
        const uint32_t k = order_key(c);
        box = role < 7 ? min(box, k) : max(box, k);
        cnt++;
    }
    // the last runs of the wave's four sub-groups: where two hold the same id the lower one flushes for both (one giant group:
    // four atomics per word and chunk, not sixteen).  Every lane of the wave is here: the walks above have ended.
#pragma unroll
    for (int d = MOMENT_LANES; d < 64; d <<= 1) {
        const int other = __shfl_xor(cur, d, 64);
        const double other_acc = __shfl_xor(acc, d, 64);
        const uint32_t other_box = __shfl_xor(box, d, 64), other_cnt = __shfl_xor(cnt, d, 64);
        if (cur >= 0 && other == cur) {
            if (threadIdx.x & d) {
                cur = -1;
            } else {
                acc += other_acc;
                box = role < 7 ? min(box, other_box) : max(box, other_box);
                cnt += other_cnt;
            }
        }
    }
    flush_moments(job, cur, role, acc, box, cnt);
}

// the second pass: lanes 0 .. 5 of a sub-group keep xx xy xz yy yz zz
__device__ __forceinline__ void walk_cov(const Job& job, int n, const uint32_t* s_key, const double* s_d, const float* s_w) {
    const int sub = threadIdx.x / MOMENT_LANES, role = threadIdx.x % MOMENT_LANES, subs = 256 / MOMENT_LANES;
    const int begin = n * sub / subs, end = n * (sub + 1) / subs;
    const int a = role < 3 ? 0 : (role < 5 ? 1 : 2), b = role < 3 ? role : (role < 5 ? role - 2 : 2);
    double acc = 0.0;
    int cur = -1;
    for (int pos = begin; pos < end; pos++) {
        const uint32_t key = s_key[pos];
        const int g = (int)(key >> LOG_ROWS), li = (int)(key & (ROWS - 1));
        if (g != cur) {
            if (cur >= 0 && role < 6) atomicAdd(job.t.cov + (size_t)cur * 6 + role, acc);
            cur = g;
            acc = 0.0;
        }
        if (role < 6) acc += ((double)s_w[li] * s_d[li * 3 + a]) * s_d[li * 3 + b];
    }
#pragma unroll
    for (int d = MOMENT_LANES; d < 64; d <<= 1) {                            // (as in walk_moments)
        const int other = __shfl_xor(cur, d, 64);
        const double other_acc = __shfl_xor(acc, d, 64);
        if (cur >= 0 && other == cur) {
            if (threadIdx.x & d) cur = -1;
            else acc += other_acc;
        }
    }
    if (cur >= 0 && role < 6) atomicAdd(job.t.cov + (size_t)cur * 6 + role, acc);
}

// sub-groups of `lanes_per_row` lanes over the sorted members, the lanes across the channels of a block of 4 x lanes_per_row
// channels: VEC: lane l the four channels from 4 l (one 16-byte load), otherwise l, l + lanes, l + 2 lanes, l + 3 lanes
template <bool VEC>
__device__ __forceinline__ void walk_features(const Job& job, size_t base, int n, const uint32_t* s_key, const float4* s_pt) {
    const int lanes = job.lanes_per_row, subs = 256 / lanes;
    const int sub = threadIdx.x / lanes, l = threadIdx.x % lanes;
    const int begin = n * sub / subs, end = n * (sub + 1) / subs;
    const int C = job.C;
    for (int cb = 0; cb < C; cb += 4 * lanes) {
        int ch[4];
#pragma unroll
        for (int q = 0; q < 4; q++) ch[q] = VEC ? cb + 4 * l + q : cb + l + lanes * q;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int cur = -1;
        auto flush = [&]() {
            if (cur < 0) return;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (ch[q] < C) atomicAdd(job.t.feat + (size_t)cur * C + ch[q], acc[q]);
        };
        for (int pos = begin; pos < end; pos += IN_FLIGHT) {
            int g[IN_FLIGHT];
            float w[IN_FLIGHT], f[IN_FLIGHT][4];
#pragma unroll
            for (int u = 0; u < IN_FLIGHT; u++) {
                g[u] = -1;
#pragma unroll
                for (int q = 0; q < 4; q++) f[u][q] = 0.f;
                w[u] = 0.f;
                if (pos + u < end) {
                    const uint32_t key = s_key[pos + u];
                    const int li = (int)(key & (ROWS - 1));
                    g[u] = (int)(key >> LOG_ROWS);
                    w[u] = s_pt[li].w;
                    const float* row = job.features + (base + li) * (size_t)job.stride;      // (a member: base + li < P)
                    if (VEC) {
                        if (ch[0] < C) {                                                     // (C % 4 == 0: all four or none)
                            const float4 v = *reinterpret_cast<const float4*>(row + ch[0]);
                            f[u][0] = v.x, f[u][1] = v.y, f[u][2] = v.z, f[u][3] = v.w;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; q++)
                            if (ch[q] < C) f[u][q] = row[ch[q]];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < IN_FLIGHT; u++) {
                if (g[u] < 0) continue;
                if (g[u] != cur) {
                    flush();
                    cur = g[u];
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[q] = 0.0;
                }
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] += (double)w[u] * (double)f[u][q];    // (exact products)
            }
        }
        for (int d = lanes; d < 64; d <<= 1) {                               // (as in walk_moments; `lanes` is the same for the whole grid)
            const int other = __shfl_xor(cur, d, 64);
            double other_acc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) other_acc[q] = __shfl_xor(acc[q], d, 64);
            if (cur >= 0 && other == cur) {
                if (threadIdx.x & d) {
                    cur = -1;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[q] += other_acc[q];
                }
            }
        }
        flush();
    }
}

// PASS 0: the moments and the feature sums.  PASS 1: the centred second moments.
template <int PASS, bool VEC>
__global__ void __launch_bounds__(256) group_pass_kernel(Job job) {
    __shared__ uint32_t s_key[ROWS];
    __shared__ float4 s_pt[PASS == 0 ? ROWS : 1];
    __shared__ double s_d[PASS == 1 ? ROWS * 3 : 1];
    __shared__ float s_w[PASS == 1 ? ROWS : 1];
    const size_t base = (size_t)blockIdx.x * ROWS;
#pragma unroll
    for (int t = 0; t < RPT; t++) {
        const int li = t * 256 + threadIdx.x;
        const size_t i = base + li;
        uint32_t key = NO_KEY;
        if (i < (size_t)job.P) {
            const int g = job.groups[i];
            const float x = job.xyz ? job.xyz[i * 3] : 0.f, y = job.xyz ? job.xyz[i * 3 + 1] : 0.f, z = job.xyz ? job.xyz[i * 3 + 2] : 0.f;   // (no xyz: group_sums.h)
            const float w = job.weight ? job.weight[i] : 1.f;
            if (is_member(g, job.G, x, y, z, w)) {
                key = ((uint32_t)g << LOG_ROWS) | (uint32_t)li;
                if (PASS == 0) {
                    s_pt[li] = make_float4(x, y, z, w);
                } else {
                    const double* c = job.t.center + (size_t)g * 3;
                    s_d[li * 3] = (double)x - c[0];
                    s_d[li * 3 + 1] = (double)y - c[1];
                    s_d[li * 3 + 2] = (double)z - c[2];
                    s_w[li] = w;
                }
            }
        }
        s_key[li] = key;
    }
    sort_keys(s_key);
    const int n = count_members(s_key);
    if (PASS == 0) {
        if (job.roles) walk_moments(job, n, s_key, s_pt);
        if (job.lanes_per_row) walk_features<VEC>(job, base, n, s_key, s_pt);
    } else {
        walk_cov(job, n, s_key, s_d, s_w);
    }
}

__global__ void __launch_bounds__(256) group_center_kernel(int G, Table t) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const double m = t.mass[g];
    for (int a = 0; a < 3; a++) t.center[(size_t)g * 3 + a] = m > 0.0 ? t.sum[(size_t)g * 3 + a] / m : 0.0;
}

__global__ void __launch_bounds__(256) group_finish_kernel(int G, Table t, int32_t* __restrict__ count, float* __restrict__ mass,
                                                           float* __restrict__ centroid, float* __restrict__ cov, float* __restrict__ aabb) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const double m = t.mass[g];
    if (count) count[g] = (int32_t)t.count[g];
    if (mass) mass[g] = (float)m;
    if (centroid)
        for (int a = 0; a < 3; a++) centroid[(size_t)g * 3 + a] = m > 0.0 ? (float)(t.sum[(size_t)g * 3 + a] / m) : 0.f;
    if (cov)
        for (int a = 0; a < 6; a++) cov[(size_t)g * 6 + a] = m > 0.0 ? (float)(t.cov[(size_t)g * 6 + a] / m) : 0.f;
    if (aabb) {
        const bool empty = t.box[(size_t)g * 6] > t.box[(size_t)g * 6 + 3];      // still (max key, min key): nobody came
        for (int a = 0; a < 6; a++)
            aabb[(size_t)g * 6 + a] = empty ? (a < 3 ? INFINITY : -INFINITY) : key_value(t.box[(size_t)g * 6 + a]);
    }
}

__global__ void __launch_bounds__(256) group_finish_features_kernel(size_t n, int C, Table t, float* __restrict__ feature_mean) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n) return;
    const double m = t.mass[at / C];
    feature_mean[at] = m > 0.0 ? (float)(t.feat[at] / m) : 0.f;
}

unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

int feature_lanes(int C) {
    const int need = (C + 3) / 4;
    int lanes = MOMENT_LANES;                        // (not fewer: every sub-group of a chunk flushes at least once per channel)
    while (lanes < need && lanes < 64) lanes <<= 1;
    return lanes;
}

bool vector_rows(const float* features, int C, int64_t stride) { return C % 4 == 0 && stride % 4 == 0 && aligned16(features); }

void launch_clear_and_pass0(const Job& job, bool vec, hipStream_t st) {
    const size_t doubles = table_doubles(job.G, job.C);
    hipLaunchKernelGGL(group_clear_kernel, dim3(std::min(blocks_of(doubles, 256), 4096u)), dim3(256), 0, st, job.G, doubles, job.t);
    if (job.P > 0) {
        const unsigned chunks = blocks_of((size_t)job.P, ROWS);
        if (vec) hipLaunchKernelGGL((group_pass_kernel<0, true>), dim3(chunks), dim3(256), 0, st, job);
        else hipLaunchKernelGGL((group_pass_kernel<0, false>), dim3(chunks), dim3(256), 0, st, job);
    }
}

// ---- the merge ---------------------------------------------------------------------------------------------------------------

struct MergeGraph {
    int P, K, G, words;                              // words: 32-bit words of a row of the bit matrix
    const int32_t* groups;
    const int32_t* idx;
    const float* dist2;                              // read only when `limited`
    float max_dist2;
    bool limited, mutual;
};

size_t merge_words(int G) { return (size_t)((G + 31) / 32); }
size_t merge_bytes(int G) { return ((size_t)G * merge_words(G) + (size_t)G) * sizeof(uint32_t); }

__global__ void __launch_bounds__(256) merge_init_kernel(int G, size_t words, uint32_t* __restrict__ bits, int32_t* __restrict__ parent,
                                                         int32_t* __restrict__ status) {
    const size_t step = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (first == 0) *status = 0;
    for (size_t i = first; i < words; i += step) bits[i] = 0u;
    for (size_t i = first; i < (size_t)G; i += step) parent[i] = (int32_t)i;
}

// one thread per (node, slot): f3dgs_knn_components' edge rules with "equal labels" turned into "different ids"
__global__ void __launch_bounds__(256) merge_adjacency_kernel(MergeGraph g, uint32_t* __restrict__ bits) {
    const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (size_t)g.P * g.K) return;
    const int i = (int)(at / g.K);
    const int a = g.groups[i];
    if (a < 0 || a >= g.G) return;
    const int j = g.idx[at];
    if (j < 0 || j >= g.P || j == i) return;                                 // idx is the caller's: nothing is read out of bounds
    if (g.limited && !(g.dist2[at] <= g.max_dist2)) return;
    const int b = g.groups[j];
    if (b < 0 || b >= g.G || b == a) return;
    if (g.mutual) {                                                          // row j holds i in a slot that is an edge by its own distance
        bool back = false;
        for (int t = 0; t < g.K; t++) {
            const size_t o = (size_t)j * g.K + t;
            back = back || (g.idx[o] == i && (!g.limited || g.dist2[o] <= g.max_dist2));
        }
        if (!back) return;
    }
    const int lo = min(a, b), hi = max(a, b);
    uint32_t* const word = bits + (size_t)lo * g.words + (hi >> 5);
    const uint32_t bit = 1u << (hi & 31);
    if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
}

// one wave per row a of the matrix: its set bits are the groups b > a adjacent to a
__global__ void __launch_bounds__(256) merge_unite_kernel(int G, int C, int words, const uint32_t* __restrict__ bits,
                                                          const float* __restrict__ fm, float min_cos, int32_t* __restrict__ parent,
                                                          int32_t* __restrict__ status) {
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (a >= G) return;
    const float* const ma = fm + (size_t)a * C;
    for (int w0 = 0; w0 < words; w0 += 64) {
        const uint32_t mine = w0 + lane < words ? bits[(size_t)a * words + w0 + lane] : 0u;
        unsigned long long have = __ballot(mine != 0u);
        while (have) {
            const int src = __ffsll((long long)have) - 1;
            have &= have - 1;
            uint32_t word = __shfl(mine, src);
            while (word) {
                const int b = (w0 + src) * 32 + (__ffs((int)word) - 1);      // < G: only such bits are set
                word &= word - 1;
                const float* const mb = fm + (size_t)b * C;
                double ab = 0.0, aa = 0.0, bb = 0.0;
                for (int c = lane; c < C; c += 64) {
                    const double x = (double)ma[c], y = (double)mb[c];
                    ab += x * y;
                    aa += x * x;
                    bb += y * y;
                }
                ab = wave_sum(ab);
                aa = wave_sum(aa);
                bb = wave_sum(bb);
                if (lane == 0 && aa > 0.0 && bb > 0.0 && ab / sqrt(aa * bb) >= (double)min_cos) unite(parent, a, b, G, status);
            }
        }
    }
}

__global__ void __launch_bounds__(256) merge_flatten_kernel(int G, int32_t* __restrict__ parent, int32_t* __restrict__ group_root,
                                                            int32_t* __restrict__ status) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < G) group_root[g] = find_root(parent, g, G, status);
}

__global__ void __launch_bounds__(256) merge_gather_kernel(int P, int G, const int32_t* groups, const int32_t* __restrict__ group_root,
                                                           int32_t* groups_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int g = groups[i];                                                 // (groups_out may be groups: read before the store)
    groups_out[i] = (g >= 0 && g < G) ? group_root[g] : -1;
}

}  // namespace

// group_sums.h
size_t group_feature_sums_bytes(int G, int C) { return table_bytes(G, C) + 8; }

GroupSums launch_group_feature_sums(int P, int G, int C, const int32_t* groups, const float* weight, const float* features, int64_t stride,
                                    void* scratch, hipStream_t st) {
    Job job{};
    job.P = P, job.G = G, job.C = C;
    job.groups = groups, job.xyz = nullptr, job.weight = weight, job.features = features, job.stride = stride;
    job.t = carve_table(scratch, G, C);
    job.roles = ROLE_MASS | ROLE_COUNT;
    job.lanes_per_row = feature_lanes(C);
    launch_clear_and_pass0(job, vector_rows(features, C, stride), st);
    return GroupSums{job.t.mass, job.t.feat, job.t.count};
}

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_group_stats_scratch_bytes(int G, int C) {
    const int g = std::min(std::max(G, 0), F3DGS_GROUP_MAX_GROUPS), c = std::min(std::max(C, 0), F3DGS_GROUP_MAX_CHANNELS);
    return table_bytes(g, c) + 8;                                            // (never 0: an allocation of its own for every call)
}

int f3dgs_group_stats(int P, int G, int C, const int32_t* groups, const float* xyz, const float* weight, const float* features,
                      int64_t feature_stride, int32_t* count, float* mass, float* centroid, float* cov, float* aabb,
                      float* feature_mean, void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "f3dgs_group_stats";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (G < 1 || G > F3DGS_GROUP_MAX_GROUPS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: G = %d groups, 1 .. %d are taken", who, G, F3DGS_GROUP_MAX_GROUPS);
    if (C < 0 || C > F3DGS_GROUP_MAX_CHANNELS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: C = %d channels, 0 .. %d are taken", who, C, F3DGS_GROUP_MAX_CHANNELS);
    if (C > 0 && !features) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (C = %d needs features)", who, C);
    if (C == 0 && feature_mean) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: feature_mean with C = 0", who);
    if (C > 0 && feature_stride < C)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: feature_stride = %lld below C = %d", who, (long long)feature_stride, C);
    if (P > 0 && (!groups || !xyz)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (groups, xyz)", who);
    if (!count && !mass && !centroid && !cov && !aabb && !feature_mean)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: every output is NULL", who);
    if (!scratch || scratch_bytes < f3dgs_group_stats_scratch_bytes(G, C))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch of %zu bytes, %zu are needed", who, scratch ? scratch_bytes : (size_t)0,
                             f3dgs_group_stats_scratch_bytes(G, C));
    if (reinterpret_cast<uintptr_t>(scratch) & 7u) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 8-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    Job job{};
    job.P = P, job.G = G, job.C = C;
    job.groups = groups, job.xyz = xyz, job.weight = weight, job.features = features, job.stride = feature_stride;
    job.t = carve_table(scratch, G, C);
    job.roles = ((mass || centroid || cov || feature_mean) ? ROLE_MASS : 0u) | ((centroid || cov) ? ROLE_SUM : 0u) | (aabb ? ROLE_BOX : 0u) |
                (count ? ROLE_COUNT : 0u);
    if (feature_mean) job.lanes_per_row = feature_lanes(C);
    const unsigned groups_blocks = blocks_of((size_t)G, 256), chunks = blocks_of((size_t)P, ROWS);
    launch_clear_and_pass0(job, vector_rows(features, C, feature_stride), st);
    if (P > 0) {
        if (cov) {
            hipLaunchKernelGGL(group_center_kernel, dim3(groups_blocks), dim3(256), 0, st, G, job.t);
            hipLaunchKernelGGL((group_pass_kernel<1, false>), dim3(chunks), dim3(256), 0, st, job);
        }
    }
    if (count || mass || centroid || cov || aabb)
        hipLaunchKernelGGL(group_finish_kernel, dim3(groups_blocks), dim3(256), 0, st, G, job.t, count, mass, centroid, cov, aabb);
    if (feature_mean)
        hipLaunchKernelGGL(group_finish_features_kernel, dim3(blocks_of((size_t)G * C, 256)), dim3(256), 0, st, (size_t)G * C, C, job.t,
                           feature_mean);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

size_t f3dgs_group_merge_scratch_bytes(int G) {
    return merge_bytes(std::min(std::max(G, 0), F3DGS_GROUP_MERGE_MAX_GROUPS)) + 8;
}

int f3dgs_group_merge(int P, int K, int G, int C, const int32_t* groups, const int32_t* idx, const float* dist2, float max_dist2,
                      int mutual, const float* feature_mean, float min_cos, int32_t* group_root, int32_t* groups_out, int32_t* status,
                      void* scratch, size_t scratch_bytes, void* stream) {
    const char* who = "f3dgs_group_merge";
    if (P < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: P < 0", who);
    if (K < 1 || K > F3DGS_KNN_MAX_NEIGHBORS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: K = %d neighbours, 1 .. %d are taken", who, K, F3DGS_KNN_MAX_NEIGHBORS);
    if (G < 1 || G > F3DGS_GROUP_MERGE_MAX_GROUPS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: G = %d groups, 1 .. %d are taken", who, G, F3DGS_GROUP_MERGE_MAX_GROUPS);
    if (C < 1 || C > F3DGS_GROUP_MAX_CHANNELS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: C = %d channels, 1 .. %d are taken", who, C, F3DGS_GROUP_MAX_CHANNELS);
    if (P > (1 << 30)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: more than 2^30 points", who);
    if (!(max_dist2 >= 0.f)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: max_dist2 is negative or NaN", who);
    if (min_cos != min_cos) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: min_cos is NaN", who);
    if (!feature_mean || !group_root || !status) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (P > 0 && (!groups || !idx || !groups_out)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (P > 0 && max_dist2 < INFINITY && !dist2) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a finite max_dist2 needs dist2", who);
    if (!scratch || scratch_bytes < f3dgs_group_merge_scratch_bytes(G))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch of %zu bytes, %zu are needed", who, scratch ? scratch_bytes : (size_t)0,
                             f3dgs_group_merge_scratch_bytes(G));
    if (reinterpret_cast<uintptr_t>(scratch) & 3u) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 4-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int words = (int)merge_words(G);
    uint32_t* const bits = static_cast<uint32_t*>(scratch);
    int32_t* const parent = reinterpret_cast<int32_t*>(bits + (size_t)G * words);
    const size_t all = (size_t)G * words;
    hipLaunchKernelGGL(merge_init_kernel, dim3(std::min(blocks_of(std::max(all, (size_t)G), 256), 2048u)), dim3(256), 0, st, G, all, bits, parent,
                       status);
    if (P > 0) {
        MergeGraph g{P, K, G, words, groups, idx, dist2, max_dist2, max_dist2 < INFINITY, mutual != 0};
        hipLaunchKernelGGL(merge_adjacency_kernel, dim3(blocks_of((size_t)P * K, 256)), dim3(256), 0, st, g, bits);
        hipLaunchKernelGGL(merge_unite_kernel, dim3(blocks_of((size_t)G, 4)), dim3(256), 0, st, G, C, words, bits, feature_mean, min_cos, parent,
                           status);
    }
    hipLaunchKernelGGL(merge_flatten_kernel, dim3(blocks_of((size_t)G, 256)), dim3(256), 0, st, G, parent, group_root, status);
    if (P > 0) hipLaunchKernelGGL(merge_gather_kernel, dim3(blocks_of((size_t)P, 256)), dim3(256), 0, st, P, G, groups, group_root, groups_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
