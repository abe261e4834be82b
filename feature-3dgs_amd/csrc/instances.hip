// instances.hip - association of one view's SAM instances with the 3D instances built so far (f3dgs_instance_associate,
// f3dgs_instance_merge).  No counterpart in the reference, which never lifts SAM masks to the Gaussians.
//
// SAM numbers its masks afresh in every view.  The label vote (contrib.hip: label_votes_kernel) gives, per Gaussian, the blend
// weight that fell under each of the view's M masks: acc_view (P, M + 1), column M the weight total.  The global accumulator
// acc (P, L + 1) holds the same sums per 3D instance.  Everything here runs over those two dense matrices - no tile list is
// touched:
//   inst_fill_kernel      T = 0 (and, for P == 0, the outputs of an empty match): a launch, not a memset node
//   inst_overlap_kernel   a wave takes 64 consecutive Gaussians per grid-stride step: their totals first, one per lane in one round
//                         trip - an unseen row (total not > 0) costs that one read -, then the seen rows one after the other,
//                         the wave on each.  c = the lowest index of the largest of acc[g][0..L) (wave maximum, then the lowest
//                         index among the lanes that hold it), L where that maximum is not > 0, and one float atomic T[m][c] += acc_view[g][m] per
//                         NON-ZERO of the view's row; row M receives max(0, total - sum_m acc_view[g][m]), the sum formed in
//                         fp32 in ascending m (adding a zero changes nothing, so only the non-zeros are walked, in order) -
//                         through 16 copies of that row in scratch, a wave into one of them
//   inst_sums_kernel      T[M] = the sum of its copies; row[m] (columns < L), rowall[m] (all columns), col[l] (rows <= M) of T
//                         in double, a fixed order
//   inst_best_kernel      one wave per mask: iou[m][l] = T / ((row + col) - T) in double over l < count, the largest, the lowest
//                         l among equals
//   inst_winner_kernel    one thread per instance: its claimant (best_iou >= iou_thresh) of largest IoU, the lowest m among equals
//   inst_assign_kernel    ONE workgroup: accepted claims, a prefix over the remaining masks of rowall > min_weight for the new
//                         ids count, count + 1, ... < L, the write of mapping, count and dropped
//   inst_merge_kernel     the same walk over the seen rows: acc[g][mapping[m]] += acc_view[g][m], acc[g][L] += total, the non-zeros
//                         it read written back as zeros with clear_view.  Every workgroup first marks mapping's targets in LDS:
//                         an injective mapping takes one plain fp32 add per element (the bits of a single add), a mapping that
//                         repeats a target float atomics within the row
// Launches follow each other on the stream; no workgroup waits for another, no host read, every loop is bounded by M, L or a
// grid stride.  Compiled without FMA contraction: the quotient decides labels.

#include "common.h"

namespace f3dgs {

namespace {

constexpr int INST_BLOCK = 256;                  // 4 waves: 256 Gaussians (or 4 masks) per workgroup and step
constexpr int INST_MAX_M = 1024, INST_MAX_L = 4096;
// Copies of the table's last row (the weight under no mask) the overlap kernel adds into, a wave into copy (its number % 16): every
// seen Gaussian adds there, and as one row of L + 1 floats they met on its few 64-byte lines (measured: DESIGN 3.19).  The
// copies are summed in a fixed order into T[M] by inst_sums_kernel.
constexpr int INST_REST_COPIES = 16;

struct InstScratch {
    double* row;       // [M]  sum over l < L of T[m][l]
    double* rowall;    // [M]  ... over l <= L
    double* col;       // [L]  sum over m <= M of T[m][l]
    int* winner;       // [L]  the accepted claimant of instance l, or -1
    float* rest;       // [INST_REST_COPIES][L + 1]  partial sums of T[M]
    static InstScratch carve(char* base, int M, int L, size_t* bytes) {
        Carver c(base);
        InstScratch s;
        s.row = c.take<double>(M);
        s.rowall = c.take<double>(M);
        s.col = c.take<double>(L);
        s.winner = c.take<int>(L);
        s.rest = c.take<float>((size_t)INST_REST_COPIES * (L + 1));
        if (bytes) *bytes = c.total();
        return s;
    }
};

// T = 0; with `outputs` (P == 0) also what a match over an empty table gives: every mask unmatched
__global__ void __launch_bounds__(INST_BLOCK) inst_fill_kernel(size_t n, float* __restrict__ T, size_t n_rest, float* __restrict__ rest, int M,
                                                               int outputs, int* __restrict__ mapping, int* __restrict__ best_label,
                                                               double* __restrict__ best_iou) {
    const size_t stride = (size_t)gridDim.x * INST_BLOCK;
    for (size_t i = (size_t)blockIdx.x * INST_BLOCK + threadIdx.x; i < n; i += stride) T[i] = 0.f;
    for (size_t i = (size_t)blockIdx.x * INST_BLOCK + threadIdx.x; i < n_rest; i += stride) rest[i] = 0.f;      // (n_rest = 0: no scratch)
    if (outputs && blockIdx.x == 0)
        for (int m = threadIdx.x; m < M; m += INST_BLOCK) {
            mapping[m] = -1;
            best_label[m] = -1;
            best_iou[m] = 0.0;
        }
}

// The totals of 64 consecutive rows, one per lane, in one round trip; returns the ballot of the rows seen in the view (total > 0)
__device__ __forceinline__ unsigned long long inst_seen_rows(const float* __restrict__ acc_view, int P, int M, long long base, int lane, float& tot) {
    const long long g = base + lane;
    tot = g < P ? acc_view[(size_t)g * (M + 1) + M] : 0.f;
    return __ballot(tot > 0.f);
}

__global__ void __launch_bounds__(INST_BLOCK) inst_overlap_kernel(int P, int M, int L, const float* __restrict__ acc_view,
                                                                  const float* __restrict__ acc, float* __restrict__ T,
                                                                  float* __restrict__ rest_copies) {
    const int lane = threadIdx.x & 63;
    const long long step = (long long)gridDim.x * INST_BLOCK;          // rows per grid step: 64 per wave
    float* const rest_row = rest_copies + (size_t)((blockIdx.x * (INST_BLOCK / 64) + (threadIdx.x >> 6)) % INST_REST_COPIES) * (L + 1);
    for (long long base = (long long)blockIdx.x * INST_BLOCK + (threadIdx.x & ~63); base < P; base += step) {      // wave-uniform
        float tot_l;
        unsigned long long rows = inst_seen_rows(acc_view, P, M, base, lane, tot_l);      // an unseen row costs this one read
        while (rows) {                                                 // wave-uniform: at most 64 steps
            const int r = __ffsll((long long)rows) - 1;
            rows &= rows - 1;
            const int g = (int)base + r;
            const float tot = __shfl(tot_l, r, 64);
            const float* vrow = acc_view + (size_t)g * (M + 1);
            const float v0 = lane < M ? vrow[lane] : 0.f;              // the view's first 64 masks: in flight beside the 3D row
            // the 3D label: the lowest index of the largest of acc[g][0..L)
            const float* arow = acc + (size_t)g * (L + 1);
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int l = lane; l < L; l += 64) {
                const float v = arow[l];
                if (v > bv) { bv = v; bi = l; }                        // ascending l: the lowest index of a lane's largest
            }
            float mx = bv;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
            int c = L;
            if (mx > 0.f) {                                            // some lane holds the maximum: the lowest of their indices
                int cand = bv == mx ? bi : 0x7fffffff;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) cand = min(cand, __shfl_xor(cand, d, 64));
                c = cand;
            }
            // the view's row: one atomic per non-zero; their fp32 sum in ascending m
            float s = 0.f;
            for (int m0 = 0; m0 < M; m0 += 64) {
                const int m = m0 + lane;
                const float v = m0 == 0 ? v0 : (m < M ? vrow[m] : 0.f);
                const bool nz = v != 0.f;
                if (nz) atomicAdd(T + (size_t)m * (L + 1) + c, v);
                unsigned long long bits = __ballot(nz);
                while (bits) {                                         // wave-uniform: at most 64 steps
                    const int b = __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    s += __shfl(v, b, 64);
                }
            }
            const float rest = fmaxf(0.f, tot - s);
            if (lane == 0 && rest > 0.f) atomicAdd(rest_row + c, rest);
        }
    }
}

// workgroups [0, row_blocks): one wave per mask row; the others: one thread per column l <= L, which first sums the copies of the
// last row into T[M][l] (no row wave reads that row)
__global__ void __launch_bounds__(INST_BLOCK) inst_sums_kernel(int M, int L, int row_blocks, float* __restrict__ T, InstScratch sc) {
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x < row_blocks) {
        const int m = blockIdx.x * (INST_BLOCK / 64) + (threadIdx.x >> 6);
        if (m >= M) return;
        const float* t = T + (size_t)m * (L + 1);
        double s = 0.0;
        for (int l = lane; l < L; l += 64) s += (double)t[l];
        s = wave_sum(s);
        if (lane == 0) {
            sc.row[m] = s;
            sc.rowall[m] = s + (double)t[L];
        }
    } else {
        const int l = ((int)blockIdx.x - row_blocks) * INST_BLOCK + threadIdx.x;
        if (l > L) return;
        float under_none = 0.f;
        for (int k = 0; k < INST_REST_COPIES; k++) under_none += sc.rest[(size_t)k * (L + 1) + l];
        T[(size_t)M * (L + 1) + l] = under_none;
        if (l == L) return;
        double s = 0.0;
        for (int m = 0; m < M; m++) s += (double)T[(size_t)m * (L + 1) + l];
        sc.col[l] = s + (double)under_none;
    }
}

__global__ void __launch_bounds__(INST_BLOCK) inst_best_kernel(int M, int L, const float* __restrict__ T, InstScratch sc,
                                                               const int* __restrict__ count, int* __restrict__ best_label,
                                                               double* __restrict__ best_iou) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * (INST_BLOCK / 64) + (threadIdx.x >> 6);
    if (m >= M) return;
    const int n = min(max(*count, 0), L);
    const float* t = T + (size_t)m * (L + 1);
    const double r = sc.row[m];
    double bv = 0.0;
    int bi = 0x7fffffff;
    for (int l = lane; l < n; l += 64) {
        const double x = (double)t[l];
        const double den = (r + sc.col[l]) - x;
        const double q = den == 0.0 ? 0.0 : x / den;
        if (q > bv) { bv = q; bi = l; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(bv, d, 64);
        const int oi = __shfl_xor(bi, d, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        const bool any = bv > 0.0;
        best_label[m] = any ? bi : -1;
        best_iou[m] = any ? bv : 0.0;
    }
}

__global__ void __launch_bounds__(INST_BLOCK) inst_winner_kernel(int M, int L, double iou_thresh, const int* __restrict__ best_label,
                                                                 const double* __restrict__ best_iou, InstScratch sc) {
    const int l = blockIdx.x * INST_BLOCK + threadIdx.x;
    if (l >= L) return;
    double bv = -1.0;
    int bm = -1;
    for (int m = 0; m < M; m++) {
        const double q = best_iou[m];
        if (best_label[m] == l && q >= iou_thresh && q > bv) { bv = q; bm = m; }      // ascending m: the lowest among equals
    }
    sc.winner[l] = bm;
}

// one workgroup of INST_MAX_M threads, a mask each
__global__ void __launch_bounds__(INST_MAX_M) inst_assign_kernel(int M, int L, double iou_thresh, double min_weight,
                                                                 const int* __restrict__ best_label, const double* __restrict__ best_iou,
                                                                 InstScratch sc, int* __restrict__ count, int* __restrict__ dropped,
                                                                 int* __restrict__ mapping) {
    __shared__ int wave_total[INST_MAX_M / 64];
    const int m = threadIdx.x, lane = m & 63, w = m >> 6;
    const int n = min(max(*count, 0), L);
    int target = -1;
    bool fresh = false;
    if (m < M) {
        const int bl = best_label[m];
        if (bl >= 0 && best_iou[m] >= iou_thresh && sc.winner[bl] == m) target = bl;
        else fresh = sc.rowall[m] > min_weight;
    }
    // exclusive prefix of `fresh` in ascending m: within the wave by the ballot, across the waves through LDS
    const unsigned long long bits = __ballot(fresh);
    const int before = __popcll(bits & ((1ull << lane) - 1ull));
    if (lane == 0) wave_total[w] = __popcll(bits);
    __syncthreads();
    int base = 0, total = 0;
    for (int i = 0; i < INST_MAX_M / 64; i++) {
        const int t = wave_total[i];
        if (i < w) base += t;
        total += t;
    }
    if (fresh) {
        const int id = n + base + before;
        target = id < L ? id : -1;
    }
    if (m < M) mapping[m] = target;
    if (m == 0) {
        const int room = L - n;
        *count = n + min(total, room);
        if (total > room) *dropped += total - room;
    }
}

__global__ void __launch_bounds__(INST_BLOCK) inst_merge_kernel(int P, int M, int L, float* __restrict__ acc_view, int clear_view,
                                                                const int* __restrict__ mapping, float* __restrict__ acc) {
    __shared__ unsigned int taken[INST_MAX_L / 32];
    __shared__ int repeats;
    for (int i = threadIdx.x; i < INST_MAX_L / 32; i += INST_BLOCK) taken[i] = 0u;
    if (threadIdx.x == 0) repeats = 0;
    __syncthreads();
    for (int m = threadIdx.x; m < M; m += INST_BLOCK) {
        const int t = mapping[m];
        if (t >= 0 && t < L && (atomicOr(&taken[t >> 5], 1u << (t & 31)) >> (t & 31) & 1u)) repeats = 1;
    }
    __syncthreads();
    const bool atomics = repeats != 0;
    const int lane = threadIdx.x & 63;
    const long long step = (long long)gridDim.x * INST_BLOCK;
    for (long long base = (long long)blockIdx.x * INST_BLOCK + (threadIdx.x & ~63); base < P; base += step) {      // wave-uniform
        float tot_l;
        unsigned long long rows = inst_seen_rows(acc_view, P, M, base, lane, tot_l);
        while (rows) {
            const int r = __ffsll((long long)rows) - 1;
            rows &= rows - 1;
            const int g = (int)base + r;
            const float tot = __shfl(tot_l, r, 64);
            float* vrow = acc_view + (size_t)g * (M + 1);
            float* arow = acc + (size_t)g * (L + 1);
            for (int m = lane; m < M; m += 64) {
                const float v = vrow[m];
                if (v == 0.f) continue;
                const int t = mapping[m];
                if (t >= 0 && t < L) {
                    if (atomics) atomicAdd(arow + t, v);
                    else arow[t] += v;
                }
                if (clear_view) vrow[m] = 0.f;
            }
            if (lane == 0) {
                arow[L] += tot;
                if (clear_view) vrow[M] = 0.f;
            }
        }
    }
}

int inst_grid(int P) {
    const long long blocks = ((long long)P + INST_BLOCK - 1) / INST_BLOCK;          // a wave takes 64 consecutive rows per step
    return (int)std::min<long long>(std::max<long long>(blocks, 1), 256 * 8);      // 8 workgroups = 32 waves per CU
}

size_t instance_scratch_bytes(int M, int L) {
    size_t b = 0;
    InstScratch::carve(nullptr, M, L, &b);
    return b;
}

hipError_t launch_instance_associate(int P, int M, int L, const float* acc_view, const float* acc, double iou_thresh, double min_weight,
                                     int* count, int* dropped, int* mapping, int* best_label, double* best_iou, float* table,
                                     char* scratch, hipStream_t s) {
    const size_t n = (size_t)(M + 1) * (L + 1);
    const int fill_blocks = (int)std::min<size_t>((n + INST_BLOCK - 1) / INST_BLOCK, 1024);
    const InstScratch sc = InstScratch::carve(scratch, M, L, nullptr);
    hipLaunchKernelGGL(inst_fill_kernel, dim3(fill_blocks), dim3(INST_BLOCK), 0, s, n, table, P == 0 ? (size_t)0 : (size_t)INST_REST_COPIES * (L + 1),
                       sc.rest, M, P == 0 ? 1 : 0, mapping, best_label, best_iou);
    if (P == 0) return hipGetLastError();
    hipLaunchKernelGGL(inst_overlap_kernel, dim3(inst_grid(P)), dim3(INST_BLOCK), 0, s, P, M, L, acc_view, acc, table, sc.rest);
    const int row_blocks = (M + INST_BLOCK / 64 - 1) / (INST_BLOCK / 64), col_blocks = (L + INST_BLOCK - 1) / INST_BLOCK;
    // (L + 1 columns: one more thread than col_blocks * INST_BLOCK may hold)
    hipLaunchKernelGGL(inst_sums_kernel, dim3(row_blocks + (L + 1 + INST_BLOCK - 1) / INST_BLOCK), dim3(INST_BLOCK), 0, s, M, L, row_blocks, table, sc);
    hipLaunchKernelGGL(inst_best_kernel, dim3(row_blocks), dim3(INST_BLOCK), 0, s, M, L, table, sc, count, best_label, best_iou);
    hipLaunchKernelGGL(inst_winner_kernel, dim3(col_blocks), dim3(INST_BLOCK), 0, s, M, L, iou_thresh, best_label, best_iou, sc);
    hipLaunchKernelGGL(inst_assign_kernel, dim3(1), dim3(INST_MAX_M), 0, s, M, L, iou_thresh, min_weight, best_label, best_iou, sc, count,
                       dropped, mapping);
    return hipGetLastError();
}

hipError_t launch_instance_merge(int P, int M, int L, float* acc_view, bool clear_view, const int* mapping, float* acc, hipStream_t s) {
    hipLaunchKernelGGL(inst_merge_kernel, dim3(inst_grid(P)), dim3(INST_BLOCK), 0, s, P, M, L, acc_view, clear_view ? 1 : 0, mapping, acc);
    return hipGetLastError();
}

// nullptr if the sizes are taken, else the reason
const char* instance_bad_sizes(int P, int M, int L) {
    if (P < 0) return "%s: P < 0 (P = %d, M = %d, L = %d)";
    if (M < 1 || M > F3DGS_INSTANCE_MAX_MASKS) return "%s: bad sizes: M outside 1 .. 1024 (P = %d, M = %d, L = %d)";
    if (L < 1 || L > F3DGS_INSTANCE_MAX_INSTANCES) return "%s: bad sizes: L outside 1 .. 4096 (P = %d, M = %d, L = %d)";
    return nullptr;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_instance_scratch_bytes(int M, int L) {
    if (instance_bad_sizes(0, M, L)) return 0;
    return instance_scratch_bytes(M, L);
}

int f3dgs_instance_associate(int P, int M, int L, const float* acc_view, const float* acc, double iou_thresh, double min_weight,
                             int32_t* count, int32_t* dropped, int32_t* mapping, int32_t* best_label, double* best_iou, float* table,
                             void* scratch, void* stream) {
    const char* who = "f3dgs_instance_associate";
    if (const char* why = instance_bad_sizes(P, M, L)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, why, who, P, M, L);
    if (!(iou_thresh >= 0.0)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: iou_thresh is negative or NaN", who);
    if (!(min_weight >= 0.0)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: min_weight is negative or NaN", who);
    if (!count || !dropped || !mapping || !best_label || !best_iou || !table || !scratch || (P > 0 && (!acc_view || !acc)))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (!aligned16(scratch)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch must be 16-byte aligned", who);
    HIP_TRY(launch_instance_associate(P, M, L, acc_view, acc, iou_thresh, min_weight, count, dropped, mapping, best_label, best_iou, table,
                                      static_cast<char*>(scratch), static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

int f3dgs_instance_merge(int P, int M, int L, float* acc_view, int clear_view, const int32_t* mapping, float* acc, void* stream) {
    const char* who = "f3dgs_instance_merge";
    if (const char* why = instance_bad_sizes(P, M, L)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, why, who, P, M, L);
    if (!mapping || (P > 0 && (!acc_view || !acc))) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (P == 0) return F3DGS_OK;      // no rows: nothing to add
    HIP_TRY(launch_instance_merge(P, M, L, acc_view, clear_view != 0, mapping, acc, static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

}  // extern "C"
