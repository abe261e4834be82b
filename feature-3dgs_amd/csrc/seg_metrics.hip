// seg_metrics.hip - segmentation scores of N rendered views in one launch chain, and the palette pictures of a label map
// (include/f3dgs.h: f3dgs_seg_metrics*, f3dgs_seg_colorize).
//
// Replaces the scoring half of the reference's semantic-segmentation evaluation (encoders/lseg_encoder/segmentation_metric.py:58-108
// calculate_accuracy, calculate_accuracy_mask, calculate_iou, calculate_iou_mask; :818-832 the per-view calls), which per view
// builds two boolean maps and four host sums per class, and the pictures of segmentation.py:547-559.  Stages:
//   K0 sm_clear_kernel    zeroes the counter block (a kernel, not a memset node: api.hip, zero_fill)
//   K1 sm_count_kernel    workgroup b of view n walks tiles b, b + bpv, ... of 1024 pixels of that view.   Per tile every map's
//                         span is staged into LDS as 16-bit labels - whole aligned 4-element groups by vector loads, the
//                         groups that reach over either end of the (N,H,W) block element by element; the range test
//                         0 <= v < L is made on the loaded value at its full width and a value outside becomes BAD - and
//                         the pixels are counted into per-label LDS counters.  The lanes of a wave that hold the same
//                         (teacher, student, gt) triple are folded into ONE add of their number (up to FOLD_ROUNDS distinct
//                         triples per wave-step; what is left adds for itself), so a view of one label does not serialise
//                         64 ways on one LDS word.  At the end the non-zero counters go to global memory by 64-bit adds.
//   K2 sm_finish_kernel   one workgroup per view, plus one for the pooled row (label-wise sums of the counters over the N
//                         views and the caller's carry): ranks the labels by counting, fp64 accuracy and IoU.
// Integer atomics only: two calls give the same bits.  No host read and no memset: the call may be captured into a graph.

#include <math.h>

#include "common.h"

namespace f3dgs {

namespace {

constexpr int MAXL = F3DGS_SEGMENT_MAX_TEXTS;   // label slots
constexpr int TILE_PIX = 1024;                  // pixels a workgroup stages at a time: 4 per thread
constexpr int MAX_BLOCKS_PER_VIEW = 32;         // workgroups per view: each flushes its counters once
constexpr int MAX_VIEWS = 1 << 16;              // views per call
constexpr int FOLD_ROUNDS = 4;
constexpr uint32_t BAD = 0xFFFFu;               // staged value of a label outside [0, L)
constexpr int NARR = 7;                         // counter arrays: n_t, n_s, n_ts, n_g, m_g, m_s, m_gs
constexpr int NSCAL = 5;                        // scalars: valid, equal, invalid, matched, correct
enum { A_NT = 0, A_NS, A_NTS, A_NG, A_MG, A_MS, A_MGS };
enum { S_VALID = 0, S_EQUAL, S_INVALID, S_MATCHED, S_CORRECT };

struct Map {
    const void* p;     // (N,H,W) block, aligned to its element size
    int fmt;           // F3DGS_LABELS_*
};

// the staged 16-bit label of a value of any width: the comparison is made before anything is narrowed
__device__ __forceinline__ uint32_t stage_u8(uint32_t v, uint32_t L) { return v < L ? v : BAD; }
__device__ __forceinline__ uint32_t stage_i32(int32_t v, uint32_t L) { return (uint32_t)v < L ? (uint32_t)v : BAD; }
__device__ __forceinline__ uint32_t stage_i64(int64_t v, uint32_t L) { return (uint64_t)v < (uint64_t)L ? (uint32_t)v : BAD; }

__device__ __forceinline__ uint32_t load_one(const Map& m, size_t e, uint32_t L) {
    if (m.fmt == F3DGS_LABELS_U8) return stage_u8(static_cast<const unsigned char*>(m.p)[e], L);
    if (m.fmt == F3DGS_LABELS_I32) return stage_i32(static_cast<const int32_t*>(m.p)[e], L);
    return stage_i64(static_cast<const int64_t*>(m.p)[e], L);
}

// Elements [g0, g0 + len) of the block of `total` elements -> dst[0 .. len).  `mis` = (address of element 0 / element size) % 4:
// group k covers elements a0 + 4 k .. + 3 with a0 = g0 - (g0 + mis) % 4, so its address is a multiple of four elements.
__device__ __forceinline__ void stage_map(uint16_t* dst, const Map& m, uint32_t mis, size_t g0, int len, size_t total, uint32_t L) {
    const int back = (int)((g0 + mis) & 3);
    const int groups = (back + len + 3) >> 2;                  // <= 257
    for (int k = threadIdx.x; k < groups; k += 256) {
        const int first = 4 * k - back;                        // position in dst of the group's first element, may be < 0
        uint32_t v[4];
        // whole group inside the block (first >= -3, so g0 + first cannot wrap once g0 >= 3; the test below covers g0 < 3)
        const bool inside = (first >= 0 || g0 >= (size_t)(-first)) && g0 + first + 4 <= total;
        if (inside) {
            const size_t e = g0 + first;
            if (m.fmt == F3DGS_LABELS_U8) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(static_cast<const unsigned char*>(m.p) + e);
#pragma unroll
                for (int j = 0; j < 4; j++) v[j] = stage_u8((w >> (8 * j)) & 255u, L);
            } else if (m.fmt == F3DGS_LABELS_I32) {
                const int4 w = *reinterpret_cast<const int4*>(static_cast<const int32_t*>(m.p) + e);
                v[0] = stage_i32(w.x, L); v[1] = stage_i32(w.y, L); v[2] = stage_i32(w.z, L); v[3] = stage_i32(w.w, L);
            } else {
                const longlong2* const q = reinterpret_cast<const longlong2*>(static_cast<const int64_t*>(m.p) + e);
                const longlong2 w0 = q[0], w1 = q[1];
                v[0] = stage_i64(w0.x, L); v[1] = stage_i64(w0.y, L); v[2] = stage_i64(w1.x, L); v[3] = stage_i64(w1.y, L);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int d = first + j;
                v[j] = (d >= 0 && d < len) ? load_one(m, g0 + d, L) : BAD;      // (d in [0, len) lies inside the block)
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int d = first + j;
            if (d >= 0 && d < len) dst[d] = (uint16_t)v[j];
        }
    }
}

__device__ __forceinline__ void zero_counters(int64_t* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0;
}
__global__ void __launch_bounds__(256) sm_clear_kernel(int64_t* __restrict__ p, size_t n) { zero_counters(p, n); }

// the adds of one (teacher, student, gt) triple, c pixels of it
template <bool GT>
__device__ __forceinline__ void add_triple(uint32_t (*cnt)[MAXL], uint32_t t, uint32_t s, uint32_t g, uint32_t c) {
    atomicAdd(&cnt[A_NT][t], c);
    atomicAdd(&cnt[A_NS][s], c);
    if (t == s) atomicAdd(&cnt[A_NTS][t], c);
    if constexpr (GT) {
        atomicAdd(&cnt[A_NG][g], c);
        if (g == t) {
            atomicAdd(&cnt[A_MG][g], c);
            atomicAdd(&cnt[A_MS][s], c);
            if (s == g) atomicAdd(&cnt[A_MGS][g], c);
        }
    }
}

// Counter block: int64 counts[A][N + 1][L] (A = 7 with gt, 3 without), then int64 scalars[5][N + 1]; row N is the pooled one.
// grid: N x bpv workgroups, view-major.  H W < 2^31: a 32-bit LDS counter cannot overflow.
template <bool GT>
__global__ void __launch_bounds__(256)
sm_count_kernel(int N, uint32_t bpv, uint32_t HW, uint32_t L, Map mt, Map ms, Map mg, uint32_t mis_t, uint32_t mis_s, uint32_t mis_g,
                int64_t* __restrict__ counts, int64_t* __restrict__ scalars) {
    constexpr int A = GT ? NARR : 3;
    __shared__ uint32_t cnt[A][MAXL];
    __shared__ uint32_t scal[NSCAL];
    __shared__ uint16_t lab[GT ? 3 : 2][TILE_PIX];
    const int n = blockIdx.x / bpv;
    const uint32_t b = blockIdx.x - n * bpv;
    for (int i = threadIdx.x; i < A * MAXL; i += 256) (&cnt[0][0])[i] = 0;
    if (threadIdx.x < NSCAL) scal[threadIdx.x] = 0;
    const size_t total = (size_t)N * HW, view0 = (size_t)n * HW;
    const uint32_t tiles = (HW + TILE_PIX - 1) / TILE_PIX;
    uint32_t valid = 0, equal = 0, matched = 0, correct = 0, invalid = 0;      // this thread's pixels
    const int lane = threadIdx.x & 63;
    for (uint32_t tile = b; tile < tiles; tile += bpv) {
        const uint32_t p0 = tile * TILE_PIX;
        const int len = (int)min((uint32_t)TILE_PIX, HW - p0);
        __syncthreads();                                   // the previous tile's labels are read, the counters are zero
        stage_map(lab[0], mt, mis_t, view0 + p0, len, total, L);
        stage_map(lab[1], ms, mis_s, view0 + p0, len, total, L);
        if constexpr (GT) stage_map(lab[2], mg, mis_g, view0 + p0, len, total, L);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < TILE_PIX / 256; it++) {
            const int d = it * 256 + threadIdx.x;
            const bool in = d < len;
            uint32_t t = BAD, s = BAD, g = 0;
            if (in) {
                t = lab[0][d];
                s = lab[1][d];
                if constexpr (GT) g = lab[2][d];
            }
            const bool ok = in && t != BAD && s != BAD && g != BAD;
            if (in && !ok) invalid++;
            if (ok) {
                valid++;
                equal += t == s;
                if constexpr (GT) {
                    matched += g == t;
                    correct += g == t && s == g;
                }
            }
            // fold the lanes of equal triples: the lowest pending lane names a triple, its holders leave, it adds their number
            const uint32_t key = t | (s << 8) | (g << 16);         // (t, s, g < 256 where ok)
            bool pending = ok;
#pragma unroll 1
            for (int r = 0; r < FOLD_ROUNDS; r++) {
                const uint64_t open = __ballot(pending);
                if (open == 0) break;
                const int leader = __ffsll((unsigned long long)open) - 1;
                const uint32_t lk = (uint32_t)__shfl((int)key, leader, 64);
                const uint64_t same = __ballot(pending && key == lk);
                if (pending && key == lk) {
                    pending = false;
                    if (lane == leader) add_triple<GT>(cnt, t, s, g, (uint32_t)__popcll(same));
                }
            }
            if (pending) add_triple<GT>(cnt, t, s, g, 1u);
        }
    }
    const uint32_t mine[NSCAL] = {valid, equal, invalid, matched, correct};
#pragma unroll
    for (int k = 0; k < NSCAL; k++) {
        uint32_t v = mine[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
        if (lane == 0 && v) atomicAdd(&scal[k], v);
    }
    __syncthreads();
    // flush: thread i owns label i
    if (threadIdx.x < L) {
#pragma unroll
        for (int a = 0; a < A; a++) {
            const uint32_t v = cnt[a][threadIdx.x];
            if (v) atomicAdd(reinterpret_cast<unsigned long long*>(counts + ((size_t)a * (N + 1) + n) * L + threadIdx.x),
                             (unsigned long long)v);
        }
    }
    if (threadIdx.x < NSCAL) {
        const uint32_t v = scal[threadIdx.x];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(scalars + (size_t)threadIdx.x * (N + 1) + n), (unsigned long long)v);
    }
}

struct FinishOut {
    double* scores;          // [2 K][N + 1]: accuracy, iou (, accuracy_masked, iou_masked)
    double* iou_per_label;   // [K][N + 1][L]
    int64_t* labels_ranked;  // [K][N + 1][num_classes]
};

// One ranking and its mean IoU, by the whole workgroup: thread i < L holds label i's rank key and its intersection / union.
// Rank = how many labels go ahead: a larger key, or an equal key and a lower label.  Kept: rank < num_classes and key > 0 (the
// labels of key 0 rank behind every other one).  The mean adds the kept, non-NaN values in rank order.
__device__ __forceinline__ double ranked_mean(int L, int num_classes, int64_t key, int64_t inter, int64_t uni, int64_t* keys,
                                              double* by_rank, int64_t* label_by_rank, double* per_label, int64_t* ranked) {
    const int i = threadIdx.x;
    __syncthreads();
    if (i < L) keys[i] = key;
    if (i < num_classes) { by_rank[i] = nan(""); label_by_rank[i] = -1; }
    __syncthreads();
    if (i < L) {
        int rank = 0;
        for (int j = 0; j < L; j++) {
            const int64_t kj = keys[j];
            rank += (kj > key || (kj == key && j < i)) ? 1 : 0;
        }
        const bool kept = rank < num_classes && key > 0;
        const double iou = uni > 0 ? (double)inter / (double)uni : nan("");
        per_label[i] = kept ? iou : nan("");
        if (kept) { by_rank[rank] = iou; label_by_rank[rank] = i; }
    }
    __syncthreads();
    if (i < num_classes) ranked[i] = label_by_rank[i];
    double mean = nan("");
    if (i == 0) {
        double sum = 0.0;
        int terms = 0;
        for (int r = 0; r < num_classes; r++) {
            const double v = by_rank[r];
            if (v == v) { sum += v; terms++; }
        }
        if (terms) mean = sum / (double)terms;
    }
    return mean;      // (thread 0's)
}

// grid N + 1: row n < N is view n, row N pools the views (and `carry_*`, the pooled counters of earlier calls) and writes its
// sums into row N of the counter block.
template <bool GT>
__global__ void __launch_bounds__(256)
sm_finish_kernel(int N, int L, int num_classes, int64_t* __restrict__ counts, int64_t* __restrict__ scalars,
                 const int64_t* __restrict__ carry_counts, const int64_t* __restrict__ carry_scalars, FinishOut o) {
    constexpr int A = GT ? NARR : 3;
    __shared__ int64_t keys[MAXL];
    __shared__ double by_rank[MAXL];
    __shared__ int64_t label_by_rank[MAXL];
    __shared__ int64_t sc[NSCAL];
    const int row = blockIdx.x, i = threadIdx.x;
    const size_t R = (size_t)N + 1;
    int64_t c[A];
#pragma unroll
    for (int a = 0; a < A; a++) c[a] = 0;
    if (row < N) {
        if (i < L)
#pragma unroll
            for (int a = 0; a < A; a++) c[a] = counts[((size_t)a * R + row) * L + i];
        if (i < NSCAL) sc[i] = scalars[(size_t)i * R + row];
    } else {
        if (i < L) {
#pragma unroll
            for (int a = 0; a < A; a++) {
                int64_t v = carry_counts ? carry_counts[(size_t)a * L + i] : 0;
                for (int n = 0; n < N; n++) v += counts[((size_t)a * R + n) * L + i];
                c[a] = v;
                counts[((size_t)a * R + N) * L + i] = v;
            }
        }
        if (i < NSCAL) {
            int64_t v = carry_scalars ? carry_scalars[i] : 0;
            for (int n = 0; n < N; n++) v += scalars[(size_t)i * R + n];
            sc[i] = v;
            scalars[(size_t)i * R + N] = v;
        }
    }
    if (!o.scores) return;      // (the same in every thread)
    {
        const int64_t both = c[A_NT] + c[A_NS];
        const double mean = ranked_mean(L, num_classes, both, c[A_NTS], both - c[A_NTS], keys, by_rank, label_by_rank,
                                        o.iou_per_label + (size_t)row * L, o.labels_ranked + (size_t)row * num_classes);
        if (i == 0) {
            o.scores[0 * R + row] = (double)sc[S_EQUAL] / (double)sc[S_VALID];       // 0 / 0: NaN, as the reference
            o.scores[1 * R + row] = mean;
        }
    }
    if constexpr (GT) {
        const double mean = ranked_mean(L, num_classes, c[A_NG] + c[A_NT] + c[A_NS], c[A_MGS], c[A_MG] + c[A_MS] - c[A_MGS], keys,
                                        by_rank, label_by_rank, o.iou_per_label + (R + row) * L,
                                        o.labels_ranked + (R + row) * num_classes);
        if (i == 0) {
            o.scores[2 * R + row] = (double)sc[S_CORRECT] / (double)sc[S_MATCHED];
            o.scores[3 * R + row] = mean;
        }
    }
}

// ---- colour -----------------------------------------------------------------------------------------------------------------
// What `(vis.numpy() * 255).astype(np.uint8)` makes of v in [0, 1]; the clamp defines the values outside, NaN gives 0.
__device__ __forceinline__ unsigned char to_byte(float v) { return (unsigned char)fminf(fmaxf(__fmul_rn(v, 255.0f), 0.0f), 255.0f); }

// One thread per output pixel (n, y, x') of the (N, H, W', 3) picture; W' = 3 W for the strip.
__global__ void __launch_bounds__(256)
sm_colorize_kernel(size_t pixels, uint32_t HW, uint32_t W, uint32_t L, Map labels, const unsigned char* __restrict__ palette,
                   const float* __restrict__ image, int mode, float a, float b, uint32_t fill, unsigned char* __restrict__ out) {
    __shared__ unsigned char pal[MAXL * 3];
    for (uint32_t i = threadIdx.x; i < 3 * L; i += 256) pal[i] = palette[i];
    __syncthreads();
    const uint32_t Wo = mode == F3DGS_SEG_COLOR_STRIP ? 3 * W : W;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < pixels; o += (size_t)gridDim.x * 256) {
        const size_t line = o / Wo;                       // n H + y
        const uint32_t xo = (uint32_t)(o - line * Wo);
        const uint32_t part = mode == F3DGS_SEG_COLOR_STRIP ? xo / W : (mode == F3DGS_SEG_COLOR_BLEND ? 1u : 2u);
        const uint32_t x = xo - (mode == F3DGS_SEG_COLOR_STRIP ? part * W : 0u);
        const size_t p = line * W + x;                    // pixel of the (N,H,W) block
        unsigned char rgb[3];
        uint32_t m[3] = {fill & 255u, (fill >> 8) & 255u, (fill >> 16) & 255u};
        if (part != 0) {
            const uint32_t l = load_one(labels, p, L);
            if (l != BAD) { m[0] = pal[3 * l]; m[1] = pal[3 * l + 1]; m[2] = pal[3 * l + 2]; }
        }
        if (part == 2) {
            rgb[0] = (unsigned char)m[0]; rgb[1] = (unsigned char)m[1]; rgb[2] = (unsigned char)m[2];
        } else {
            const size_t n = p / HW, q = p - n * HW;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const float v = image[(n * 3 + ch) * HW + q];
                // the reference's chain, one rounding per operation: mask / 255, img * a, mask * b, their sum
                rgb[ch] = part == 0 ? to_byte(v)
                                    : to_byte(__fadd_rn(__fmul_rn(v, a), __fmul_rn(__fdiv_rn((float)m[ch], 255.0f), b)));
            }
        }
        out[3 * o] = rgb[0]; out[3 * o + 1] = rgb[1]; out[3 * o + 2] = rgb[2];
    }
}

bool known_format(int f) { return f == F3DGS_LABELS_U8 || f == F3DGS_LABELS_I32 || f == F3DGS_LABELS_I64; }
size_t element_size(int f) { return f == F3DGS_LABELS_U8 ? 1 : (f == F3DGS_LABELS_I32 ? 4 : 8); }
uint32_t misalignment(const void* p, int f) { return (uint32_t)((reinterpret_cast<uintptr_t>(p) / element_size(f)) & 3); }

struct Block {
    size_t count_words, words;     // int64 words of the counts, of the whole counter block
};
Block counter_block(int N, int L, bool gt) {
    Block b;
    b.count_words = (size_t)(gt ? NARR : 3) * ((size_t)N + 1) * L;
    b.words = b.count_words + (size_t)NSCAL * ((size_t)N + 1);
    return b;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_seg_metrics_scratch_bytes(int N, int L, int has_gt) {
    if (N < 1 || N > MAX_VIEWS || L < 1 || L > MAXL) return 0;
    return counter_block(N, L, has_gt != 0).words * sizeof(int64_t);
}

int f3dgs_seg_metrics(int N, int H, int W, int L, int num_classes, const void* teacher, int teacher_format, const void* student,
                      int student_format, const void* gt, int gt_format, const int64_t* carry_counts, const int64_t* carry_scalars,
                      int64_t* counters, double* scores, double* iou_per_label, int64_t* labels_ranked, void* stream) {
    if (N == 0) return F3DGS_OK;
    if (N < 0 || H < 1 || W < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_metrics: bad sizes N=%d H=%d W=%d", N, H, W);
    // (the count grid is up to MAX_BLOCKS_PER_VIEW x N workgroups of 256 threads: 2^29 threads at the limit, a launch takes 2^32)
    if (N > MAX_VIEWS) return report_errorf(F3DGS_ERR_UNSUPPORTED, "seg_metrics: N=%d views: up to %d per call are supported", N, MAX_VIEWS);
    if ((size_t)H * W > 0x7fffffffull)
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "seg_metrics: views of %d x %d pixels: fewer than 2^31 are supported", H, W);
    if (L < 1 || L > MAXL) return report_errorf(F3DGS_ERR_UNSUPPORTED, "seg_metrics: L=%d label slots: 1 to %d are supported", L, MAXL);
    if (num_classes < 1 || num_classes > L)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_metrics: num_classes=%d outside 1..L=%d", num_classes, L);
    if (!known_format(teacher_format) || !known_format(student_format) || (gt && !known_format(gt_format)))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_metrics: unknown label format %d / %d / %d", teacher_format, student_format,
                             gt_format);
    if (!teacher || !student || !counters) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_metrics: null pointer");
    if ((scores || iou_per_label || labels_ranked) && !(scores && iou_per_label && labels_ranked))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_metrics: scores, iou_per_label and labels_ranked go together");
    if ((carry_counts == nullptr) != (carry_scalars == nullptr))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_metrics: carry_counts and carry_scalars go together");
    const Map maps[3] = {{teacher, teacher_format}, {student, student_format}, {gt, gt ? gt_format : F3DGS_LABELS_U8}};
    for (const Map& m : maps)
        if (m.p && (reinterpret_cast<uintptr_t>(m.p) % element_size(m.fmt)))
            return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_metrics: a label map is not aligned to its element size");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Block blk = counter_block(N, L, gt != nullptr);
    int64_t* const scal = counters + blk.count_words;
    const unsigned clear_grid = (unsigned)std::min<size_t>((blk.words + 255) / 256, 1024);
    hipLaunchKernelGGL(sm_clear_kernel, dim3(clear_grid), dim3(256), 0, s, counters, blk.words);
    const uint32_t HW = (uint32_t)((size_t)H * W);
    const uint32_t tiles = (HW + TILE_PIX - 1) / TILE_PIX;
    const uint32_t bpv = std::min<uint32_t>(tiles, MAX_BLOCKS_PER_VIEW);
    const dim3 grid(bpv * (unsigned)N);
    const uint32_t mt = misalignment(teacher, teacher_format), ms = misalignment(student, student_format);
    const FinishOut fo{scores, iou_per_label, labels_ranked};
    if (gt) {
        hipLaunchKernelGGL(sm_count_kernel<true>, grid, dim3(256), 0, s, N, bpv, HW, (uint32_t)L, maps[0], maps[1], maps[2], mt, ms,
                           misalignment(gt, gt_format), counters, scal);
        hipLaunchKernelGGL(sm_finish_kernel<true>, dim3(N + 1), dim3(256), 0, s, N, L, num_classes, counters, scal, carry_counts,
                           carry_scalars, fo);
    } else {
        hipLaunchKernelGGL(sm_count_kernel<false>, grid, dim3(256), 0, s, N, bpv, HW, (uint32_t)L, maps[0], maps[1], maps[2], mt, ms, 0u,
                           counters, scal);
        hipLaunchKernelGGL(sm_finish_kernel<false>, dim3(N + 1), dim3(256), 0, s, N, L, num_classes, counters, scal, carry_counts,
                           carry_scalars, fo);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "seg_metrics: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

int f3dgs_seg_colorize(int N, int H, int W, int L, const void* labels, int labels_format, const unsigned char* palette,
                       const float* image, int mode, float a, float b, const unsigned char* fill, unsigned char* out, void* stream) {
    if (N == 0) return F3DGS_OK;
    if (N < 0 || H < 1 || W < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_colorize: bad sizes N=%d H=%d W=%d", N, H, W);
    if ((size_t)H * W > 0x7fffffffull / 3)
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "seg_colorize: views of %d x %d pixels are too large", H, W);
    if (L < 1 || L > MAXL) return report_errorf(F3DGS_ERR_UNSUPPORTED, "seg_colorize: L=%d palette rows: 1 to %d are supported", L, MAXL);
    if (mode != F3DGS_SEG_COLOR_MASK && mode != F3DGS_SEG_COLOR_BLEND && mode != F3DGS_SEG_COLOR_STRIP)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_colorize: unknown mode %d", mode);
    if (!known_format(labels_format)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_colorize: unknown label format %d", labels_format);
    if (!labels || !palette || !out || (mode != F3DGS_SEG_COLOR_MASK && !image))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_colorize: null pointer");
    if (reinterpret_cast<uintptr_t>(labels) % element_size(labels_format))
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "seg_colorize: the label map is not aligned to its element size");
    const uint32_t f = fill ? (uint32_t)fill[0] | ((uint32_t)fill[1] << 8) | ((uint32_t)fill[2] << 16) : 0u;      // (host memory)
    const size_t pixels = (size_t)N * H * W * (mode == F3DGS_SEG_COLOR_STRIP ? 3 : 1);
    const unsigned grid = (unsigned)std::min<size_t>((pixels + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(sm_colorize_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), pixels, (uint32_t)(H * W),
                       (uint32_t)W, (uint32_t)L, Map{labels, labels_format}, palette, image, mode, a, b, f, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "seg_colorize: %s", hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
