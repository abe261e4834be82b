// sam_masks.hip - what runs after SAM's mask decoder, from the low-resolution logits to the list of mask records, without the
// full-size float masks ever existing (include/f3dgs.h: f3dgs_sam_masks*, f3dgs_sam_upscale, f3dgs_box_nms*, f3dgs_mask_rle_*,
// f3dgs_mask_unpack).
//
// Replaces, of the reference's encoders/sam_encoder/segment_anything: Sam.postprocess_masks (modeling/sam.py:133-162: two bilinear
// resizes around a crop), calculate_stability_score, the threshold, batched_mask_to_box, is_box_near_crop_edge, uncrop_masks and
// mask_to_rle_pytorch (utils/amg.py), as automatic_mask_generator.py:295-320 chains them, and torchvision's batched_nms.  Kernels:
//   sam_init_kernel       the (M, 8) int32 block of raw statistics: counts 0, minima INT_MAX, maxima -1 (a kernel, not a memset)
//   sam_pass_kernel<0>    one workgroup per (mask, 64 x 64 tile OF THE FRAME).  The stage-1 values (h x w -> S x S, kept to
//                         ih x iw) that the tile's taps reach are formed once into LDS - a dense patch of rows r_lo..r_hi and
//                         columns c_lo..c_hi; where that patch would not fit (a strong down-scale) every tap forms its stage-1
//                         value for itself, by the same arithmetic.  Stage 2 runs from the patch with the LANES ALONG y: the
//                         ballot of v > t over a wave IS the two packed words (x, y / 32) of a column, the counts are popcounts
//                         of three ballots, the box is a min / max over columns and the first / last set bit of the ballots'
//                         union.  One set of integer atomics per workgroup.  A tile outside the crop, and every tile of a mask
//                         that failed the predicted-IoU test, writes its zero words and returns.
//   sam_pass_kernel<1|2>  the same body with the lanes along x, storing v (float) or v > t (bool): f3dgs_sam_upscale
//   sam_finish_kernel     one workgroup: boxes by batched_mask_to_box's rule, stability, the three filters, the ascending list
//                         of kept masks and their number
//   nms_matrix_kernel     bit (i, j) of an M x ceil(M / 64) word matrix: j > i and IoU(box i, box j) > threshold (boxes in score order)
//   nms_sweep_kernel      one workgroup walks the rows 64 at a time: the 64 x 64 diagonal block is resolved in registers, the
//                         rows of the kept boxes are OR-ed into one `removed` word per thread
//   rle_count_kernel, rle_emit_kernel, unpack_kernel   run lengths down the columns of the packed masks
// Both resizes are PyTorch's upsample_bilinear2d with align_corners = False, in fp32, one rounding per operation (this unit is
// compiled with -ffp-contract=off): scale = (float)in / out, src = max(scale * (dst + 0.5f) - 0.5f, 0), i1 = i0 + (i0 < in - 1),
// value = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d).  Integer atomics only: two calls give the same bits.

#include <limits.h>
#include <math.h>

#include "common.h"

namespace f3dgs {

namespace {

constexpr int TS = 64;                  // tile edge: one wave of lanes along it
constexpr int PATCH_MAX = 6144;         // floats of the stage-1 patch (24 KB): an up-scale needs at most 66 x 67
constexpr int RAW = 8;                  // raw statistics per mask: n_hi, n_lo, area, xmin, ymin, xmax, ymax, unused
constexpr int MAX_MASKS = 65535;        // grid.y
constexpr int NMS_MAX = F3DGS_BOX_NMS_MAX;

struct Geo {
    int h, w;          // low-resolution logits
    int ih, iw;        // the part of the S x S grid that is kept
    int H, W;          // output (the crop)
    float s1y, s1x;    // (float)h / S, (float)w / S
    float s2y, s2x;    // (float)ih / H, (float)iw / W
};

struct Frame {
    int FH, FW, NW;    // frame, words per column = ceil(FH / 32)
    int cx0, cy0;      // crop origin
};

struct Tap {
    int i0, i1;
    float l0, l1;
};

// area_pixel_compute_source_index and the two neighbours of upsample_bilinear2d (the index is clamped as the CPU kernel clamps
// it; in range that changes nothing)
__device__ __forceinline__ Tap tap(float scale, int dst, int in) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    Tap t;
    t.i0 = min((int)src, in - 1);
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = fminf(fmaxf(src - (float)t.i0, 0.0f), 1.0f);
    t.l0 = 1.0f - t.l1;
    return t;
}

__device__ __forceinline__ float blend4(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
    return ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * c + tx.l1 * d);
}

// value (r, c) of the S x S grid, 0 <= r < ih <= S, 0 <= c < iw <= S
__device__ __forceinline__ float stage1(const float* __restrict__ lr, const Geo& g, int r, int c) {
    const Tap ty = tap(g.s1y, r, g.h), tx = tap(g.s1x, c, g.w);
    const float* const r0 = lr + (size_t)ty.i0 * g.w;
    const float* const r1 = lr + (size_t)ty.i1 * g.w;
    return blend4(ty, tx, r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1]);
}

struct Patch {
    const float* lds;
    int r_lo, c_lo, pitch;
    bool on;
};

__device__ __forceinline__ float stage2(const Tap& ty, const Tap& tx, const Patch& p, const float* __restrict__ lr, const Geo& g) {
    if (p.on) {
        const float* const q0 = p.lds + (ty.i0 - p.r_lo) * p.pitch - p.c_lo;
        const float* const q1 = p.lds + (ty.i1 - p.r_lo) * p.pitch - p.c_lo;
        return blend4(ty, tx, q0[tx.i0], q0[tx.i1], q1[tx.i0], q1[tx.i1]);
    }
    return blend4(ty, tx, stage1(lr, g, ty.i0, tx.i0), stage1(lr, g, ty.i0, tx.i1), stage1(lr, g, ty.i1, tx.i0), stage1(lr, g, ty.i1, tx.i1));
}

__global__ void __launch_bounds__(256) sam_init_kernel(int M, int32_t* __restrict__ raw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * RAW) return;
    const int f = i % RAW;
    raw[i] = (f == 3 || f == 4) ? INT_MAX : (f == 5 || f == 6) ? -1 : 0;
}

// MODE 0: packed bits and statistics (lanes along y, tiles of the frame); 1: dense float; 2: dense bool (lanes along x, tiles of the crop)
template <int MODE>
__global__ void __launch_bounds__(256) sam_pass_kernel(Geo g, Frame fr, int tiles_x, const float* __restrict__ low_res,
                                                       const float* __restrict__ iou, float iou_thr, float t, float t_hi, float t_lo,
                                                       uint32_t* __restrict__ packed, int32_t* __restrict__ raw, void* __restrict__ dense) {
    __shared__ float s_patch[PATCH_MAX];
    __shared__ int32_t s_red[4][RAW];
    const int m = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fx0 = (blockIdx.x % tiles_x) * TS, fy0 = (blockIdx.x / tiles_x) * TS;
    // the tile's part of the crop, in the crop's coordinates
    const int xa = max(fx0 - fr.cx0, 0), xb = min(fx0 + TS - 1 - fr.cx0, g.W - 1);
    const int ya = max(fy0 - fr.cy0, 0), yb = min(fy0 + TS - 1 - fr.cy0, g.H - 1);
    const bool skipped = iou != nullptr && !(iou[m] > iou_thr);            // (strict; NaN fails)
    if (skipped || xa > xb || ya > yb) {
        if constexpr (MODE == 0) {
            const int j = threadIdx.x >> 1, k = (fy0 >> 5) + (threadIdx.x & 1);      // 64 columns x 2 words
            if (threadIdx.x < 2 * TS && fx0 + j < fr.FW && k < fr.NW) packed[((size_t)m * fr.FW + fx0 + j) * fr.NW + k] = 0u;
        }
        return;
    }
    const float* const lr = low_res + (size_t)m * g.h * g.w;

    Patch p;
    p.lds = s_patch;
    p.r_lo = tap(g.s2y, ya, g.ih).i0;
    p.c_lo = tap(g.s2x, xa, g.iw).i0;
    const int nr = tap(g.s2y, yb, g.ih).i1 - p.r_lo + 1, nc = tap(g.s2x, xb, g.iw).i1 - p.c_lo + 1;
    p.pitch = nc | 1;
    p.on = nr * p.pitch <= PATCH_MAX;
    if (p.on) {
        for (int i = threadIdx.x; i < nr * nc; i += 256) {
            const int j = i / nc, k = i - j * nc;
            s_patch[j * p.pitch + k] = stage1(lr, g, p.r_lo + j, p.c_lo + k);
        }
        __syncthreads();
    }

    if constexpr (MODE == 0) {
        const int y = fy0 + lane - fr.cy0;
        const bool lane_ok = y >= ya && y <= yb;
        const Tap ty = tap(g.s2y, min(max(y, ya), yb), g.ih);
        int n_hi = 0, n_lo = 0, area = 0, xmin = INT_MAX, xmax = -1;
        unsigned long long rows = 0ull;
        for (int j = wave * (TS / 4); j < (wave + 1) * (TS / 4); j++) {
            const int fx = fx0 + j, x = fx - fr.cx0;
            if (fx >= fr.FW) break;
            unsigned long long bt = 0ull;
            if (x >= xa && x <= xb) {                                       // (the same for the whole wave)
                const Tap tx = tap(g.s2x, x, g.iw);
                const float v = stage2(ty, tx, p, lr, g);
                bt = __ballot(lane_ok && v > t);
                n_hi += __popcll(__ballot(lane_ok && v > t_hi));
                n_lo += __popcll(__ballot(lane_ok && v > t_lo));
                if (bt) {
                    area += __popcll(bt);
                    rows |= bt;
                    xmin = min(xmin, x);
                    xmax = x;
                }
            }
            const int k = (fy0 >> 5) + lane;
            if (lane < 2 && k < fr.NW) packed[((size_t)m * fr.FW + fx) * fr.NW + k] = (uint32_t)(bt >> (32 * lane));
        }
        if (lane == 0) {
            s_red[wave][0] = n_hi;
            s_red[wave][1] = n_lo;
            s_red[wave][2] = area;
            s_red[wave][3] = xmin;
            s_red[wave][4] = rows ? fy0 - fr.cy0 + (int)__builtin_ctzll(rows) : INT_MAX;
            s_red[wave][5] = xmax;
            s_red[wave][6] = rows ? fy0 - fr.cy0 + 63 - (int)__builtin_clzll(rows) : -1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t r[7];
            for (int f = 0; f < 7; f++) r[f] = s_red[0][f];
            for (int w = 1; w < 4; w++) {
                r[0] += s_red[w][0];
                r[1] += s_red[w][1];
                r[2] += s_red[w][2];
                r[3] = min(r[3], s_red[w][3]);
                r[4] = min(r[4], s_red[w][4]);
                r[5] = max(r[5], s_red[w][5]);
                r[6] = max(r[6], s_red[w][6]);
            }
            int32_t* const o = raw + (size_t)m * RAW;
            if (r[0]) atomicAdd(o + 0, r[0]);
            if (r[1]) atomicAdd(o + 1, r[1]);
            if (r[2]) {
                atomicAdd(o + 2, r[2]);
                atomicMin(o + 3, r[3]);
                atomicMin(o + 4, r[4]);
                atomicMax(o + 5, r[5]);
                atomicMax(o + 6, r[6]);
            }
        }
    } else {
        const int x = fx0 + lane;
        const bool lane_ok = x <= xb;
        const Tap tx = tap(g.s2x, min(x, xb), g.iw);
        for (int j = wave * (TS / 4); j < (wave + 1) * (TS / 4); j++) {
            const int y = fy0 + j;
            if (y > yb) break;
            const Tap ty = tap(g.s2y, y, g.ih);
            const float v = stage2(ty, tx, p, lr, g);
            if (lane_ok) {
                const size_t o = ((size_t)m * g.H + y) * g.W + x;
                if constexpr (MODE == 1) static_cast<float*>(dense)[o] = v;
                else static_cast<unsigned char*>(dense)[o] = v > t ? 1 : 0;
            }
        }
    }
}

struct Filter {
    float stability_thresh;      // <= 0: off
    int edge;                    // the crop-edge test on / off
    float crop[4], orig[4];      // XYXY of the crop in the frame and of the frame
};

struct FinishOut {
    int32_t* counts;       // M x 3
    int32_t* box;          // M x 4
    int32_t* box_frame;    // M x 4
    float* stability;      // M
    unsigned char* keep;   // M
    int32_t* kept_index;   // M, ascending, -1 beyond the count
    int32_t* kept_count;   // 1
};

__global__ void __launch_bounds__(256) sam_finish_kernel(int M, const int32_t* __restrict__ raw, const float* __restrict__ iou, float iou_thr,
                                                         Frame fr, Filter fl, FinishOut out) {
    __shared__ int s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int run = 0;
    for (int base = 0; base < M; base += 256) {
        const int m = base + threadIdx.x;
        bool keep = false;
        if (m < M) {
            const int32_t* const r = raw + (size_t)m * RAW;
            const int n_hi = r[0], n_lo = r[1], area = r[2];
            int32_t b[4] = {r[3], r[4], r[5], r[6]};
            if (area == 0) b[0] = b[1] = b[2] = b[3] = 0;
            const int32_t bf[4] = {b[0] + fr.cx0, b[1] + fr.cy0, b[2] + fr.cx0, b[3] + fr.cy0};
            const float stab = __fdiv_rn((float)n_hi, (float)n_lo);          // 0 / 0 = NaN, as the reference's
            bool near = false;
            for (int k = 0; k < 4; k++)
                near |= fabsf((float)bf[k] - fl.crop[k]) <= 20.0f && !(fabsf((float)bf[k] - fl.orig[k]) <= 20.0f);
            keep = (iou == nullptr || iou[m] > iou_thr) && (fl.stability_thresh > 0.0f ? stab >= fl.stability_thresh : true) &&
                   !(fl.edge && near);
            out.counts[3 * m + 0] = n_hi;
            out.counts[3 * m + 1] = n_lo;
            out.counts[3 * m + 2] = area;
            for (int k = 0; k < 4; k++) {
                out.box[4 * m + k] = b[k];
                out.box_frame[4 * m + k] = bf[k];
            }
            out.stability[m] = stab;
            out.keep[m] = keep ? 1 : 0;
        }
        const unsigned long long bal = __ballot(keep);
        __syncthreads();
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; w++) {
            if (w < wave) before += s_w[w];
            total += s_w[w];
        }
        if (keep) out.kept_index[run + before + __popcll(bal & ((1ull << lane) - 1ull))] = m;
        run += total;
    }
    for (int i = run + threadIdx.x; i < M; i += 256) out.kept_index[i] = -1;
    if (threadIdx.x == 0) *out.kept_count = run;
}

// ---- box NMS ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) nms_matrix_kernel(int M, int W64, const float* __restrict__ boxes, const int32_t* __restrict__ cats,
                                                        float thr, unsigned long long* __restrict__ mat) {
    const int bx = blockIdx.x, by = blockIdx.y;
    if (bx < by) return;                                      // (the sweep reads the diagonal and what lies right of it)
    __shared__ float s_box[64][4];
    __shared__ int32_t s_cat[64];
    const int lane = threadIdx.x;
    const int col = bx * 64 + lane;
    if (col < M) {
        for (int k = 0; k < 4; k++) s_box[lane][k] = boxes[4 * (size_t)col + k];
        s_cat[lane] = cats ? cats[col] : 0;
    }
    __syncthreads();
    const int i = by * 64 + lane;
    if (i >= M) return;
    const float x0 = boxes[4 * (size_t)i], y0 = boxes[4 * (size_t)i + 1], x1 = boxes[4 * (size_t)i + 2], y1 = boxes[4 * (size_t)i + 3];
    const float area_i = (x1 - x0) * (y1 - y0);
    const int32_t cat_i = cats ? cats[i] : 0;
    unsigned long long bits = 0ull;
    const int ncol = min(64, M - bx * 64);
    for (int j = 0; j < ncol; j++) {
        if (bx * 64 + j <= i || s_cat[j] != cat_i) continue;
        const float a0 = s_box[j][0], b0 = s_box[j][1], a1 = s_box[j][2], b1 = s_box[j][3];
        const float iw = fmaxf(fminf(x1, a1) - fmaxf(x0, a0), 0.0f), ih = fmaxf(fminf(y1, b1) - fmaxf(y0, b0), 0.0f);
        const float inter = iw * ih;
        const float q = __fdiv_rn(inter, area_i + (a1 - a0) * (b1 - b0) - inter);
        if (q > thr) bits |= 1ull << j;                       // (NaN - two empty boxes - never suppresses)
    }
    mat[(size_t)i * W64 + bx] = bits;
}

__global__ void __launch_bounds__(256) nms_sweep_kernel(int M, int W64, const unsigned long long* __restrict__ mat,
                                                        const int32_t* __restrict__ order, int32_t* __restrict__ keep,
                                                        int32_t* __restrict__ count) {
    __shared__ unsigned long long s_rem[2];
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long mine = 0ull;                           // `removed` bits of boxes 64 tid .. 64 tid + 63
    int run = 0;
    for (int c = 0; c < W64; c++) {
        if (tid == c) s_rem[c & 1] = mine;
        __syncthreads();
        unsigned long long rem = s_rem[c & 1];
        const int left = M - c * 64;
        if (left < 64) rem |= ~0ull << left;
        const int row = c * 64 + lane;
        const unsigned long long d = row < M ? mat[(size_t)row * W64 + c] : 0ull;
        for (int k = 0; k < 64; k++) {
            const unsigned long long dk = __shfl(d, k);
            if (!((rem >> k) & 1ull)) rem |= dk;
        }
        const unsigned long long kept = ~rem;
        if (tid > c && tid < W64)
            for (unsigned long long kk = kept; kk; kk &= kk - 1ull)
                mine |= mat[(size_t)(c * 64 + __builtin_ctzll(kk)) * W64 + tid];
        if (tid < 64 && ((kept >> lane) & 1ull)) keep[run + __popcll(kept & ((1ull << lane) - 1ull))] = order ? order[row] : row;
        run += __popcll(kept);
    }
    for (int i = run + tid; i < M; i += 256) keep[i] = -1;
    if (tid == 0) *count = run;
}

// ---- run lengths ------------------------------------------------------------------------------------------------------------
// bit b: pixel p = x FH + 32 wy + b of the column-major order differs from pixel p - 1 (never for p = 0)
__device__ __forceinline__ uint32_t transitions(const uint32_t* __restrict__ pm, int x, int wy, int NW, int FH) {
    const uint32_t w = pm[(size_t)x * NW + wy];
    uint32_t prev;
    if (wy > 0) prev = pm[(size_t)x * NW + wy - 1] >> 31;
    else if (x > 0) prev = (pm[(size_t)(x - 1) * NW + NW - 1] >> ((FH - 1) & 31)) & 1u;
    else prev = w & 1u;
    const int nb = min(32, FH - 32 * wy);
    const uint32_t valid = nb == 32 ? 0xffffffffu : ((1u << nb) - 1u);
    return (w ^ ((w << 1) | prev)) & valid;
}

__device__ __forceinline__ const uint32_t* mask_of(const uint32_t* packed, const int32_t* index, int k, int FW, int NW) {
    return packed + (size_t)(index ? index[k] : k) * FW * NW;
}

__global__ void __launch_bounds__(256) rle_count_kernel(int FH, int FW, int NW, const uint32_t* __restrict__ packed,
                                                        const int32_t* __restrict__ index, int32_t* __restrict__ lens) {
    __shared__ int s_n;
    const uint32_t* const pm = mask_of(packed, index, blockIdx.x, FW, NW);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    int n = 0;
    for (int q = threadIdx.x; q < FW * NW; q += 256) n += __popc(transitions(pm, q / NW, q % NW, NW, FH));
    if (n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0) lens[blockIdx.x] = s_n + 1 + (int)(pm[0] & 1u);
}

__global__ void __launch_bounds__(256) rle_emit_kernel(int FH, int FW, int NW, const uint32_t* __restrict__ packed,
                                                       const int32_t* __restrict__ index, const int32_t* __restrict__ lens,
                                                       const int64_t* __restrict__ ends, int64_t capacity, int32_t* __restrict__ out) {
    __shared__ int s_w[4];
    const int k = blockIdx.x;
    const int len = lens[k];
    const int64_t off = ends[k] - len;
    if (off + len > capacity) return;                         // (the caller sees the total and comes again with room)
    const uint32_t* const pm = mask_of(packed, index, k, FW, NW);
    const int lead = (int)(pm[0] & 1u);
    int32_t* const o = out + off + lead;                      // slot i: Q[i + 1] - Q[i] of Q = 0, the transitions, FH FW
    const int n = len - 1 - lead;                             // transitions
    if (lead && threadIdx.x == 0) out[off] = 0;
    int rank = 0;
    const int words = FW * NW;
    for (int q0 = 0; q0 < words; q0 += 256) {
        const int q = q0 + threadIdx.x;
        const int x = q / NW, wy = q - x * NW;
        uint32_t tw = q < words ? transitions(pm, x, wy, NW, FH) : 0u;
        int total;
        int at = rank + block_scan((int)__popc(tw), s_w, total);
        for (; tw; tw &= tw - 1u) {
            if (at < n) o[at] = x * FH + 32 * wy + (int)__builtin_ctz(tw);       // (at < n always: the bound guards the store)
            at++;
        }
        rank += total;
    }
    if (threadIdx.x == 0) o[n] = FH * FW;
    __syncthreads();
    // positions -> differences, from the top down: a chunk reads below itself only what no chunk has rewritten yet
    for (int hi = n + 1; hi > 0; hi -= 256) {
        const int i = hi - 1 - (int)threadIdx.x;
        int cur = 0, prev = 0;
        if (i >= 0) {
            cur = o[i];
            prev = i > 0 ? o[i - 1] : 0;
        }
        __syncthreads();
        if (i >= 0) o[i] = cur - prev;
    }
}

__global__ void __launch_bounds__(256) unpack_kernel(size_t total, int FH, int FW, int NW, const uint32_t* __restrict__ packed,
                                                     const int32_t* __restrict__ index, unsigned char* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % FW);
        const size_t r = i / FW;
        const int y = (int)(r % FH), k = (int)(r / FH);
        out[i] = (mask_of(packed, index, k, FW, NW)[(size_t)x * NW + (y >> 5)] >> (y & 31)) & 1u;
    }
}

// The painter's picture of K masks (show_anns): per pixel the largest j whose mask has the bit set, -1 without one.  A workgroup
// takes IM_COLS columns x IM_WORDS words of a column (32 rows each); a thread owns one word position, walks the masks from the
// last one down, four words in flight, and paints each bit the first time it meets it into the LDS tile, which is then stored
// by rows.  The words of a column are consecutive (IM_WORDS x 4 bytes per column and mask are read together), the stores are
// rows of IM_COLS x 4 bytes.
constexpr int IM_COLS = 32, IM_WORDS = 8, IM_ROWS = 32 * IM_WORDS, IM_PITCH = IM_COLS + 1;

__global__ void __launch_bounds__(256) instance_map_kernel(int K, int FH, int FW, int NW, int tiles_x, const uint32_t* __restrict__ packed,
                                                           const int32_t* __restrict__ index, int32_t* __restrict__ out) {
    __shared__ int32_t tile[IM_ROWS * IM_PITCH];
    const int x0 = (int)(blockIdx.x % tiles_x) * IM_COLS, w0 = (int)(blockIdx.x / tiles_x) * IM_WORDS;
    const int wl = threadIdx.x % IM_WORDS, xl = threadIdx.x / IM_WORDS;
    const int x = x0 + xl, wy = w0 + wl;
    int32_t* const mine = tile + (wl * 32) * IM_PITCH + xl;           // bit b of this thread's word: mine[b * IM_PITCH]
#pragma unroll
    for (int b = 0; b < 32; b++) mine[b * IM_PITCH] = -1;
    if (x < FW && wy < NW) {
        const size_t at = (size_t)x * NW + wy;
        uint32_t open = ~0u;                                          // bits no mask has painted yet
        auto paint = [&](uint32_t w, int j) {
            for (uint32_t t = w & open; t; t &= t - 1u) mine[(int)__builtin_ctz(t) * IM_PITCH] = j;
            open &= ~w;
        };
        int j = K - 1;
        for (; j >= 3 && open; j -= 4) {
            const uint32_t a = mask_of(packed, index, j, FW, NW)[at], b = mask_of(packed, index, j - 1, FW, NW)[at];
            const uint32_t c = mask_of(packed, index, j - 2, FW, NW)[at], d = mask_of(packed, index, j - 3, FW, NW)[at];
            paint(a, j); paint(b, j - 1); paint(c, j - 2); paint(d, j - 3);
        }
        for (; j >= 0 && open; j--) paint(mask_of(packed, index, j, FW, NW)[at], j);
    }
    __syncthreads();
    const int cx = threadIdx.x % IM_COLS;
    for (int r = threadIdx.x / IM_COLS; r < IM_ROWS; r += 256 / IM_COLS) {
        const int y = w0 * 32 + r;
        if (y < FH && x0 + cx < FW) out[(size_t)y * FW + x0 + cx] = tile[r * IM_PITCH + cx];
    }
}

int check_geometry(const char* who, int M, int h, int w, int S, int ih, int iw, int H, int W) {
    if (M < 0 || h < 1 || w < 1 || S < 1 || ih < 1 || iw < 1 || H < 1 || W < 1)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: bad sizes M=%d h=%d w=%d S=%d input=%dx%d original=%dx%d", who, M, h, w, S, ih, iw, H, W);
    if (ih > S || iw > S) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: input size %d x %d beyond img_size %d", who, ih, iw, S);
    if (M > MAX_MASKS) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: M=%d masks: up to %d per call are supported", who, M, MAX_MASKS);
    if (h > 32768 || w > 32768 || S > 32768 || H > 32768 || W > 32768)
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: sizes up to 32768 are supported", who);
    if ((size_t)M * H * W > 0x7fffffffffull) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: too large", who);
    return F3DGS_OK;
}

Geo geometry(int h, int w, int S, int ih, int iw, int H, int W) {
    return Geo{h, w, ih, iw, H, W, (float)h / (float)S, (float)w / (float)S, (float)ih / (float)H, (float)iw / (float)W};
}

int last_launch(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

int check_packed(const char* who, int K, int FH, int FW) {
    if (K < 0 || FH < 1 || FW < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: bad sizes K=%d FH=%d FW=%d", who, K, FH, FW);
    if ((size_t)FH * FW > 0x3fffffffull) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: frames of %d x %d pixels: up to 2^30 are supported", who, FH, FW);
    return F3DGS_OK;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_sam_masks_scratch_bytes(int M) {
    if (M < 1 || M > MAX_MASKS) return 0;
    return (size_t)M * RAW * sizeof(int32_t);
}

int f3dgs_sam_masks(int M, int h, int w, int S, int ih, int iw, int H, int W, int FH, int FW, int cx0, int cy0, const float* low_res,
                    const float* iou_preds, float pred_iou_thresh, float t, float t_hi, float t_lo, float stability_thresh,
                    int edge_filter, uint32_t* packed, int32_t* counts, int32_t* box, int32_t* box_frame, float* stability,
                    unsigned char* keep, int32_t* kept_index, int32_t* kept_count, void* scratch, void* stream) {
    if (const int rc = check_geometry("sam_masks", M, h, w, S, ih, iw, H, W)) return rc;
    if (FH < 1 || FW < 1 || cx0 < 0 || cy0 < 0 || (long long)cx0 + W > FW || (long long)cy0 + H > FH)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "sam_masks: the crop %d x %d at (%d, %d) does not lie in the frame %d x %d", H, W, cx0,
                             cy0, FH, FW);
    if (const int rc = check_packed("sam_masks", M, FH, FW)) return rc;
    if (!kept_count) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "sam_masks: null pointer");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Frame fr{FH, FW, (FH + 31) / 32, cx0, cy0};
    const Filter fl{stability_thresh, edge_filter != 0, {(float)cx0, (float)cy0, (float)(cx0 + W), (float)(cy0 + H)}, {0.0f, 0.0f, (float)FW, (float)FH}};
    const FinishOut fo{counts, box, box_frame, stability, keep, kept_index, kept_count};
    const float* const iou = pred_iou_thresh > 0.0f ? iou_preds : nullptr;      // (a threshold <= 0 switches the test off)
    if (M > 0) {
        if (!low_res || !packed || !counts || !box || !box_frame || !stability || !keep || !kept_index || !scratch)
            return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "sam_masks: null pointer");
        int32_t* const raw = static_cast<int32_t*>(scratch);
        hipLaunchKernelGGL(sam_init_kernel, dim3((M * RAW + 255) / 256), dim3(256), 0, s, M, raw);
        const int tiles_x = (FW + TS - 1) / TS, tiles_y = (FH + TS - 1) / TS;
        hipLaunchKernelGGL(sam_pass_kernel<0>, dim3(tiles_x * tiles_y, M), dim3(256), 0, s, geometry(h, w, S, ih, iw, H, W), fr, tiles_x, low_res,
                           iou, pred_iou_thresh, t, t_hi, t_lo, packed, raw, (void*)nullptr);
    }
    hipLaunchKernelGGL(sam_finish_kernel, dim3(1), dim3(256), 0, s, M, static_cast<const int32_t*>(scratch), iou, pred_iou_thresh, fr, fl, fo);
    return last_launch("sam_masks");
}

int f3dgs_sam_upscale(int M, int h, int w, int S, int ih, int iw, int H, int W, const float* low_res, float t, int out_bool, void* out,
                      void* stream) {
    if (const int rc = check_geometry("sam_upscale", M, h, w, S, ih, iw, H, W)) return rc;
    if (M == 0) return F3DGS_OK;
    if (!low_res || !out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "sam_upscale: null pointer");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const Frame fr{H, W, (H + 31) / 32, 0, 0};
    const int tiles_x = (W + TS - 1) / TS, tiles_y = (H + TS - 1) / TS;
    const dim3 grid(tiles_x * tiles_y, M);
    const Geo g = geometry(h, w, S, ih, iw, H, W);
    if (out_bool)
        hipLaunchKernelGGL(sam_pass_kernel<2>, grid, dim3(256), 0, s, g, fr, tiles_x, low_res, (const float*)nullptr, 0.0f, t, t, t,
                           (uint32_t*)nullptr, (int32_t*)nullptr, out);
    else
        hipLaunchKernelGGL(sam_pass_kernel<1>, grid, dim3(256), 0, s, g, fr, tiles_x, low_res, (const float*)nullptr, 0.0f, t, t, t,
                           (uint32_t*)nullptr, (int32_t*)nullptr, out);
    return last_launch("sam_upscale");
}

size_t f3dgs_box_nms_scratch_bytes(int M) {
    if (M < 1 || M > NMS_MAX) return 0;
    const size_t W64 = ((size_t)M + 63) / 64;
    return (size_t)M * W64 * sizeof(unsigned long long);
}

int f3dgs_box_nms(int M, const float* boxes, const int32_t* categories, float iou_threshold, const int32_t* order, int32_t* keep,
                  int32_t* count, void* scratch, void* stream) {
    if (M < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "box_nms: M=%d", M);
    if (M > NMS_MAX) return report_errorf(F3DGS_ERR_UNSUPPORTED, "box_nms: M=%d boxes: up to %d are supported", M, NMS_MAX);
    if (!count || (M > 0 && (!boxes || !keep || !scratch))) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "box_nms: null pointer");
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int W64 = (M + 63) / 64;
    unsigned long long* const mat = static_cast<unsigned long long*>(scratch);
    if (M > 0) hipLaunchKernelGGL(nms_matrix_kernel, dim3(W64, W64), dim3(64), 0, s, M, W64, boxes, categories, iou_threshold, mat);
    hipLaunchKernelGGL(nms_sweep_kernel, dim3(1), dim3(256), 0, s, M, W64, mat, order, keep, count);
    return last_launch("box_nms");
}

int f3dgs_mask_rle_count(int K, int FH, int FW, const uint32_t* packed, const int32_t* index, int32_t* lens, void* stream) {
    if (const int rc = check_packed("mask_rle_count", K, FH, FW)) return rc;
    if (K == 0) return F3DGS_OK;
    if (!packed || !lens) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_rle_count: null pointer");
    hipLaunchKernelGGL(rle_count_kernel, dim3(K), dim3(256), 0, static_cast<hipStream_t>(stream), FH, FW, (FH + 31) / 32, packed, index, lens);
    return last_launch("mask_rle_count");
}

int f3dgs_mask_rle_emit(int K, int FH, int FW, const uint32_t* packed, const int32_t* index, const int32_t* lens, const int64_t* ends,
                        int64_t capacity, int32_t* out, void* stream) {
    if (const int rc = check_packed("mask_rle_emit", K, FH, FW)) return rc;
    if (capacity < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_rle_emit: capacity %lld", (long long)capacity);
    if (K == 0) return F3DGS_OK;
    if (!packed || !lens || !ends || !out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_rle_emit: null pointer");
    hipLaunchKernelGGL(rle_emit_kernel, dim3(K), dim3(256), 0, static_cast<hipStream_t>(stream), FH, FW, (FH + 31) / 32, packed, index, lens,
                       ends, capacity, out);
    return last_launch("mask_rle_emit");
}

int f3dgs_mask_unpack(int K, int FH, int FW, const uint32_t* packed, const int32_t* index, unsigned char* out, void* stream) {
    if (const int rc = check_packed("mask_unpack", K, FH, FW)) return rc;
    if (K == 0) return F3DGS_OK;
    if (!packed || !out) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_unpack: null pointer");
    const size_t total = (size_t)K * FH * FW;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(unpack_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), total, FH, FW, (FH + 31) / 32, packed, index, out);
    return last_launch("mask_unpack");
}

int f3dgs_mask_instance_map(int K, int FH, int FW, const uint32_t* packed, const int32_t* index, int32_t* out, void* stream) {
    if (const int rc = check_packed("mask_instance_map", K, FH, FW)) return rc;
    if (!out || (K > 0 && !packed)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "mask_instance_map: null pointer");
    const int NW = (FH + 31) / 32, tiles_x = (FW + IM_COLS - 1) / IM_COLS, tiles_y = (NW + IM_WORDS - 1) / IM_WORDS;
    hipLaunchKernelGGL(instance_map_kernel, dim3(tiles_x * tiles_y), dim3(256), 0, static_cast<hipStream_t>(stream), K, FH, FW, NW, tiles_x,
                       packed, index, out);
    return last_launch("mask_instance_map");
}

}  // extern "C"
