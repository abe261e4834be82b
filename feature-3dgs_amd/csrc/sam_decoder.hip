// sam_decoder.hip - SAM's prompt encoder and mask decoder, forward only (include/f3dgs.h: f3dgs_sam_decoder_*).
//
// From a rendered 256-channel feature map and point / box prompts to the decoder's low-resolution logits and IoU predictions:
// the step between the rasterizer's feature map and sam_masks.hip.  Exactly SAM's decoder: width 256, depth 2, 8 heads, MLP
// 2048, 4 mask tokens + 1 IoU token, a 4x upscaler (two 2x2 stride-2 transposed convolutions) and hypernetwork heads.
//
// Numeric contract.  fp32 in, fp32 out.  Every contraction over a weight matrix runs on v_mfma_f32_32x32x2_f32 (exact fp32
// products, one accumulation chain per output element, the instruction's own order).  An output element's chain is a function
// of its own row of X and of W alone: which other rows share its 32-row tile moves nothing.  No atomics; every reduction (the
// LayerNorms' butterfly sums, the softmax sums, the combine over chunks of image tokens) has a fixed order.  A prompt's
// outputs are therefore the same bits at every batch size and every position in the batch.
//
// K index of a matrix step.  As in decoder_tile.h, lane (r = l & 31, h = l >> 5) contracts k = h KC/2 + s in step s of a
// KC-wide chunk (any bijection of K works as long as both operands use it).  The weights are packed for it once
// (f3dgs_sam_decoder_pack_weights): Wp[k / 4][n][k % 4], so that one 16-byte load feeds four steps of an output column.
//
// Kernels.
//   plan (once per feature map)   sd_src_kernel: src0 = features^T + no_mask_embed and the dense positional encoding, both
//                                 token-major; then three sd_lin_kernel launches: layer 0's K0, V0 (token -> image) and Q0
//                                 (image -> token), which are the same for every prompt of the image.
//   token side                    sd_tokens_kernel (prompt encoding), sd_lin_kernel (row-tiled linear over all B T rows with
//                                 bias / ReLU / residual / LayerNorm epilogues), sd_self_attn_kernel (<= 16 tokens).
//   token -> image attention      sd_t2i_kernel per (prompt, chunk of 256 image tokens): projects a 32-token tile of the prompt's
//                                 keys to K and V on the matrix pipe (layer 0: reads K0 / V0), scores it against the prompt's
//                                 queries and keeps a running max / sum / accumulator; sd_t2i_combine_kernel joins the chunks
//                                 in chunk order.  The per-prompt (hw, 128) K and V never exist in memory.
//   image -> token block          sd_i2t_kernel per (prompt, 32-token tile): q projection (layer 0: Q0), softmax over the
//                                 prompt's tokens, attn V, out_proj, + keys, LayerNorm; writes the prompt's new keys tile.
//   upscale and masks             sd_upscale_kernel per (prompt, 32-token tile): both transposed convolutions, LayerNorm2d, the
//                                 GELUs and the products with the prompt's hypernetwork vectors; each image token gives a 4x4
//                                 block of logits per requested mask, stored straight into low_res.  The 64- and 32-channel
//                                 upscaled maps never exist in memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "common.h"
#include "decoder_tile.h"

namespace f3dgs {

namespace {

constexpr int D = 256;            // transformer width
constexpr int DI = 128;           // internal width of the cross attentions
constexpr int MLP = 2048;
constexpr int TMAX = F3DGS_SAM_DECODER_MAX_TOKENS;
constexpr int XS = D + 4;         // LDS row stride of a 32 x 256 tile: 16-byte aligned rows
constexpr int CHUNK = 256;        // image tokens per workgroup of the token -> image attention (8 tiles)
constexpr int PART = 18;          // floats of a partial: max, sum, 16 accumulators
constexpr float TWO_PI = 6.2831855f;       // float32(2 pi), as the reference's `2 * np.pi * coords` rounds it

// ---- the packed weights ------------------------------------------------------------------------------------------------------
struct AttnW {
    size_t q, qb, k, kb, v, vb, o, ob;
};
struct LayerW {
    AttnW self, t2i, i2t;
    size_t n1w, n1b, n2w, n2b, n3w, n3b, n4w, n4b, l1, l1b, l2, l2b;
};
struct Layout {
    size_t gauss, pt[4], nap, nomask, iou_tok, mask_tok;
    LayerW L[2];
    AttnW fin;
    size_t nfw, nfb;
    size_t c1, c1b, lnw, lnb, c2, c2b;
    size_t hyp, hyp_stride, h_w[3], h_b[3];      // hypernetwork i at hyp + i hyp_stride; h_w / h_b relative to it
    size_t i_w[3], i_b[3];
    size_t total;
};
// one source parameter: where it goes and how.  kind 0: n floats copied (zeros up to npad); 1: a Linear weight (N, K);
// 2: a ConvTranspose2d weight (K, O, 2, 2) as the (K, 4 O) matrix of column n = (2 a + b) O + o
struct Item {
    size_t dst;
    int kind, K, N, npad;
};

struct Builder {
    std::vector<Item> items;
    size_t at = 0;
    size_t take(size_t n) {
        const size_t o = at;
        at += (n + 63) / 64 * 64;            // every sub-buffer on a 256-byte boundary
        return o;
    }
    size_t vec(int n, int npad = 0) {
        npad = std::max(npad, n);
        const size_t o = take((size_t)npad);
        items.push_back({o, 0, 1, n, npad});
        return o;
    }
    size_t mat(int K, int N, int npad = 0, int kind = 1) {
        npad = std::max(npad, N);
        const size_t o = take((size_t)K * npad);
        items.push_back({o, kind, K, N, npad});
        return o;
    }
    void attn(AttnW& a, int inner) {
        a.q = mat(D, inner), a.qb = vec(inner);
        a.k = mat(D, inner), a.kb = vec(inner);
        a.v = mat(D, inner), a.vb = vec(inner);
        a.o = mat(inner, D), a.ob = vec(D);
    }
};

// the order of f3dgs_sam_decoder_pack_weights' table (include/f3dgs.h lists it)
void build_layout(Layout& L, std::vector<Item>* items) {
    Builder b;
    L.gauss = b.vec(2 * 128);
    for (int i = 0; i < 4; i++) L.pt[i] = b.vec(D);
    L.nap = b.vec(D), L.nomask = b.vec(D), L.iou_tok = b.vec(D), L.mask_tok = b.vec(4 * D);
    for (int l = 0; l < 2; l++) {
        LayerW& w = L.L[l];
        b.attn(w.self, D);
        w.n1w = b.vec(D), w.n1b = b.vec(D);
        b.attn(w.t2i, DI);
        w.n2w = b.vec(D), w.n2b = b.vec(D);
        w.l1 = b.mat(D, MLP), w.l1b = b.vec(MLP), w.l2 = b.mat(MLP, D), w.l2b = b.vec(D);
        w.n3w = b.vec(D), w.n3b = b.vec(D);
        w.n4w = b.vec(D), w.n4b = b.vec(D);
        b.attn(w.i2t, DI);
    }
    b.attn(L.fin, DI);
    L.nfw = b.vec(D), L.nfb = b.vec(D);
    L.c1 = b.mat(D, 4 * 64, 0, 2), L.c1b = b.vec(64);
    L.lnw = b.vec(64), L.lnb = b.vec(64);
    L.c2 = b.mat(64, 4 * 32, 0, 2), L.c2b = b.vec(32);
    L.hyp = b.at;
    for (int i = 0; i < 4; i++) {
        const size_t base = b.at;
        const size_t w0 = b.mat(D, D), b0 = b.vec(D), w1 = b.mat(D, D), b1 = b.vec(D), w2 = b.mat(D, 32), b2 = b.vec(32);
        if (i == 0) {
            L.h_w[0] = w0 - base, L.h_b[0] = b0 - base, L.h_w[1] = w1 - base, L.h_b[1] = b1 - base, L.h_w[2] = w2 - base, L.h_b[2] = b2 - base;
        }
        L.hyp_stride = b.at - base;
    }
    L.i_w[0] = b.mat(D, D), L.i_b[0] = b.vec(D), L.i_w[1] = b.mat(D, D), L.i_b[1] = b.vec(D);
    L.i_w[2] = b.mat(D, 4, 32), L.i_b[2] = b.vec(4, 32);       // four outputs in a 32-column block of zeros
    L.total = b.at;
    if (items) *items = std::move(b.items);
}

const Layout& layout() {
    static const Layout L = [] {
        Layout l{};
        build_layout(l, nullptr);
        return l;
    }();
    return L;
}

__global__ void __launch_bounds__(256) sd_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int kind, int K, int N, int npad) {
    const size_t n_all = (size_t)K * npad;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_all) return;
    if (kind == 0) {
        dst[e] = e < (size_t)N ? src[e] : 0.f;
        return;
    }
    const int k = (int)((e >> 2) / npad) * 4 + (int)(e & 3), n = (int)((e >> 2) % npad);
    float v = 0.f;
    if (n < N) {
        if (kind == 1) {
            v = src[(size_t)n * K + k];
        } else {
            const int O = N / 4, s = n / O, o = n - s * O;
            v = src[((size_t)k * O + o) * 4 + s];
        }
    }
    dst[e] = v;
}

// ---- the matrix step ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; i++) z[i] = 0.f;
    return z;
}

// acc += Xs[32 x KC] (LDS, row stride XS) . W[k0 .. k0 + KC)[column block] for this wave's column `col` (= block + (lane & 31)).
// Four chains per output element (steps 4 s, 4 s + 1, 4 s + 2, 4 s + 3), joined as (c0 + c1) + (c2 + c3): a quarter of the
// rounding steps of one chain, and four independent matrix instructions in flight.  The chains start at zero whatever `acc`
// holds: a K above 256 is summed chunk by chunk.
template <int KC>
__device__ __forceinline__ void mm(f32x16& acc, const float* Xs, const float* __restrict__ Wp, int k0, int npad, int col, int r, int h) {
    const float* xrow = Xs + r * XS + h * (KC >> 1);
    const float4* w = reinterpret_cast<const float4*>(Wp) + (size_t)((k0 + h * (KC >> 1)) >> 2) * npad + col;
    constexpr int steps = KC >> 3;
    f32x16 c0 = zero16(), c1 = zero16(), c2 = zero16(), c3 = zero16();
#pragma unroll 4
    for (int s4 = 0; s4 < steps; s4++) {
        const float4 a = *reinterpret_cast<const float4*>(xrow + 4 * s4);
        const float4 b = w[(size_t)s4 * npad];
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c1, 0, 0, 0);
        c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c2, 0, 0, 0);
        c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c3, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] += (c0[i] + c1[i]) + (c2[i] + c3[i]);
}
// two column blocks per wave (col and col + 128), one after the other: the eight chains of both at once would leave one wave per
// SIMD, and the X operand is an LDS read per four matrix steps
template <int KC>
__device__ __forceinline__ void mm2(f32x16& acc0, f32x16& acc1, const float* Xs, const float* __restrict__ Wp, int k0, int npad, int col, int r,
                                    int h) {
    mm<KC>(acc0, Xs, Wp, k0, npad, col, r, h);
    mm<KC>(acc1, Xs, Wp, k0, npad, col + 128, r, h);
}

// rows w 8 .. w 8 + 7 of the 32 x 256 tile in Ts: LayerNorm (biased variance, two passes, butterfly sums), stored to Y
__device__ __forceinline__ void layer_norm_rows(const float* Ts, int w, int lane, const float* __restrict__ lnw, const float* __restrict__ lnb, float eps,
                                                float* __restrict__ Y, size_t ldy, int row0, int M) {
    const float4 g = *reinterpret_cast<const float4*>(lnw + lane * 4), bb = *reinterpret_cast<const float4*>(lnb + lane * 4);
    for (int i = 0; i < 8; i++) {
        const int row = w * 8 + i;
        const float4 x = *reinterpret_cast<const float4*>(Ts + row * XS + lane * 4);
        const float mean = wave_sum((x.x + x.y) + (x.z + x.w)) * (1.f / D);
        const float dx = x.x - mean, dy = x.y - mean, dz = x.z - mean, dw = x.w - mean;
        const float var = wave_sum((dx * dx + dy * dy) + (dz * dz + dw * dw)) * (1.f / D);
        const float rs = 1.f / sqrtf(var + eps);
        if (row0 + row < M) {
            float4 y;
            y.x = dx * rs * g.x + bb.x, y.y = dy * rs * g.y + bb.y, y.z = dz * rs * g.z + bb.z, y.w = dw * rs * g.w + bb.w;
            *reinterpret_cast<float4*>(Y + (size_t)(row0 + row) * ldy + lane * 4) = y;
        }
    }
}

// 32 rows x KC columns of X (+ X2) from row0 / column k0 into Xs; rows past M as zeros
__device__ __forceinline__ void stage_rows(float* Xs, const float* __restrict__ X, const float* __restrict__ X2, size_t ldx, int row0, int M, int k0, int KC) {
    const int per_row = KC >> 2;
    for (int e = threadIdx.x; e < 32 * per_row; e += 256) {
        const int row = e / per_row, c = (e - row * per_row) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + row < M) {
            v = *reinterpret_cast<const float4*>(X + (size_t)(row0 + row) * ldx + k0 + c);
            if (X2) {
                const float4 u = *reinterpret_cast<const float4*>(X2 + (size_t)(row0 + row) * ldx + k0 + c);
                v.x += u.x, v.y += u.y, v.z += u.z, v.w += u.w;
            }
        }
        *reinterpret_cast<float4*>(Xs + row * XS + c) = v;
    }
}

// ---- the row-tiled linear ----------------------------------------------------------------------------------------------------
// Y[M x N] = act((X [+ X2]) Wp + bias) [+ R], optionally LayerNorm over the 256 columns.  Workgroup = 32 rows x 256 columns
// (blockIdx.y: further column groups, blockIdx.z: independent problems at the z strides).  Columns [col_first, col_first +
// col_count) are stored, at Y[row][col - col_first].
struct LinArgs {
    const float* X;
    const float* X2;
    size_t ldx;
    const float* W;
    const float* bias;
    const float* R;
    size_t ldr;
    const float* lnw;
    const float* lnb;
    float eps;
    float* Y;
    size_t ldy;
    int M, K, npad, relu, col_first, col_count;
    size_t xz, wz, bz, yz;
};

__global__ void __launch_bounds__(256, 2) sd_lin_kernel(LinArgs a) {
    __shared__ __attribute__((aligned(16))) float Xs[32 * XS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int row0 = blockIdx.x * 32, z = blockIdx.z;
    const float* X = a.X + z * a.xz;
    const float* W = a.W + z * a.wz;
    const float* bias = a.bias + z * a.bz;
    float* Y = a.Y + z * a.yz;
    const int col0 = blockIdx.y * 256 + w * 32, col1 = col0 + 128;
    const bool v0 = col0 < a.npad, v1 = col1 < a.npad;
    f32x16 acc0 = zero16(), acc1 = zero16();
    const int KC = a.K < 256 ? a.K : 256;
    for (int k0 = 0; k0 < a.K; k0 += KC) {
        stage_rows(Xs, X, a.X2, a.ldx, row0, a.M, k0, KC);
        __syncthreads();
        if (KC == 256) {
            if (v1) mm2<256>(acc0, acc1, Xs, W, k0, a.npad, col0 + r, r, h);
            else if (v0) mm<256>(acc0, Xs, W, k0, a.npad, col0 + r, r, h);
        } else {                                  // K = 128
            if (v1) mm2<128>(acc0, acc1, Xs, W, k0, a.npad, col0 + r, r, h);
            else if (v0) mm<128>(acc0, Xs, W, k0, a.npad, col0 + r, r, h);
        }
        __syncthreads();
    }
    if (a.lnw) {                                  // npad == 256: the whole row lies in this workgroup
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int row = mfma_row(i, h);
            const bool ok = row0 + row < a.M;
            float y0 = acc0[i] + bias[col0 + r], y1 = acc1[i] + bias[col1 + r];
            if (a.R && ok) y0 += a.R[(size_t)(row0 + row) * a.ldr + col0 + r], y1 += a.R[(size_t)(row0 + row) * a.ldr + col1 + r];
            Xs[row * XS + col0 + r] = y0, Xs[row * XS + col1 + r] = y1;
        }
        __syncthreads();
        layer_norm_rows(Xs, w, lane, a.lnw, a.lnb, a.eps, Y, a.ldy, row0, a.M);
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int row = row0 + mfma_row(i, h);
        if (row >= a.M) continue;
        if (v0) {
            const int c = col0 + r;
            float y = acc0[i] + bias[c];
            if (a.relu) y = fmaxf(y, 0.f);
            if (a.R) y += a.R[(size_t)row * a.ldr + c];
            if (c >= a.col_first && c < a.col_first + a.col_count) Y[(size_t)row * a.ldy + c - a.col_first] = y;
        }
        if (v1) {
            const int c = col1 + r;
            float y = acc1[i] + bias[c];
            if (a.relu) y = fmaxf(y, 0.f);
            if (a.R) y += a.R[(size_t)row * a.ldr + c];
            if (c >= a.col_first && c < a.col_first + a.col_count) Y[(size_t)row * a.ldy + c - a.col_first] = y;
        }
    }
}

// ---- positional encoding -----------------------------------------------------------------------------------------------------
// the reference's _pe_encoding of a point (x, y) in [0, 1]^2, frequency c: the angle whose sine and cosine are the embedding
__device__ __forceinline__ float pe_angle(float x, float y, const float* __restrict__ gauss, int c) {
    const float cx = 2.f * x - 1.f, cy = 2.f * y - 1.f;
    return TWO_PI * fmaf(cy, gauss[128 + c], cx * gauss[c]);
}

// plan: src0[t][c] = features[c][t] + no_mask_embed[c] and pe[t][:], 32 tokens per workgroup (transposed through LDS)
__global__ void __launch_bounds__(256) sd_src_kernel(int h, int w, const float* __restrict__ feat, int64_t sc, int64_t sy, int64_t sx,
                                                     const float* __restrict__ wts, size_t nomask, size_t gauss, float* __restrict__ src0,
                                                     float* __restrict__ pe) {
    __shared__ float Ts[32 * (D + 1)];
    const int hw = h * w, t0 = blockIdx.x * 32;
    const int tl = threadIdx.x & 31, cg = threadIdx.x >> 5;
    const int t = t0 + tl;
    if (t < hw) {
        const int i = t / w, j = t - i * w;
        const float* f = feat + (int64_t)i * sy + (int64_t)j * sx;
        for (int c = cg; c < D; c += 8) Ts[tl * (D + 1) + c] = f[(int64_t)c * sc] + wts[nomask + c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * D; e += 256) {
        const int row = e >> 8, c = e & 255;
        const int tt = t0 + row;
        if (tt >= hw) break;
        src0[(size_t)tt * D + c] = Ts[row * (D + 1) + c];
        const int i = tt / w, j = tt - i * w;
        const float ang = pe_angle(((float)j + 0.5f) / (float)w, ((float)i + 0.5f) / (float)h, wts + gauss, c & 127);
        pe[(size_t)tt * D + c] = c < 128 ? sinf(ang) : cosf(ang);
    }
}

// the tokens of every prompt: [iou, mask0..3, points..., pad point if no box, box corner 0, box corner 1]; one workgroup per row
__global__ void __launch_bounds__(256) sd_tokens_kernel(int T, int n_points, const float* __restrict__ coords, const int32_t* __restrict__ labels,
                                                        const float* __restrict__ boxes, float in_h, float in_w, const float* __restrict__ wts,
                                                        Layout L, float* __restrict__ tok) {
    const int b = blockIdx.x / T, t = blockIdx.x - b * T, c = threadIdx.x;
    float v;
    if (t == 0) {
        v = wts[L.iou_tok + c];
    } else if (t < 5) {
        v = wts[L.mask_tok + (t - 1) * D + c];
    } else {
        const int p = t - 5;
        float px, py;
        int label;
        if (p < n_points) {
            px = coords[((size_t)b * n_points + p) * 2], py = coords[((size_t)b * n_points + p) * 2 + 1];
            label = labels[(size_t)b * n_points + p];
        } else if (!boxes) {
            px = py = 0.f, label = -1;                                  // the pad point
        } else {
            const int corner = p - n_points;
            px = boxes[(size_t)b * 4 + corner * 2], py = boxes[(size_t)b * 4 + corner * 2 + 1];
            label = 2 + corner;
        }
        if (label == -1) {
            v = wts[L.nap + c];
        } else {
            const float ang = pe_angle((px + 0.5f) / in_w, (py + 0.5f) / in_h, wts + L.gauss, c & 127);
            v = c < 128 ? sinf(ang) : cosf(ang);
            if (label >= 0 && label < 4) v += wts[L.pt[label] + c];
        }
    }
    tok[(size_t)blockIdx.x * D + c] = v;
}

// ---- self attention over the <= 16 tokens of a prompt: 8 heads of 32; thread = (token, head) ---------------------------------
__global__ void __launch_bounds__(128) sd_self_attn_kernel(int T, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           float* __restrict__ out) {
    const int b = blockIdx.x, t = threadIdx.x >> 3, hd = threadIdx.x & 7;
    if (t >= T) return;
    const size_t base = (size_t)b * T * D + hd * 32;
    float qr[32];
#pragma unroll
    for (int c = 0; c < 32; c += 4) {
        const float4 x = *reinterpret_cast<const float4*>(q + base + (size_t)t * D + c);
        qr[c] = x.x, qr[c + 1] = x.y, qr[c + 2] = x.z, qr[c + 3] = x.w;
    }
    float s[TMAX];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < TMAX; j++) {
        s[j] = -INFINITY;
        if (j < T) {
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < 32; c += 4) {
                const float4 x = *reinterpret_cast<const float4*>(k + base + (size_t)j * D + c);
                d = fmaf(qr[c], x.x, d), d = fmaf(qr[c + 1], x.y, d), d = fmaf(qr[c + 2], x.z, d), d = fmaf(qr[c + 3], x.w, d);
            }
            s[j] = d / 5.656854249492381f;          // sqrt(32)
            m = fmaxf(m, s[j]);
        }
    }
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < TMAX; j++) {
        s[j] = j < T ? expf(s[j] - m) : 0.f;
        l += s[j];
    }
    float o[32];
#pragma unroll
    for (int c = 0; c < 32; c++) o[c] = 0.f;
#pragma unroll
    for (int j = 0; j < TMAX; j++) {
        if (j < T) {
            const float p = s[j] / l;
#pragma unroll
            for (int c = 0; c < 32; c += 4) {
                const float4 x = *reinterpret_cast<const float4*>(v + base + (size_t)j * D + c);
                o[c] = fmaf(p, x.x, o[c]), o[c + 1] = fmaf(p, x.y, o[c + 1]), o[c + 2] = fmaf(p, x.z, o[c + 2]), o[c + 3] = fmaf(p, x.w, o[c + 3]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 32; c += 4) *reinterpret_cast<float4*>(out + base + (size_t)t * D + c) = make_float4(o[c], o[c + 1], o[c + 2], o[c + 3]);
}

// ---- token -> image attention ------------------------------------------------------------------------------------------------
struct T2IArgs {
    const float* keys;       // (B, hw, 256) the prompts' keys, or null: layer 0, K0 / V0 of the plan
    const float* pe;
    const float* K0;
    const float* V0;
    const float* wk;
    const float* bk;
    const float* wv;
    const float* bv;
    const float* q;          // (B T, 128)
    float* part;             // (B, nch, 128, PART)
    int T, hw, nch;
};

__global__ void __launch_bounds__(256, 2) sd_t2i_kernel(T2IArgs a) {
    __shared__ __attribute__((aligned(16))) float buf[32 * XS];       // the X tile; then Ks = buf, Vs = buf + 32 * 128
    float* const Ks = buf;
    float* const Vs = buf + 32 * DI;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, chunk = blockIdx.x;
    // two threads per (token, head): each scores its half of a tile's rows (16) against the tile's common maximum, so that the
    // two running sums stay on one scale and are added at the end
    const int p = threadIdx.x >> 1, half = threadIdx.x & 1, t = p >> 3, hd = p & 7;
    const bool active = t < a.T;
    float qr[16], acc[16];
#pragma unroll
    for (int c = 0; c < 16; c++) qr[c] = 0.f, acc[c] = 0.f;
    if (active) {
#pragma unroll
        for (int c = 0; c < 16; c += 4) {
            const float4 x = *reinterpret_cast<const float4*>(a.q + ((size_t)b * a.T + t) * DI + hd * 16 + c);
            qr[c] = x.x, qr[c + 1] = x.y, qr[c + 2] = x.z, qr[c + 3] = x.w;
        }
    }
    float m = -INFINITY, l = 0.f;
    for (int tile = 0; tile < CHUNK / 32; tile++) {
        const int t0 = chunk * CHUNK + tile * 32;
        if (t0 >= a.hw) break;
        const int nv = min(32, a.hw - t0);
        if (a.keys) {
            const float* kb = a.keys + (size_t)b * a.hw * D;
            stage_rows(buf, kb, a.pe, D, t0, a.hw, 0, D);             // keys + pe
            __syncthreads();
            f32x16 ak = zero16(), av = zero16();
            mm<D>(ak, buf, a.wk, 0, DI, w * 32 + r, r, h);
            __syncthreads();
            stage_rows(buf, kb, nullptr, D, t0, a.hw, 0, D);          // keys
            __syncthreads();
            mm<D>(av, buf, a.wv, 0, DI, w * 32 + r, r, h);
            __syncthreads();
            const float bkc = a.bk[w * 32 + r], bvc = a.bv[w * 32 + r];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int row = mfma_row(i, h);
                Ks[row * DI + w * 32 + r] = ak[i] + bkc;
                Vs[row * DI + w * 32 + r] = av[i] + bvc;
            }
        } else {
            for (int e = threadIdx.x; e < 32 * (DI / 4); e += 256) {
                const int row = e >> 5, c = (e & 31) * 4;
                float4 kk = make_float4(0.f, 0.f, 0.f, 0.f), vv = kk;
                if (row < nv) {
                    kk = *reinterpret_cast<const float4*>(a.K0 + (size_t)(t0 + row) * DI + c);
                    vv = *reinterpret_cast<const float4*>(a.V0 + (size_t)(t0 + row) * DI + c);
                }
                *reinterpret_cast<float4*>(Ks + row * DI + c) = kk;
                *reinterpret_cast<float4*>(Vs + row * DI + c) = vv;
            }
        }
        __syncthreads();
        {
            float s[16];
            float tmax = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < 16; jj++) {
                const int j = half * 16 + jj;
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < 16; c += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(Ks + j * DI + hd * 16 + c);
                    d = fmaf(qr[c], x.x, d), d = fmaf(qr[c + 1], x.y, d), d = fmaf(qr[c + 2], x.z, d), d = fmaf(qr[c + 3], x.w, d);
                }
                s[jj] = j < nv ? d * 0.25f : -INFINITY;               // / sqrt(16)
                tmax = fmaxf(tmax, s[jj]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 1, 64));              // row 0 of the tile exists: finite in half 0
            const float mn = fmaxf(m, tmax);
            const float sc = expf(m - mn);                            // the first tile: exp(-inf) = 0
            l *= sc;
#pragma unroll
            for (int c = 0; c < 16; c++) acc[c] *= sc;
#pragma unroll
            for (int jj = 0; jj < 16; jj++) {
                const int j = half * 16 + jj;
                const float pj = j < nv ? expf(s[jj] - mn) : 0.f;
                l += pj;
#pragma unroll
                for (int c = 0; c < 16; c += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(Vs + j * DI + hd * 16 + c);
                    acc[c] = fmaf(pj, x.x, acc[c]), acc[c + 1] = fmaf(pj, x.y, acc[c + 1]), acc[c + 2] = fmaf(pj, x.z, acc[c + 2]),
                    acc[c + 3] = fmaf(pj, x.w, acc[c + 3]);
                }
            }
            m = mn;
        }
        __syncthreads();
    }
    l += __shfl_xor(l, 1, 64);
#pragma unroll
    for (int c = 0; c < 16; c++) acc[c] += __shfl_xor(acc[c], 1, 64);
    if (active && half == 0) {
        float* o = a.part + (((size_t)b * a.nch + chunk) * 128 + p) * PART;
        o[0] = m, o[1] = l;
#pragma unroll
        for (int c = 0; c < 16; c++) o[2 + c] = acc[c];
    }
}

// the chunks of a (prompt, token, head) in chunk order: out (B T, 128)
__global__ void __launch_bounds__(128) sd_t2i_combine_kernel(int T, int nch, const float* __restrict__ part, float* __restrict__ out) {
    const int b = blockIdx.x, p = threadIdx.x, t = p >> 3, hd = p & 7;
    if (t >= T) return;
    const float* base = part + ((size_t)b * nch * 128 + p) * PART;
    float m = -INFINITY;
    for (int c = 0; c < nch; c++) m = fmaxf(m, base[(size_t)c * 128 * PART]);
    float l = 0.f, acc[16];
#pragma unroll
    for (int c = 0; c < 16; c++) acc[c] = 0.f;
    for (int ch = 0; ch < nch; ch++) {
        const float* o = base + (size_t)ch * 128 * PART;
        const float sc = expf(o[0] - m);
        l = fmaf(o[1], sc, l);
#pragma unroll
        for (int c = 0; c < 16; c++) acc[c] = fmaf(o[2 + c], sc, acc[c]);
    }
    float* y = out + ((size_t)b * T + t) * DI + hd * 16;
#pragma unroll
    for (int c = 0; c < 16; c++) y[c] = acc[c] / l;
}

// ---- image -> token block ----------------------------------------------------------------------------------------------------
struct I2TArgs {
    const float* keys_in;    // layer 0: src0 (bstride 0); else the prompts' keys
    size_t in_bstride;
    const float* pe;
    const float* Q0;         // layer 0: the plan's q; else null
    const float* wq;
    const float* bq;
    const float* kt;         // (B T, 128) the tokens' k and v
    const float* vt;
    const float* wo;
    const float* bo;
    const float* lnw;
    const float* lnb;
    float* keys_out;         // (B, hw, 256)
    int T, hw;
};

__global__ void __launch_bounds__(256, 2) sd_i2t_kernel(I2TArgs a) {
    __shared__ __attribute__((aligned(16))) float buf[32 * XS];       // keys + pe; then q / attn out (32 x 128 at stride XS); then the new rows
    __shared__ __attribute__((aligned(16))) float Kt[TMAX * DI];
    __shared__ __attribute__((aligned(16))) float Vt[TMAX * DI];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * 32;
    const float* kin = a.keys_in + (size_t)b * a.in_bstride;
    for (int e = threadIdx.x; e < a.T * (DI / 4); e += 256) {
        *reinterpret_cast<float4*>(Kt + e * 4) = *reinterpret_cast<const float4*>(a.kt + (size_t)b * a.T * DI + e * 4);
        *reinterpret_cast<float4*>(Vt + e * 4) = *reinterpret_cast<const float4*>(a.vt + (size_t)b * a.T * DI + e * 4);
    }
    if (a.Q0) {
        stage_rows(buf, a.Q0, nullptr, DI, t0, a.hw, 0, DI);
        __syncthreads();
    } else {
        stage_rows(buf, kin, a.pe, D, t0, a.hw, 0, D);
        __syncthreads();
        f32x16 aq = zero16();
        mm<D>(aq, buf, a.wq, 0, DI, w * 32 + r, r, h);
        __syncthreads();
        const float bq = a.bq[w * 32 + r];
#pragma unroll
        for (int i = 0; i < 16; i++) buf[mfma_row(i, h) * XS + w * 32 + r] = aq[i] + bq;
        __syncthreads();
    }
    {   // thread = (row, head): softmax over the prompt's tokens, attn V, back into its own 16 columns
        const int row = threadIdx.x >> 3, hd = threadIdx.x & 7;
        float* qp = buf + row * XS + hd * 16;
        float qr[16];
#pragma unroll
        for (int c = 0; c < 16; c += 4) {
            const float4 x = *reinterpret_cast<const float4*>(qp + c);
            qr[c] = x.x, qr[c + 1] = x.y, qr[c + 2] = x.z, qr[c + 3] = x.w;
        }
        float s[TMAX];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < TMAX; j++) {
            s[j] = -INFINITY;
            if (j < a.T) {
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < 16; c += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(Kt + j * DI + hd * 16 + c);
                    d = fmaf(qr[c], x.x, d), d = fmaf(qr[c + 1], x.y, d), d = fmaf(qr[c + 2], x.z, d), d = fmaf(qr[c + 3], x.w, d);
                }
                s[j] = d * 0.25f;
                m = fmaxf(m, s[j]);
            }
        }
        float l = 0.f;
#pragma unroll
        for (int j = 0; j < TMAX; j++) {
            s[j] = j < a.T ? expf(s[j] - m) : 0.f;
            l += s[j];
        }
        float o[16];
#pragma unroll
        for (int c = 0; c < 16; c++) o[c] = 0.f;
#pragma unroll
        for (int j = 0; j < TMAX; j++) {
            if (j < a.T) {
                const float pj = s[j] / l;
#pragma unroll
                for (int c = 0; c < 16; c += 4) {
                    const float4 x = *reinterpret_cast<const float4*>(Vt + j * DI + hd * 16 + c);
                    o[c] = fmaf(pj, x.x, o[c]), o[c + 1] = fmaf(pj, x.y, o[c + 1]), o[c + 2] = fmaf(pj, x.z, o[c + 2]), o[c + 3] = fmaf(pj, x.w, o[c + 3]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 16; c += 4) *reinterpret_cast<float4*>(qp + c) = make_float4(o[c], o[c + 1], o[c + 2], o[c + 3]);
    }
    __syncthreads();
    f32x16 y0 = zero16(), y1 = zero16();
    mm2<DI>(y0, y1, buf, a.wo, 0, D, w * 32 + r, r, h);
    __syncthreads();
    const int c0 = w * 32 + r, c1 = c0 + 128;
    const float b0 = a.bo[c0], b1 = a.bo[c1];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int row = mfma_row(i, h);
        float r0 = 0.f, r1 = 0.f;
        if (t0 + row < a.hw) r0 = kin[(size_t)(t0 + row) * D + c0], r1 = kin[(size_t)(t0 + row) * D + c1];
        buf[row * XS + c0] = r0 + (y0[i] + b0);
        buf[row * XS + c1] = r1 + (y1[i] + b1);
    }
    __syncthreads();
    layer_norm_rows(buf, w, lane, a.lnw, a.lnb, 1e-5f, a.keys_out + (size_t)b * a.hw * D, D, t0, a.hw);
}

// ---- upscale and masks -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.7071067811865476f)); }

struct UpArgs {
    const float* keys;       // (B, hw, 256)
    const float* c1;
    const float* c1b;
    const float* lnw;
    const float* lnb;
    const float* c2;
    const float* c2b;
    const float* hyp;        // (B, nm, 32)
    float* low_res;          // (B, nm, 4h, 4w)
    int h, w, nm;
};

__global__ void __launch_bounds__(256, 2) sd_upscale_kernel(UpArgs a) {
    __shared__ __attribute__((aligned(16))) float buf[32 * XS];       // the keys tile; then the first convolution's 4 x 64 outputs per token
    __shared__ __attribute__((aligned(16))) float Zs[32 * (DI + 4)];  // the second convolution's 4 x 32 outputs of one sub-position
    __shared__ __attribute__((aligned(16))) float Ls[32 * 4 * 16];    // [token][mask][y][x] logits
    __shared__ __attribute__((aligned(16))) float Hs[4 * 32];
    constexpr int ZS = DI + 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.y, t0 = blockIdx.x * 32, hw = a.h * a.w;
    if (threadIdx.x < a.nm * 32) Hs[threadIdx.x] = a.hyp[(size_t)b * a.nm * 32 + threadIdx.x];
    stage_rows(buf, a.keys + (size_t)b * hw * D, nullptr, D, t0, hw, 0, D);
    __syncthreads();
    {
        f32x16 y0 = zero16(), y1 = zero16();
        mm2<D>(y0, y1, buf, a.c1, 0, D, w * 32 + r, r, h);
        __syncthreads();
        const int c0 = w * 32 + r, c1 = c0 + 128;
        const float b0 = a.c1b[c0 & 63], b1 = a.c1b[c1 & 63];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int row = mfma_row(i, h);
            buf[row * XS + c0] = y0[i] + b0;
            buf[row * XS + c1] = y1[i] + b1;
        }
    }
    __syncthreads();
    {   // LayerNorm2d over the 64 channels of a (token, sub-position) and GELU: two threads per group
        const int g = threadIdx.x >> 1, half = threadIdx.x & 1;
        float* x = buf + (g >> 2) * XS + (g & 3) * 64 + half * 32;
        float v[32];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 32; c += 4) {
            const float4 q = *reinterpret_cast<const float4*>(x + c);
            v[c] = q.x, v[c + 1] = q.y, v[c + 2] = q.z, v[c + 3] = q.w;
            sum += (q.x + q.y) + (q.z + q.w);
        }
        sum += __shfl_xor(sum, 1, 64);
        const float mean = sum * (1.f / 64);
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < 32; c++) {
            v[c] -= mean;
            ss = fmaf(v[c], v[c], ss);
        }
        ss += __shfl_xor(ss, 1, 64);
        const float rs = 1.f / sqrtf(ss * (1.f / 64) + 1e-6f);
#pragma unroll
        for (int c = 0; c < 32; c++) x[c] = gelu(v[c] * rs * a.lnw[half * 32 + c] + a.lnb[half * 32 + c]);
    }
    __syncthreads();
    const float b2 = a.c2b[r];
    for (int s1 = 0; s1 < 4; s1++) {
        f32x16 z = zero16();
        mm<64>(z, buf + s1 * 64, a.c2, 0, DI, w * 32 + r, r, h);      // wave w: the second sub-position s2 = w
#pragma unroll
        for (int i = 0; i < 16; i++) Zs[mfma_row(i, h) * ZS + w * 32 + r] = gelu(z[i] + b2);
        __syncthreads();
        {   // thread = (token, s2, which): the masks which, which + 2
            const int pr = threadIdx.x >> 1, which = threadIdx.x & 1, row = pr >> 2, s2 = pr & 3;
            const int yo = 2 * (s1 >> 1) + (s2 >> 1), xo = 2 * (s1 & 1) + (s2 & 1);
            const float* zr = Zs + row * ZS + s2 * 32;
#pragma unroll
            for (int mm_ = 0; mm_ < 2; mm_++) {
                const int mk = which + 2 * mm_;
                if (mk < a.nm) {
                    float d = 0.f;
#pragma unroll
                    for (int c = 0; c < 32; c += 4) {
                        const float4 zz = *reinterpret_cast<const float4*>(zr + c);
                        const float4 hh = *reinterpret_cast<const float4*>(Hs + mk * 32 + c);
                        d = fmaf(hh.x, zz.x, d), d = fmaf(hh.y, zz.y, d), d = fmaf(hh.z, zz.z, d), d = fmaf(hh.w, zz.w, d);
                    }
                    Ls[((row * 4 + mk) * 4 + yo) * 4 + xo] = d;
                }
            }
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < 32 * a.nm * 4; e += 256) {
        const int yo = e & 3, mk = (e >> 2) % a.nm, row = (e >> 2) / a.nm;
        const int t = t0 + row;
        if (t >= hw) continue;
        const int i = t / a.w, j = t - i * a.w;
        const float4 v = *reinterpret_cast<const float4*>(Ls + ((row * 4 + mk) * 4 + yo) * 4);
        *reinterpret_cast<float4*>(a.low_res + (((size_t)b * a.nm + mk) * (4 * a.h) + 4 * i + yo) * (size_t)(4 * a.w) + 4 * j) = v;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
size_t up64(size_t n) { return (n + 63) / 64 * 64; }

struct PlanLayout {
    size_t src0, pe, K0, V0, Q0, total;      // in floats
};
PlanLayout plan_layout(size_t hw) {
    PlanLayout p{};
    size_t at = 0;
    p.src0 = at, at += up64(hw * D);
    p.pe = at, at += up64(hw * D);
    p.K0 = at, at += up64(hw * DI);
    p.V0 = at, at += up64(hw * DI);
    p.Q0 = at, at += up64(hw * DI);
    p.total = at;
    return p;
}

struct ScratchLayout {
    size_t tok, Q, q, k, v, att, hid, part, hyp, h1, h2, keys, total;      // in floats
};
ScratchLayout scratch_layout(size_t B, size_t hw, size_t T) {
    ScratchLayout s{};
    const size_t M = B * T, nch = (hw + CHUNK - 1) / CHUNK;
    size_t at = 0;
    s.tok = at, at += up64(M * D);
    s.Q = at, at += up64(M * D);
    s.q = at, at += up64(M * D);
    s.k = at, at += up64(M * D);
    s.v = at, at += up64(M * D);
    s.att = at, at += up64(M * D);
    s.hid = at, at += up64(M * MLP);
    s.part = at, at += up64(B * nch * 128 * PART);
    s.hyp = at, at += up64(B * 4 * 32);
    s.h1 = at, at += up64(4 * B * D);
    s.h2 = at, at += up64(4 * B * D);
    s.keys = at, at += up64(B * hw * D);
    s.total = at;
    return s;
}

LinArgs lin_args(const float* X, size_t ldx, const float* W, const float* bias, float* Y, size_t ldy, int M, int K, int npad) {
    LinArgs a{};
    a.X = X, a.ldx = ldx, a.W = W, a.bias = bias, a.Y = Y, a.ldy = ldy, a.M = M, a.K = K, a.npad = npad;
    a.col_first = 0, a.col_count = npad, a.eps = 1e-5f;
    return a;
}
void launch_lin(const LinArgs& a, int Z, hipStream_t st) {
    hipLaunchKernelGGL(sd_lin_kernel, dim3((unsigned)((a.M + 31) / 32), (unsigned)((a.npad + 255) / 256), (unsigned)Z), dim3(256), 0, st, a);
}

bool grid_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * w <= F3DGS_SAM_DECODER_MAX_GRID; }

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_sam_decoder_weights_bytes(void) { return layout().total * sizeof(float); }

int f3dgs_sam_decoder_pack_weights(const float* const* params, int n_params, float* packed, void* stream) {
    const char* who = "f3dgs_sam_decoder_pack_weights";
    if (n_params != F3DGS_SAM_DECODER_PARAMS)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: %d parameters, the table has %d", who, n_params, F3DGS_SAM_DECODER_PARAMS);
    if (!params || !packed) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (params, packed)", who);
    for (int i = 0; i < n_params; i++)
        if (!params[i]) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (parameter %d)", who, i);
    if (!aligned16(packed)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: packed must be 16-byte aligned", who);
    Layout L{};
    std::vector<Item> items;
    build_layout(L, &items);
    if ((int)items.size() != F3DGS_SAM_DECODER_PARAMS) return report_errorf(F3DGS_ERR_HIP, "%s: the table has %zu entries", who, items.size());
    const hipStream_t st = static_cast<hipStream_t>(stream);
    for (int i = 0; i < n_params; i++) {
        const Item& it = items[i];
        const size_t n = (size_t)it.K * it.npad;
        hipLaunchKernelGGL(sd_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, params[i], packed + it.dst, it.kind, it.K, it.N, it.npad);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

size_t f3dgs_sam_decoder_plan_bytes(int h, int w) {
    if (!grid_ok(h, w)) return 0;
    return plan_layout((size_t)h * w).total * sizeof(float);
}

int f3dgs_sam_decoder_plan(int C, int h, int w, const float* features, int64_t stride_c, int64_t stride_y, int64_t stride_x, const float* packed,
                           float* plan, void* stream) {
    const char* who = "f3dgs_sam_decoder_plan";
    if (C != D) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: %d channels, SAM's decoder has %d", who, C, D);
    if (h < 1 || w < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a %d x %d grid", who, h, w);
    if (!grid_ok(h, w)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: a %d x %d grid, up to %d cells are taken", who, h, w, F3DGS_SAM_DECODER_MAX_GRID);
    if (!features || !packed || !plan) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (features, packed, plan)", who);
    if (stride_c < 0 || stride_y < 0 || stride_x < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a negative stride", who);
    if (misaligned16({packed, plan})) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: packed and plan must be 16-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Layout& L = layout();
    const int hw = h * w;
    const PlanLayout P = plan_layout((size_t)hw);
    hipLaunchKernelGGL(sd_src_kernel, dim3((unsigned)((hw + 31) / 32)), dim3(256), 0, st, h, w, features, stride_c, stride_y, stride_x, packed, L.nomask,
                       L.gauss, plan + P.src0, plan + P.pe);
    LinArgs a = lin_args(plan + P.src0, D, packed + L.L[0].t2i.k, packed + L.L[0].t2i.kb, plan + P.K0, DI, hw, D, DI);
    a.X2 = plan + P.pe;
    launch_lin(a, 1, st);
    a = lin_args(plan + P.src0, D, packed + L.L[0].t2i.v, packed + L.L[0].t2i.vb, plan + P.V0, DI, hw, D, DI);
    launch_lin(a, 1, st);
    a = lin_args(plan + P.src0, D, packed + L.L[0].i2t.q, packed + L.L[0].i2t.qb, plan + P.Q0, DI, hw, D, DI);
    a.X2 = plan + P.pe;
    launch_lin(a, 1, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

size_t f3dgs_sam_decoder_scratch_bytes(int B, int h, int w, int T) {
    if (B < 0 || !grid_ok(h, w) || T < 5 || T > TMAX) return 0;
    return scratch_layout((size_t)B, (size_t)h * w, (size_t)T).total * sizeof(float);
}

int f3dgs_sam_decoder_predict(int B, int h, int w, int n_points, const float* coords, const int32_t* labels, const float* boxes, int input_h,
                              int input_w, int multimask, const float* plan, const float* packed, float* low_res, float* iou, void* scratch,
                              size_t scratch_bytes, void* stream) {
    const char* who = "f3dgs_sam_decoder_predict";
    if (B < 0 || n_points < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: B < 0 or n_points < 0", who);
    if (h < 1 || w < 1 || input_h < 1 || input_w < 1) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a %d x %d grid of a %d x %d input", who, h, w, input_h, input_w);
    if (!grid_ok(h, w)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: a %d x %d grid, up to %d cells are taken", who, h, w, F3DGS_SAM_DECODER_MAX_GRID);
    if (n_points == 0 && !boxes && B > 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: neither points nor boxes", who);
    const long long Tl = 5ll + n_points + (boxes ? 2 : (n_points > 0 ? 1 : 0));
    if (Tl > TMAX) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: %lld tokens per prompt, up to %d are taken", who, Tl, TMAX);
    if (B > 65535) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: %d prompts in one call, up to 65535 are taken", who, B);
    if (B == 0) return F3DGS_OK;
    const int T = (int)Tl;
    if (n_points > 0 && (!coords || !labels)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (coords, labels)", who);
    if (!plan || !packed || !low_res || !iou) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (plan, packed, low_res, iou)", who);
    const size_t need = f3dgs_sam_decoder_scratch_bytes(B, h, w, T);
    if (!scratch || scratch_bytes < need)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: scratch of %zu bytes, %zu are needed", who, scratch ? scratch_bytes : (size_t)0, need);
    if (misaligned16({plan, packed, low_res, scratch})) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: plan, packed, low_res and scratch must be 16-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Layout& L = layout();
    const int hw = h * w, M = B * T, nch = (hw + CHUNK - 1) / CHUNK, tiles = (hw + 31) / 32;
    const PlanLayout P = plan_layout((size_t)hw);
    const ScratchLayout S = scratch_layout((size_t)B, (size_t)hw, (size_t)T);
    float* const s = static_cast<float*>(scratch);
    float *tok = s + S.tok, *Q = s + S.Q, *q = s + S.q, *k = s + S.k, *v = s + S.v, *att = s + S.att, *hid = s + S.hid, *part = s + S.part;
    float *hyp = s + S.hyp, *h1 = s + S.h1, *h2 = s + S.h2, *keys = s + S.keys;
    const float* pe = plan + P.pe;
    auto W = [&](size_t off) { return packed + off; };

    hipLaunchKernelGGL(sd_tokens_kernel, dim3((unsigned)M), dim3(256), 0, st, T, n_points, coords, labels, boxes, (float)input_h, (float)input_w, packed, L,
                       tok);
    // Y = LayerNorm(R + X Wo + b)
    auto lin_ln = [&](const float* X, int K, size_t wo, size_t bo, const float* R, size_t lw, size_t lb) {
        LinArgs a = lin_args(X, (size_t)K, W(wo), W(bo), Q, D, M, K, D);
        a.R = R, a.ldr = D, a.lnw = W(lw), a.lnb = W(lb);
        launch_lin(a, 1, st);
    };
    auto lin_plain = [&](const float* X, const float* X2, size_t w_, size_t b_, float* Y, int N) {
        LinArgs a = lin_args(X, D, W(w_), W(b_), Y, (size_t)N, M, D, N);
        a.X2 = X2;
        launch_lin(a, 1, st);
    };
    auto t2i = [&](const AttnW& aw, bool first) {
        lin_plain(Q, tok, aw.q, aw.qb, q, DI);
        T2IArgs a{};
        a.keys = first ? nullptr : keys, a.pe = pe, a.K0 = plan + P.K0, a.V0 = plan + P.V0;
        a.wk = W(aw.k), a.bk = W(aw.kb), a.wv = W(aw.v), a.bv = W(aw.vb), a.q = q, a.part = part, a.T = T, a.hw = hw, a.nch = nch;
        hipLaunchKernelGGL(sd_t2i_kernel, dim3((unsigned)nch, (unsigned)B), dim3(256), 0, st, a);
        hipLaunchKernelGGL(sd_t2i_combine_kernel, dim3((unsigned)B), dim3(128), 0, st, T, nch, part, att);
    };
    for (int l = 0; l < 2; l++) {
        const LayerW& w_ = L.L[l];
        // self attention (layer 0: the tokens themselves, and no residual)
        const float* xin = l == 0 ? tok : Q;
        const float* xpe = l == 0 ? nullptr : tok;
        lin_plain(xin, xpe, w_.self.q, w_.self.qb, q, D);
        lin_plain(xin, xpe, w_.self.k, w_.self.kb, k, D);
        lin_plain(xin, nullptr, w_.self.v, w_.self.vb, v, D);
        hipLaunchKernelGGL(sd_self_attn_kernel, dim3((unsigned)B), dim3(128), 0, st, T, q, k, v, att);
        lin_ln(att, D, w_.self.o, w_.self.ob, l == 0 ? nullptr : Q, w_.n1w, w_.n1b);
        // tokens attend to the image
        t2i(w_.t2i, l == 0);
        lin_ln(att, DI, w_.t2i.o, w_.t2i.ob, Q, w_.n2w, w_.n2b);
        // MLP
        {
            LinArgs a = lin_args(Q, D, W(w_.l1), W(w_.l1b), hid, MLP, M, D, MLP);
            a.relu = 1;
            launch_lin(a, 1, st);
        }
        lin_ln(hid, MLP, w_.l2, w_.l2b, Q, w_.n3w, w_.n3b);
        // the image attends to the tokens
        lin_plain(Q, tok, w_.i2t.k, w_.i2t.kb, k, DI);
        lin_plain(Q, nullptr, w_.i2t.v, w_.i2t.vb, v, DI);
        I2TArgs a{};
        a.keys_in = l == 0 ? plan + P.src0 : keys, a.in_bstride = l == 0 ? 0 : (size_t)hw * D, a.pe = pe, a.Q0 = l == 0 ? plan + P.Q0 : nullptr;
        a.wq = W(w_.i2t.q), a.bq = W(w_.i2t.qb), a.kt = k, a.vt = v, a.wo = W(w_.i2t.o), a.bo = W(w_.i2t.ob), a.lnw = W(w_.n4w), a.lnb = W(w_.n4b);
        a.keys_out = keys, a.T = T, a.hw = hw;
        hipLaunchKernelGGL(sd_i2t_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, st, a);
    }
    t2i(L.fin, false);
    lin_ln(att, DI, L.fin.o, L.fin.ob, Q, L.nfw, L.nfb);
    // the heads: the requested masks' hypernetworks (blockIdx.z) and the IoU head
    const int nm = multimask ? 3 : 1, first = multimask ? 1 : 0;
    {
        const float* wb = W(L.hyp + (size_t)first * L.hyp_stride);
        LinArgs a = lin_args(Q + (size_t)(1 + first) * D, (size_t)T * D, wb + L.h_w[0], wb + L.h_b[0], h1, D, B, D, D);
        a.relu = 1, a.xz = D, a.wz = L.hyp_stride, a.bz = L.hyp_stride, a.yz = (size_t)B * D;
        launch_lin(a, nm, st);
        a = lin_args(h1, D, wb + L.h_w[1], wb + L.h_b[1], h2, D, B, D, D);
        a.relu = 1, a.xz = (size_t)B * D, a.wz = L.hyp_stride, a.bz = L.hyp_stride, a.yz = (size_t)B * D;
        launch_lin(a, nm, st);
        a = lin_args(h2, D, wb + L.h_w[2], wb + L.h_b[2], hyp, (size_t)nm * 32, B, D, 32);
        a.xz = (size_t)B * D, a.wz = L.hyp_stride, a.bz = L.hyp_stride, a.yz = 32;
        launch_lin(a, nm, st);
        a = lin_args(Q, (size_t)T * D, W(L.i_w[0]), W(L.i_b[0]), h1, D, B, D, D);
        a.relu = 1;
        launch_lin(a, 1, st);
        a = lin_args(h1, D, W(L.i_w[1]), W(L.i_b[1]), h2, D, B, D, D);
        a.relu = 1;
        launch_lin(a, 1, st);
        a = lin_args(h2, D, W(L.i_w[2]), W(L.i_b[2]), iou, (size_t)nm, B, D, 32);
        a.col_first = first, a.col_count = nm;
        launch_lin(a, 1, st);
    }
    UpArgs u{};
    u.keys = keys, u.c1 = W(L.c1), u.c1b = W(L.c1b), u.lnw = W(L.lnw), u.lnb = W(L.lnb), u.c2 = W(L.c2), u.c2b = W(L.c2b), u.hyp = hyp, u.low_res = low_res;
    u.h = h, u.w = w, u.nm = nm;
    hipLaunchKernelGGL(sd_upscale_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, st, u);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
