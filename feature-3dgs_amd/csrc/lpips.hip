// lpips.hip - LPIPS (VGG16, version 0.1) of N image pairs on the device: the reference's lpipsPyTorch (net_type 'vgg') as
// fused fp32 kernels.  include/f3dgs.h: f3dgs_lpips_*; lpips_vgg.py checks names, shapes and arguments.
//
//   z-score -> 13 x (3x3 conv, bias, ReLU), a 2x2 max-pool in front of blocks 2..5 -> five taps (relu1_2 .. relu5_3) ->
//   per tap  d_l = mean_p sum_c w_l[c] (x_c / (|x| + 1e-10) - y_c / (|y| + 1e-10))^2  ->  sum_l d_l
//
// x and y run as ONE batch of 2N images (image b < N: x_b, image N + b: y_b) through every launch: 13 convolutions, 5 tap
// launches, 1 final sum.  Activations are channel-planar (NCHW) fp32 in two ping-pong buffers of the caller's workspace.
//
// The contraction of conv1_2 .. conv5_3 is an implicit GEMM on v_mfma_f32_32x32x2_f32 (decoder_tile.h's idiom: lane = pixel
// column, rows = output channels, the accumulator started at the bias).  K runs over (chunk of 16 input channels; tap dy, dx;
// channel pair) in one fixed order for every layer and launch shape: the 144 products of a chunk are one chain of the matrix
// instruction from zero, and the chunk sums are added to the accumulator in chunk order (a blocked sum: one chain of 4608 terms
// would carry several times the rounding error of the reference's own float32 convolutions, against which the taps are held).
// What lies outside the image is staged as zeros, so an output element is a function of its 3 x 3 x Cin inputs alone: not of
// its tile, the image size, the batch size or the position in the batch.  Every reduction of the tap term is in a fixed order
// too (an fmaf chain per pixel, fp64 butterflies per workgroup, the partials added in index order): no atomics, two calls give
// the same bits.
#include "common.h"
#include "decoder_tile.h"


namespace f3dgs {
namespace {

constexpr int NCONV = 13, NTAP = 5;
constexpr int CIN[NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int COUT[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr bool POOL[NCONV] = {false, false, true, false, true, false, false, true, false, false, true, false, false};
constexpr int TAP_AFTER[NCONV] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};
constexpr int TAP_C[NTAP] = {64, 128, 256, 512, 512};

// ---- the conv tile: 64 output channels x 4 rows x 64 pixels per workgroup, a wave = one row = 2 x 2 accumulators of 32 x 32
constexpr int CH = 16;                      // input channels per staged chunk
constexpr int TCO = 64, TROWS = 4, TPX = 64;
constexpr int IN_W = TPX + 2, IN_H = TROWS + 2, IN_PLANE = IN_H * IN_W;      // 396: 8 planes apart = 32 banks apart
constexpr int IN_ELEMS = CH * IN_PLANE;                                      // 6336
constexpr int W_STRIDE = TCO + 4;                                            // 68: 8 rows apart = 32 banks apart, rows 16-byte aligned
constexpr int W_ROWS = 9 * CH;                                               // (tap, channel) rows of a slab
constexpr int W_SLAB = W_ROWS * TCO;                                         // 9216 floats, contiguous in the packed weights
constexpr int W_PER_THREAD = W_SLAB / 4 / 256;                               // 9 float4
static_assert(W_SLAB % (4 * 256) == 0 && (IN_ELEMS + W_ROWS * W_STRIDE) * 4 <= 64 * 1024, "a slab in whole float4 rounds; one LDS image under 64 KB");

struct PackedLayout {
    size_t w[NCONV], b[NCONV], lin[NTAP], total;
};
const PackedLayout& layout() {
    static const PackedLayout L = [] {
        PackedLayout l{};
        size_t at = 0;
        auto take = [&](size_t n) { const size_t o = at; at += (n + 63) & ~(size_t)63; return o; };
        for (int i = 0; i < NCONV; i++) l.w[i] = take((size_t)COUT[i] * CIN[i] * 9);
        for (int i = 0; i < NCONV; i++) l.b[i] = take(COUT[i]);
        for (int i = 0; i < NTAP; i++) l.lin[i] = take(TAP_C[i]);
        l.total = at;
        return l;
    }();
    return L;
}

// conv weights (Cout, Cin, 3, 3) -> [Cout / 64][Cin / 16][tap][16][64]: a workgroup's slab of a chunk is one contiguous run
__global__ void lpips_pack_conv_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cin, int n) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= n) return;
    const int nch = Cin / CH;
    const int col = d % TCO, c = (d / TCO) % CH, tap = (d / (TCO * CH)) % 9, chunk = (d / W_SLAB) % nch, ct = d / (W_SLAB * nch);
    dst[d] = src[((size_t)(ct * TCO + col) * Cin + chunk * CH + c) * 9 + tap];
}
__global__ void lpips_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d < n) dst[d] = src[d];
}

// ---- the image as the first layer reads it (image_metrics.hip's two conversions, restated: the units keep their own flags)
// b / 255 for an integer 0 <= b <= 255, bit for bit torch's fp32 quotient
__device__ __forceinline__ float byte_to_unit(float b) {
    constexpr float RCP = 1.0f / 255.0f;
    const float q = __fmul_rn(b, RCP);
    const float e = __fmaf_rn(-q, 255.0f, b);
    return __fmaf_rn(e, RCP, q);
}
// what a saved PNG holds of v: floor(clamp(v * 255 + 0.5, 0, 255)), two roundings
__device__ __forceinline__ float quantize(float v) {
    const float t = __fadd_rn(__fmul_rn(v, 255.0f), 0.5f);
    return (float)(uint32_t)fminf(fmaxf(t, 0.0f), 255.0f);
}

struct Side {
    const void* p;
    int64_t sn, sc, sy, sx;      // element strides
    int u8, quant;
};
struct Images {
    Side side[2];
    int n_first;                 // images of side 0; image b >= n_first is image b - n_first of side 1
};

__device__ __forceinline__ float load_z(const Side& s, int n, int c, int y, int x) {
    const int64_t at = n * s.sn + c * s.sc + y * s.sy + x * s.sx;
    float v;
    if (s.u8) v = byte_to_unit((float)static_cast<const unsigned char*>(s.p)[at]);
    else {
        v = static_cast<const float*>(s.p)[at];
        if (s.quant) v = byte_to_unit(quantize(v));
    }
    const float mean = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f), sd = c == 0 ? .458f : (c == 1 ? .448f : .450f);
    return __fdiv_rn(__fsub_rn(v, mean), sd);
}

// conv1_1 (K = 27): one thread per output pixel, 64 fmaf chains over (c, dy, dx) from the bias; the z-scored image is zero
// outside (the reference pads AFTER the z-score).  256 threads = 4 rows x 64 pixels.
__global__ __launch_bounds__(256) void lpips_conv_first_kernel(Images im, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ out, int H, int W) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (x >= W || y >= H) return;
    const Side& s = b < im.n_first ? im.side[0] : im.side[1];
    const int n = b < im.n_first ? b : b - im.n_first;
    float v[27];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                const int gy = y + dy - 1, gx = x + dx - 1;
                v[(c * 3 + dy) * 3 + dx] = gy >= 0 && gy < H && gx >= 0 && gx < W ? load_z(s, n, c, gy, gx) : 0.f;
            }
    float* o = out + ((size_t)b * 64 * H + y) * W + x;
    const size_t plane = (size_t)H * W;
    for (int co = 0; co < 64; co++) {
        float acc = bias[co];
#pragma unroll
        for (int k = 0; k < 27; k++) acc = __fmaf_rn(w[co * 27 + k], v[k], acc);
        o[co * plane] = fmaxf(acc, 0.f);
    }
}

// ---- conv1_2 .. conv5_3
// in: (images, Cin, Hin, Win); POOL_IN: the staged pixel (y, x) is the max of in[2y .. 2y + 1][2x .. 2x + 1], H = Hin / 2,
// W = Win / 2 (floor) - no pooled tensor exists.  out: (images, Cout, H, W).  grid: (pixel tiles, Cout / 64, images).
// Staging: a thread moves positions t and t + 256 (t < 140) of the 6 x 66 halo plane of each of the chunk's 16 channels, so its
// two offsets into a plane serve every channel and chunk.
constexpr int IN_SLOTS = 2 * CH;
template <bool POOL_IN>
struct StageRegs {
    float in[IN_SLOTS][POOL_IN ? 4 : 1];      // POOL_IN: the four values of a 2x2 block
    float4 w[W_PER_THREAD];
};

template <bool POOL_IN, bool DO_IN = true, bool DO_W = true>
__device__ __forceinline__ void stage_load(StageRegs<POOL_IN>& r, const float* __restrict__ in_chunk, int off0, int off1, size_t plane_in, int Win,
                                           const float* __restrict__ w_slab) {
#pragma unroll
    for (int k = 0; DO_IN && k < IN_SLOTS; k++) {
        const int off = (k & 1) ? off1 : off0;
        const bool ok = off >= 0;
        const float* p = in_chunk + (size_t)(k >> 1) * plane_in + (ok ? off : 0);
        if constexpr (POOL_IN) {
            r.in[k][0] = ok ? p[0] : 0.f;  r.in[k][1] = ok ? p[1] : 0.f;
            r.in[k][2] = ok ? p[Win] : 0.f;  r.in[k][3] = ok ? p[Win + 1] : 0.f;
        } else {
            r.in[k][0] = ok ? p[0] : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; DO_W && k < W_PER_THREAD; k++) r.w[k] = reinterpret_cast<const float4*>(w_slab)[threadIdx.x + 256 * k];
}

template <bool POOL_IN, bool DO_IN = true, bool DO_W = true>
__device__ __forceinline__ void stage_store(const StageRegs<POOL_IN>& r, float* in_s, float* w_s) {
#pragma unroll
    for (int k = 0; DO_IN && k < IN_SLOTS; k++) {
        const int pos = threadIdx.x + 256 * (k & 1);
        float v = r.in[k][0];
        if constexpr (POOL_IN) v = fmaxf(fmaxf(r.in[k][0], r.in[k][1]), fmaxf(r.in[k][2], r.in[k][3]));
        if (pos < IN_PLANE) in_s[(k >> 1) * IN_PLANE + pos] = v;
    }
#pragma unroll
    for (int k = 0; DO_W && k < W_PER_THREAD; k++) {
        const int q = threadIdx.x + 256 * k;
        *reinterpret_cast<float4*>(w_s + (q >> 4) * W_STRIDE + (q & 15) * 4) = r.w[k];
    }
}

template <int CIN_CHUNK, bool POOL_IN>
__global__ __launch_bounds__(256, POOL_IN ? 1 : 2) void lpips_conv3x3_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ wp,
                                                            const float* __restrict__ bias, int Cin, int Cout, int H, int W, int Hin, int Win,
                                                            int tiles_x) {
    static_assert(CIN_CHUNK == CH, "the staging constants are CH's");
    // POOL_IN (4 of 12 layers): the next chunk's loads are in flight during the matrix work, one workgroup per CU.  Otherwise two
    // workgroups share a CU (256 registers) and cover each other's loads, which then need no registers across the matrix work.
    constexpr bool PREFETCH = POOL_IN;
    __shared__ __attribute__((aligned(16))) float in_s[IN_ELEMS];
    __shared__ __attribute__((aligned(16))) float w_s[W_ROWS * W_STRIDE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = lane & 31, h = lane >> 5;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x0 = tx * TPX, y0 = ty * TROWS, co0 = blockIdx.y * TCO, img = blockIdx.z;
    const int nch = Cin / CH;
    const size_t plane_in = (size_t)Hin * Win;

    // what this thread stages of every channel plane: positions t and t + 256 of in_s[c][row][col], -1 = zero (outside the image)
    int off2[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int pos = t + 256 * k, r = pos / IN_W, col = pos - r * IN_W;
        const int gy = y0 + r - 1, gx = x0 + col - 1;
        const bool ok = pos < IN_PLANE && gy >= 0 && gy < H && gx >= 0 && gx < W;
        off2[k] = ok ? (POOL_IN ? 2 * gy * Win + 2 * gx : gy * Win + gx) : -1;
    }
    const int off0 = off2[0], off1 = off2[1];
    const float* in_img = in + (size_t)img * Cin * plane_in;
    const float* w_tile = wp + (size_t)blockIdx.y * nch * W_SLAB;

    f32x16 acc[2][2];      // [output-channel half][pixel half]
#pragma unroll
    for (int ct = 0; ct < 2; ct++) {
        decoder_tile::bias_start<true>(acc[ct][0], bias, Cout, co0 + 32 * ct, h);
        acc[ct][1] = acc[ct][0];
    }

    StageRegs<POOL_IN> regs;
    stage_load<POOL_IN>(regs, in_img, off0, off1, plane_in, Win, w_tile);
    stage_store<POOL_IN>(regs, in_s, w_s);
    __syncthreads();
    // this lane's operands: A = W[co = n (+32)][k], B = X[k][pixel n (+32)] with k = channel h * 8 + j of the tap
    const float* a_base = w_s + (h * (CH / 2)) * W_STRIDE + n;
    const float* b_base = in_s + (h * (CH / 2)) * IN_PLANE + wave * IN_W + n;
    for (int ch = 0; ch < nch; ch++) {
        const bool more = ch + 1 < nch;
        f32x16 part[2][2];      // the chunk's 144 products, summed from zero on the matrix pipe
#pragma unroll
        for (int ct = 0; ct < 2; ct++)
#pragma unroll
            for (int pg = 0; pg < 2; pg++)
#pragma unroll
                for (int r = 0; r < 16; r++) part[ct][pg][r] = 0.f;
        if (PREFETCH && more) stage_load<POOL_IN>(regs, in_img + (size_t)(ch + 1) * CH * plane_in, off0, off1, plane_in, Win, w_tile + (size_t)(ch + 1) * W_SLAB);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int dy = tap / 3, dx = tap - 3 * dy;
#pragma unroll
            for (int j = 0; j < CH / 2; j++) {
                const float a0 = a_base[(tap * CH + j) * W_STRIDE], a1 = a_base[(tap * CH + j) * W_STRIDE + 32];
                const float b0 = b_base[j * IN_PLANE + dy * IN_W + dx], b1 = b_base[j * IN_PLANE + dy * IN_W + dx + 32];
                part[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, part[0][0], 0, 0, 0);
                part[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, part[0][1], 0, 0, 0);
                part[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, part[1][0], 0, 0, 0);
                part[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, part[1][1], 0, 0, 0);
                if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // keeps the LDS reads of later steps from being hoisted (registers)
            }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ct++)
#pragma unroll
            for (int pg = 0; pg < 2; pg++) acc[ct][pg] += part[ct][pg];
        __syncthreads();
        if (PREFETCH) {
            if (more) stage_store<POOL_IN>(regs, in_s, w_s);
        } else if (more) {      // the halo tile, then the slab: half the registers at a time
            stage_load<POOL_IN, true, false>(regs, in_img + (size_t)(ch + 1) * CH * plane_in, off0, off1, plane_in, Win, nullptr);
            stage_store<POOL_IN, true, false>(regs, in_s, w_s);
            stage_load<POOL_IN, false, true>(regs, nullptr, off0, off1, plane_in, Win, w_tile + (size_t)(ch + 1) * W_SLAB);
            stage_store<POOL_IN, false, true>(regs, in_s, w_s);
        }
        __syncthreads();
    }

    const int y = y0 + wave;
    if (y >= H) return;
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
#pragma unroll
        for (int pg = 0; pg < 2; pg++) {
            const int x = x0 + 32 * pg + n;
            if (x >= W) continue;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int co = co0 + 32 * ct + mfma_row(r, h);
                out[((size_t)img * Cout + co) * plane + (size_t)y * W + x] = fmaxf(acc[ct][pg][r], 0.f);
            }
        }
}

// ---- the tap term: one thread per pixel of a pair, two passes over the channels of both images (the norms, then the
// weighted squared difference of the normalised values, as the reference writes it); the pixel values are summed in fp64 per
// workgroup in a fixed order into partials[pair][blocks]
__global__ __launch_bounds__(256) void lpips_tap_kernel(const float* __restrict__ taps, const float* __restrict__ lin, int C, int HW, int N,
                                                        double* __restrict__ partials, int partial_stride) {
    __shared__ double s_w[4];
    const int p = blockIdx.x * 256 + threadIdx.x, pair = blockIdx.y;
    float v = 0.f;
    if (p < HW) {
        const float* tx = taps + (size_t)pair * C * HW + p;
        const float* ty = taps + (size_t)(N + pair) * C * HW + p;
        float sx = 0.f, sy = 0.f;
        for (int c = 0; c < C; c++) {
            const float a = tx[(size_t)c * HW], b = ty[(size_t)c * HW];
            sx = __fmaf_rn(a, a, sx);
            sy = __fmaf_rn(b, b, sy);
        }
        const float na = __fadd_rn(__fsqrt_rn(sx), 1e-10f), nb = __fadd_rn(__fsqrt_rn(sy), 1e-10f);
        for (int c = 0; c < C; c++) {
            const float d = __fsub_rn(__fdiv_rn(tx[(size_t)c * HW], na), __fdiv_rn(ty[(size_t)c * HW], nb));
            v = __fmaf_rn(lin[c], __fmul_rn(d, d), v);
        }
    }
    const double s = wave_sum((double)v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[(size_t)pair * partial_stride + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

struct FinalArgs {
    int first[NTAP], blocks[NTAP], pixels[NTAP];
};
// one workgroup per pair: per layer, thread t adds partials t, t + 256, ... in index order, the 256 sums meet in a fixed tree
__global__ __launch_bounds__(256) void lpips_final_kernel(const double* __restrict__ partials, int partial_stride, FinalArgs fa,
                                                          float* __restrict__ layer_terms, float* __restrict__ totals) {
    __shared__ double s_w[4];
    const int pair = blockIdx.x;
    double total = 0.0;
    for (int l = 0; l < NTAP; l++) {
        const double* p = partials + (size_t)pair * partial_stride + fa.first[l];
        double s = 0.0;
        for (int i = threadIdx.x; i < fa.blocks[l]; i += 256) s += p[i];
        s = wave_sum(s);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
        __syncthreads();
        const double d = (((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]) / (double)fa.pixels[l];
        if (threadIdx.x == 0 && layer_terms) layer_terms[pair * NTAP + l] = (float)d;
        total += d;
    }
    if (threadIdx.x == 0 && totals) totals[pair] = (float)total;
}

// ---- host side
constexpr int MAX_IMAGES = 65534;               // gridDim.z of the conv launches
constexpr long long MAX_PIXELS = 1ll << 26;     // an offset into a plane is an int

bool size_ok(int N, int H, int W) { return N >= 0 && H >= 16 && W >= 16 && (long long)H * W <= MAX_PIXELS && 2ll * N <= MAX_IMAGES; }

struct Workspace {
    float* buf[2];
    double* partials;
    int partial_stride;
    FinalArgs fa;
    size_t total;
};
Workspace carve_workspace(char* base, int images, int pairs, int H, int W) {
    Workspace ws{};
    Carver c(base);
    const size_t act = (size_t)images * 64 * H * W;
    ws.buf[0] = c.take<float>(act);
    ws.buf[1] = c.take<float>(act);
    int at = 0, h = H, w = W;
    for (int l = 0; l < NTAP; l++) {
        ws.fa.first[l] = at; ws.fa.pixels[l] = h * w; ws.fa.blocks[l] = (h * w + 255) / 256;
        at += ws.fa.blocks[l];
        h /= 2; w /= 2;
    }
    ws.partial_stride = at;
    ws.partials = c.take<double>((size_t)pairs * at);
    ws.total = c.total();
    return ws;
}

template <bool POOL_IN>
void launch_conv(const float* in, float* out, const float* w, const float* b, int layer, int images, int H, int W, int Hin, int Win, hipStream_t st) {
    const int tiles_x = (W + TPX - 1) / TPX, tiles_y = (H + TROWS - 1) / TROWS;
    lpips_conv3x3_kernel<CH, POOL_IN><<<dim3(tiles_x * tiles_y, COUT[layer] / TCO, images), 256, 0, st>>>(in, out, w, b, CIN[layer], COUT[layer], H, W,
                                                                                                         Hin, Win, tiles_x);
}

// the 13 convolutions over `images` images; tap l lands in tap_dst[l] (or, where that is null, stays in the ping-pong buffer)
// and on_tap(l, tap, C, H_l, W_l) runs behind the block's last convolution
template <class OnTap>
void run_chain(const Images& im, int images, int H, int W, const float* packed, const Workspace& ws, float* const* tap_dst, hipStream_t st,
               OnTap on_tap) {
    const PackedLayout& L = layout();
    int h = H, w = W, cur = 0;
    lpips_conv_first_kernel<<<dim3((W + 63) / 64, (H + 3) / 4, images), 256, 0, st>>>(im, packed + L.w[0], packed + L.b[0], ws.buf[0], H, W);
    const float* src = ws.buf[0];
    for (int i = 1; i < NCONV; i++) {
        const int hin = h, win = w;
        if (POOL[i]) { h /= 2; w /= 2; }
        const int l = TAP_AFTER[i];
        float* dst = l >= 0 && tap_dst && tap_dst[l] ? tap_dst[l] : ws.buf[cur ^ 1];
        if (POOL[i]) launch_conv<true>(src, dst, packed + L.w[i], packed + L.b[i], i, images, h, w, hin, win, st);
        else launch_conv<false>(src, dst, packed + L.w[i], packed + L.b[i], i, images, h, w, hin, win, st);
        if (dst == ws.buf[cur ^ 1]) cur ^= 1;
        src = dst;
        if (l >= 0) on_tap(l, src, COUT[i], h, w);
    }
}

int check_side(const char* who, const char* name, const void* p, int format, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int flags, int qflag) {
    if (!p) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (%s)", who, name);
    if (format != F3DGS_LPIPS_F32 && format != F3DGS_LPIPS_U8) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: unknown format %d of %s", who, format, name);
    if (sn < 0 || sc < 0 || sy < 0 || sx < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a negative stride of %s", who, name);
    if (format == F3DGS_LPIPS_U8 && (flags & qflag)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: the quantize flag on the uint8 side %s", who, name);
    if (format == F3DGS_LPIPS_F32 && (reinterpret_cast<uintptr_t>(p) & 3)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", who, name);
    return F3DGS_OK;
}

}  // namespace
}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_lpips_weights_bytes(void) { return layout().total * sizeof(float); }

int f3dgs_lpips_pack_weights(const float* const* params, int n_params, float* packed, void* stream) {
    const char* who = "f3dgs_lpips_pack_weights";
    if (n_params != F3DGS_LPIPS_PARAMS) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: %d parameters, the table has %d", who, n_params, F3DGS_LPIPS_PARAMS);
    if (!params || !packed) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (params, packed)", who);
    for (int i = 0; i < n_params; i++)
        if (!params[i]) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (parameter %d)", who, i);
    if (!aligned16(packed)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: packed must be 16-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const PackedLayout& L = layout();
    for (int i = 0; i < NCONV; i++) {
        const int n = COUT[i] * CIN[i] * 9;
        if (i == 0) lpips_copy_kernel<<<(n + 255) / 256, 256, 0, st>>>(params[i], packed + L.w[i], n);
        else lpips_pack_conv_kernel<<<(n + 255) / 256, 256, 0, st>>>(params[i], packed + L.w[i], CIN[i], n);
        lpips_copy_kernel<<<(COUT[i] + 255) / 256, 256, 0, st>>>(params[NCONV + i], packed + L.b[i], COUT[i]);
    }
    for (int l = 0; l < NTAP; l++) lpips_copy_kernel<<<(TAP_C[l] + 255) / 256, 256, 0, st>>>(params[2 * NCONV + l], packed + L.lin[l], TAP_C[l]);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

size_t f3dgs_lpips_workspace_bytes(int N, int H, int W) {
    if (!size_ok(N, H, W) || N == 0) return 0;
    return carve_workspace(nullptr, 2 * N, N, H, W).total;
}

int f3dgs_lpips_forward(int N, int H, int W, const void* x, int x_format, int64_t x_stride_n, int64_t x_stride_c, int64_t x_stride_y,
                        int64_t x_stride_x, const void* y, int y_format, int64_t y_stride_n, int64_t y_stride_c, int64_t y_stride_y,
                        int64_t y_stride_x, int flags, const float* packed, float* layer_terms, float* totals, void* workspace,
                        size_t workspace_bytes, void* stream) {
    const char* who = "f3dgs_lpips_forward";
    if (N < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: N < 0", who);
    if (H < 16 || W < 16) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a %d x %d image, the fifth block needs 16 x 16", who, H, W);
    if (!size_ok(N, H, W)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: %d pairs of %d x %d: up to %d images of %lld pixels are taken", who, N, H, W, MAX_IMAGES, MAX_PIXELS);
    if (flags & ~(F3DGS_LPIPS_QUANTIZE_X | F3DGS_LPIPS_QUANTIZE_Y)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", who, flags);
    if (N == 0) return F3DGS_OK;
    int rc = check_side(who, "x", x, x_format, x_stride_n, x_stride_c, x_stride_y, x_stride_x, flags, F3DGS_LPIPS_QUANTIZE_X);
    if (rc != F3DGS_OK) return rc;
    rc = check_side(who, "y", y, y_format, y_stride_n, y_stride_c, y_stride_y, y_stride_x, flags, F3DGS_LPIPS_QUANTIZE_Y);
    if (rc != F3DGS_OK) return rc;
    if (!packed || (!layer_terms && !totals)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (packed, or both outputs)", who);
    const size_t need = f3dgs_lpips_workspace_bytes(N, H, W);
    if (!workspace || workspace_bytes < need)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: workspace of %zu bytes, %zu are needed", who, workspace ? workspace_bytes : (size_t)0, need);
    if (misaligned16({packed, workspace})) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: packed and workspace must be 16-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Workspace ws = carve_workspace(static_cast<char*>(workspace), 2 * N, N, H, W);
    Images im{};
    im.side[0] = Side{x, x_stride_n, x_stride_c, x_stride_y, x_stride_x, x_format == F3DGS_LPIPS_U8, (flags & F3DGS_LPIPS_QUANTIZE_X) != 0};
    im.side[1] = Side{y, y_stride_n, y_stride_c, y_stride_y, y_stride_x, y_format == F3DGS_LPIPS_U8, (flags & F3DGS_LPIPS_QUANTIZE_Y) != 0};
    im.n_first = N;
    const PackedLayout& L = layout();
    run_chain(im, 2 * N, H, W, packed, ws, nullptr, st, [&](int l, const float* tap, int C, int h, int w) {
        lpips_tap_kernel<<<dim3(ws.fa.blocks[l], N), 256, 0, st>>>(tap, packed + L.lin[l], C, h * w, N, ws.partials + ws.fa.first[l], ws.partial_stride);
    });
    lpips_final_kernel<<<N, 256, 0, st>>>(ws.partials, ws.partial_stride, ws.fa, layer_terms, totals);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

int f3dgs_lpips_taps(int N, int H, int W, const void* image, int format, int64_t stride_n, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                     int quantize, const float* packed, float* const* taps, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "f3dgs_lpips_taps";
    if (N < 0) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: N < 0", who);
    if (H < 16 || W < 16) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: a %d x %d image, the fifth block needs 16 x 16", who, H, W);
    if (!size_ok((N + 1) / 2, H, W)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "%s: %d images of %d x %d: up to %d images of %lld pixels are taken", who, N, H, W, MAX_IMAGES, MAX_PIXELS);
    if (N == 0) return F3DGS_OK;
    const int rc = check_side(who, "image", image, format, stride_n, stride_c, stride_y, stride_x, quantize ? 1 : 0, 1);
    if (rc != F3DGS_OK) return rc;
    if (!packed || !taps) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (packed, taps)", who);
    for (int l = 0; l < NTAP; l++)
        if (!taps[l]) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: null pointer (tap %d)", who, l);
    const size_t need = f3dgs_lpips_workspace_bytes((N + 1) / 2, H, W);
    if (!workspace || workspace_bytes < need)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: workspace of %zu bytes, %zu are needed", who, workspace ? workspace_bytes : (size_t)0, need);
    if (misaligned16({packed, workspace})) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "%s: packed and workspace must be 16-byte aligned", who);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const Workspace ws = carve_workspace(static_cast<char*>(workspace), 2 * ((N + 1) / 2), (N + 1) / 2, H, W);
    Images im{};
    im.side[0] = Side{image, stride_n, stride_c, stride_y, stride_x, format == F3DGS_LPIPS_U8, quantize != 0};
    im.side[1] = im.side[0];
    im.n_first = N;
    run_chain(im, N, H, W, packed, ws, taps, st, [](int, const float*, int, int, int) {});
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_errorf(F3DGS_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return F3DGS_OK;
}

}  // extern "C"
