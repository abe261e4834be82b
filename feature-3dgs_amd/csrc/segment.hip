// segment.hip - open-vocabulary segmentation of a rendered feature map: resize -> optional 1x1 decoder -> fp16 store ->
// per-pixel cosine against K text embeddings -> argmax, as ONE pass in which neither the decoded (Cout,Hs,Ws) map nor
// the (Hs Ws, K) logits ever exist in memory.
//
// Replaces the reference's chain over two scripts (render.py:168-180, encoders/lseg_encoder/segmentation.py:526-540):
//     feature_map = F.interpolate(feature_map[None], size=(Hs, Ws), mode='bilinear', align_corners=True)[0]
//     if speedup: feature_map = cnn_decoder(feature_map)                      # 1x1 conv, C -> Cout
//     feature_map = feature_map.half()                                        # the stored map
//     f = feature_map.float().permute(1, 2, 0).reshape(-1, Cout);  f = f / f.norm(dim=-1, keepdim=True)
//     t = text / text.norm(dim=-1, keepdim=True)
//     labels = torch.max(f @ t.t(), 1)[1]
// Stages (N = Hs*Ws output pixels):
//   seg_text_kernel   t_k / ||t_k|| in fp32 into scratch, zero rows up to a multiple of 32 (skipped: TEXT_NORMALIZED)
//   fl_resize_kernel  (feature_loss.hip, with a decoder only) the resized map, pixel-major X[N][C]: the decode's own kernel,
//                     so the decoded values below are those of f3dgs_feature_decode bit for bit
//   seg_kernel        a WAVE owns 32 pixels, a workgroup = 4 waves = 128 pixels.  Per 32-row block of the decoder:
//     phase A   D^T[co][px] = W[co][:] . X[px][:] + b[co]   fl_decode_kernel's loop itself (decoder_tile.h: one copy for both);
//               without a decoder the block is the resized map itself, taken from the source map with fl_resize_out_kernel's
//               expression, in the accumulator's layout
//     in place  ROUND_HALF: every value to IEEE fp16 and back;  ss += D^2
//     phase B   L^T[k][px] += T^[k][co] D^T[co][px]          A = the text tile (b128 LDS reads: four steps per read), B = the
//               accumulator register r of phase A itself: D's layout (lane = column px, register r = row co(r, h)) IS the
//               B layout when step r contracts co(r, 0) with co(r, 1) (feature_loss.hip, phase B) - no LDS round trip
//   after the last block   score_k = L[k] / sqrt(ss), argmax over k: NaN is the maximum, the lowest k wins a tie (edit.hip)
// Shared data: the current 32-row tile of W and the matching 32 columns of T^ in LDS, both double-buffered, the next tiles in
// flight in registers during the MFMAs.  All arithmetic is fp32 (v_mfma_f32_32x32x2_f32: exact fp32 products and sums).

#include <hip/hip_fp16.h>
#include <math.h>

#include "common.h"
#include "decoder_tile.h"
#include "resize_taps.h"

namespace f3dgs {

namespace {

constexpr int SEG_TS = 36;     // text tile row stride: 32 columns + one b128 of padding, so that the b128 reads of 32 rows hit all banks evenly

struct SegArgs {
    ResizeGeom g;
    int N, C, Cout, K;
    int text_rows;             // rows of `text` that may be read: K (the caller's matrix) or K padded to 32 (the scratch copy)
    int text_vec;              // rows can be read with 16-byte loads
    int round_half;
    int identity;              // Hs == H and Ws == W: no resize - a pixel is its source value, whatever its neighbours hold
    const float* fm;           // (C,H,W), read by the kernel itself without a decoder
    const float* X;            // [N][C], with a decoder
    const float* Wd;
    const float* bias;
    const float* text;         // normalised rows, row stride Cout
    int64_t* labels;
    float* score;              // or nullptr
};

__device__ __forceinline__ float round_h(float x) { return __half2float(__float2half_rn(x)); }

// torch.max / torch.argmax: NaN is the maximum, the lowest index wins among equals
__device__ __forceinline__ bool seg_better(float va, int ia, float vb, int ib) {
    const bool an = va != va, bn = vb != vb;
    return an ? (!bn || ia < ib) : (!bn && (va > vb || (va == vb && ia < ib)));
}

// ---- t_k / ||t_k|| (fp32 norm, fp32 quotient) into scratch rows of Cout floats; rows K .. Kpad - 1 are zero.  One wave per row.
__global__ void __launch_bounds__(256) seg_text_kernel(int K, int Kpad, int Cout, const float* __restrict__ text, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= Kpad) return;
    float* o = out + (size_t)k * Cout;
    if (k >= K) {
        for (int c = lane; c < Cout; c += 64) o[c] = 0.f;
        return;
    }
    const float* t = text + (size_t)k * Cout;
    float ss = 0.f;
    for (int c = lane; c < Cout; c += 64) ss = fmaf(t[c], t[c], ss);
    const float n = sqrtf(wave_sum(ss));
    for (int c = lane; c < Cout; c += 64) o[c] = t[c] / n;
}

// C: the decoder's input width (32, 64, 128), or 0 for no decoder.  NKB: 32-row blocks of text (K <= 32 NKB).
// Registers per lane: 16 NKB logit accumulators + C/2 (this lane's half row of X) + 16 (the decoded block) + the tiles in flight;
// the widest shapes take one wave per SIMD (512 registers), the others two.
template <int C, int NKB>
constexpr int seg_waves() { return ((C == 0 || C >= 128) && NKB > 5) || NKB > 6 ? 1 : 2; }

template <int C, int NKB>
constexpr size_t seg_lds_bytes() { return sizeof(float) * (2 * 32 * NKB * SEG_TS + (C ? 2 * 32 * decoder_tile::WS<C> : 0)); }

template <int C, int NKB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(seg_waves<C, NKB>())))
seg_kernel(const SegArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool DEC = C > 0;
    namespace dt = decoder_tile;
    constexpr int HC = DEC ? C / 2 : 1;
    constexpr int LPT = DEC ? dt::LPT<C> : 1;              // float4 per thread for one W tile
    float* const Ts = reinterpret_cast<float*>(smem);      // [2][32 NKB][SEG_TS]
    float* Ws = Ts + 2 * 32 * NKB * SEG_TS;                // the decoder's W tiles (decoder_tile.h)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int N = a.N, Cout = a.Cout;
    const int p = blockIdx.x * 128 + 32 * w + li;
    const bool p_ok = p < N;

    // text tile: columns co0 .. co0 + 31 of every row; thread t moves float4 #(t + 256 j) of the (32 NKB) x 32 tile
    auto load_text = [&](int co0, float4 (&v)[NKB]) {
#pragma unroll
        for (int j = 0; j < NKB; j++) {
            const int e = (threadIdx.x + 256 * j) * 4, k = e >> 5, c = co0 + (e & 31);
            const float* src = a.text + (size_t)k * Cout + c;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k < a.text_rows) {
                if (a.text_vec) {
                    if (c < Cout) t = *reinterpret_cast<const float4*>(src);       // Cout % 4 == 0: all four or none
                } else {
                    if (c < Cout) t.x = src[0];
                    if (c + 1 < Cout) t.y = src[1];
                    if (c + 2 < Cout) t.z = src[2];
                    if (c + 3 < Cout) t.w = src[3];
                }
            }
            v[j] = t;
        }
    };
    auto store_text = [&](int buf, const float4 (&v)[NKB]) {
#pragma unroll
        for (int j = 0; j < NKB; j++) {
            const int e = (threadIdx.x + 256 * j) * 4, k = e >> 5, c = e & 31;
            *reinterpret_cast<float4*>(Ts + ((size_t)buf * 32 * NKB + k) * SEG_TS + c) = v[j];
        }
    };
    // W tile staging (nothing without a decoder)
    auto load_w = [&](int co0, float4 (&v)[LPT]) {
        if constexpr (DEC) dt::load_w<C>(v, a.Wd, Cout, co0);
    };
    auto store_w = [&](int buf, const float4 (&v)[LPT]) {
        if constexpr (DEC) dt::store_w<C>(Ws, buf, v);
    };

    // with a decoder: this lane's half row of X.  Without: the lane's taps into the source map
    float xr[HC];
    uint32_t o00 = 0, o01 = 0, o10 = 0, o11 = 0;
    PixelTaps tp = {};
    if constexpr (DEC) {
        dt::load_x<C, false>(xr, a.X, p, N, h);
    } else {
        const int pp = p_ok ? p : 0;
        const int yo = pp / a.g.Wg, xo = pp - yo * a.g.Wg;
        tp = pixel_taps(a.g, yo, xo);
        o00 = tp.y0 * a.g.W + tp.x0; o01 = tp.y0 * a.g.W + tp.x1; o10 = tp.y1 * a.g.W + tp.x0; o11 = tp.y1 * a.g.W + tp.x1;
    }
    // addresses as (wave-uniform channel plane) + (one 32-bit lane offset per tap): channel(r, h) = channel(r, 0) + 4 h, so the
    // lane-dependent part does not depend on r (sixty-four 64-bit per-lane addresses would otherwise be formed per block)
    const size_t plane = (size_t)a.g.H * a.g.W;
    const uint32_t hp = (uint32_t)(4 * h) * (uint32_t)plane;
    // the resized block of channels c0 .. c0 + 31 in the accumulator's layout (register r = channel c0 + row(r, h)); zero beyond C
    auto resized = [&](int c0, float (&v)[16]) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int cu = c0 + mfma_row(r, 0);                                   // uniform
            const bool ok = cu + 4 * h < a.C;
            const float* pl = a.fm + (size_t)(cu < a.C ? cu : 0) * plane;         // uniform
            const uint32_t ho = ok ? hp : 0u;
            // (the taps of an identity resize have weights 1, 0, 0, 0, and 0 * inf of a neighbour would make this pixel NaN)
            const float val = a.identity ? pl[ho + o00] : bilinear_mix(tp, pl[ho + o00], pl[ho + o01], pl[ho + o10], pl[ho + o11]);
            v[r] = ok ? val : 0.f;
        }
    };

    f32x16 lg[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) lg[kb][r] = 0.f;
    float ss = 0.f;

    float4 tnext[NKB];
    float4 wnext[LPT];
    float cur[16];
    load_text(0, tnext);
    load_w(0, wnext);
    if constexpr (!DEC) resized(0, cur);
    store_text(0, tnext);
    store_w(0, wnext);
    __syncthreads();
    const int ntiles = (Cout + 31) / 32;
    for (int t = 0; t < ntiles; t++) {
        const int co0 = 32 * t, buf = t & 1;
        const bool more = t + 1 < ntiles;
        f32x16 acc;
        if constexpr (DEC) {
            constexpr bool LATE_W = dt::LATE_W<C>;
            if (!LATE_W && more) load_w(co0 + 32, wnext);
            dt::bias_start<true>(acc, a.bias, Cout, co0, h);          // Cout % 32 == 0 with a decoder
            dt::phase_a<C>(acc, Ws, buf, li, h, xr);                  // fl_decode_kernel's, call for call
            if (LATE_W && more) load_w(co0 + 32, wnext);
        } else {
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = cur[r];
            if (more) resized(co0 + 32, cur);          // the next block's taps: in flight during phase B
        }
        if (more) load_text(co0 + 32, tnext);
        // ---- the stored value (fp16 and back) and the pixel's squared norm, in place
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float v = a.round_half ? round_h(acc[r]) : acc[r];
            acc[r] = v;
            ss = fmaf(v, v, ss);
        }
        // ---- phase B: step r contracts co(r, 0) with co(r, 1); a lane's four A values of a register quad are consecutive in LDS
        const float* trow = Ts + ((size_t)buf * 32 * NKB + li) * SEG_TS + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int kb = 0; kb < NKB; kb++) {
                const float4 av = *reinterpret_cast<const float4*>(trow + (size_t)kb * 32 * SEG_TS + 8 * q);
                lg[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, acc[4 * q + 0], lg[kb], 0, 0, 0);
                lg[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, acc[4 * q + 1], lg[kb], 0, 0, 0);
                lg[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, acc[4 * q + 2], lg[kb], 0, 0, 0);
                lg[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, acc[4 * q + 3], lg[kb], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) {          // the other buffers: their readers finished a tile ago
            store_text(buf ^ 1, tnext);
            store_w(buf ^ 1, wnext);
        }
        __syncthreads();
    }

    // ---- score and argmax.  L^T[k][px]: this lane holds column px and rows k = 32 kb + row(r, h); its partner lane ^ 32 the others
    ss += __shfl_xor(ss, 32, 64);
    const float nrm = sqrtf(ss);
    float bv = -INFINITY;
    int bk = 0x7fffffff;
#pragma unroll
    for (int kb = 0; kb < NKB; kb++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int k = 32 * kb + mfma_row(r, h);
            const float s = lg[kb][r] / nrm;
            if (k < a.K && seg_better(s, k, bv, bk)) { bv = s; bk = k; }
        }
    const float ov = __shfl_xor(bv, 32, 64);
    const int ok = __shfl_xor(bk, 32, 64);
    if (seg_better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    if (p_ok && h == 0) {
        a.labels[p] = (int64_t)bk;
        if (a.score) a.score[p] = bv;
    }
}

template <int C, int NKB>
hipError_t seg_launch(const SegArgs& a, hipStream_t s) {
    constexpr size_t lds = seg_lds_bytes<C, NKB>();
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&seg_kernel<C, NKB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((seg_kernel<C, NKB>), dim3((a.N + 127) / 128), dim3(256), lds, s, a);
    return hipGetLastError();
}

template <int C>
hipError_t seg_dispatch(const SegArgs& a, hipStream_t s) {
    switch ((a.K + 31) / 32) {
        case 1: return seg_launch<C, 1>(a, s);
        case 2: return seg_launch<C, 2>(a, s);
        case 3: return seg_launch<C, 3>(a, s);
        case 4: return seg_launch<C, 4>(a, s);
        case 5: return seg_launch<C, 5>(a, s);
        case 6: return seg_launch<C, 6>(a, s);
        case 7: return seg_launch<C, 7>(a, s);
        case 8: return seg_launch<C, 8>(a, s);
    }
    return hipErrorInvalidValue;
}

struct SegScratch {
    float* X;
    float* text;
    static SegScratch carve(char* base, int C, int Cout, int N, int K, bool decoder, size_t* bytes) {
        Carver c(base);
        SegScratch s;
        s.X = c.take<float>(decoder ? (size_t)N * C : 0);
        s.text = c.take<float>((size_t)((K + 31) / 32 * 32) * Cout);
        if (bytes) *bytes = c.total();
        return s;
    }
};

size_t segment_scratch_bytes(int C, int Cout, int Hs, int Ws, int K, bool decoder) {
    size_t b = 0;
    SegScratch::carve(nullptr, C, Cout, Hs * Ws, K, decoder, &b);
    return b;
}

hipError_t launch_segment(int C, int H, int W, int Cout, int Hs, int Ws, int K, const float* feature_map, const float* weight,
                          const float* bias, const float* text, bool round_half, bool text_normalized, int64_t* labels,
                          float* score, char* scratch, hipStream_t s) {
    const bool decoder = weight != nullptr;
    const int N = Hs * Ws;
    const SegScratch sc = SegScratch::carve(scratch, C, Cout, N, K, decoder, nullptr);
    const int Kpad = (K + 31) / 32 * 32;
    SegArgs a;
    a.g = make_resize_geom(H, W, Hs, Ws);
    a.N = N; a.C = C; a.Cout = Cout; a.K = K;
    a.round_half = round_half ? 1 : 0;
    a.identity = (!decoder && H == Hs && W == Ws) ? 1 : 0;
    a.fm = feature_map; a.X = sc.X; a.Wd = weight; a.bias = bias;
    a.labels = labels; a.score = score;
    if (text_normalized) {
        a.text = text;
        a.text_rows = K;
    } else {
        hipLaunchKernelGGL(seg_text_kernel, dim3((Kpad + 3) / 4), dim3(256), 0, s, K, Kpad, Cout, text, sc.text);
        a.text = sc.text;
        a.text_rows = Kpad;
    }
    a.text_vec = (Cout % 4 == 0 && (reinterpret_cast<uintptr_t>(a.text) & 15) == 0) ? 1 : 0;
    if (!decoder) return seg_dispatch<0>(a, s);
    launch_feature_resize(C, H, W, Hs, Ws, feature_map, sc.X, s);
    if (C == 32) return seg_dispatch<32>(a, s);
    if (C == 64) return seg_dispatch<64>(a, s);
    if (C == 128) return seg_dispatch<128>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace

}  // namespace f3dgs

using namespace f3dgs;

extern "C" {

size_t f3dgs_segment_scratch_bytes(int C, int Cout, int Hs, int Ws, int K, int has_decoder) {
    if (C <= 0 || Cout <= 0 || Hs < 0 || Ws < 0 || K <= 0 || (long long)Hs * Ws > (1ll << 30)) return 0;
    return segment_scratch_bytes(C, Cout, Hs, Ws, K, has_decoder != 0);
}

int f3dgs_segment(int C, int H, int W, int Cout, int Hs, int Ws, int K, const float* feature_map, const float* weight,
                  const float* bias, const float* text, int flags, int64_t* labels, float* score, void* scratch, void* stream) {
    if (C <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Hs < 0 || Ws < 0 || K <= 0)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "segment: bad sizes C=%d H=%d W=%d Cout=%d Hs=%d Ws=%d K=%d", C, H, W, Cout, Hs, Ws, K);
    const int known = F3DGS_SEGMENT_ROUND_HALF | F3DGS_SEGMENT_TEXT_NORMALIZED;
    if (flags & ~known) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "segment: unknown flag bits 0x%x", flags & ~known);
    if ((weight == nullptr) != (bias == nullptr)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "segment: weight and bias go together");
    if (!weight && Cout != C)
        return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "segment: without a decoder the text has C = %d channels, got %d", C, Cout);
    if (K > F3DGS_SEGMENT_MAX_TEXTS) return report_errorf(F3DGS_ERR_UNSUPPORTED, "segment: K=%d beyond the limit of %d text rows", K, F3DGS_SEGMENT_MAX_TEXTS);
    if (weight && (!feature_l1_decoder_supported(C) || Cout % 32 != 0))
        return report_errorf(F3DGS_ERR_UNSUPPORTED, "segment: decoder %d -> %d: supported are input widths 32, 64, 128 and outputs that are multiples of 32", C, Cout);
    if ((long long)Hs * Ws > (1ll << 30) || (long long)H * W > (1ll << 28)) return report_errorf(F3DGS_ERR_UNSUPPORTED, "segment: too large");
    if (Hs == 0 || Ws == 0) return F3DGS_OK;
    const bool text_normalized = (flags & F3DGS_SEGMENT_TEXT_NORMALIZED) != 0;
    if (!feature_map || !text || !labels) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "segment: null pointer");
    if (!scratch && (weight || !text_normalized)) return report_errorf(F3DGS_ERR_INVALID_ARGUMENT, "segment: scratch is null");
    HIP_TRY(launch_segment(C, H, W, Cout, Hs, Ws, K, feature_map, weight, bias, text, (flags & F3DGS_SEGMENT_ROUND_HALF) != 0,
                           text_normalized, labels, score, static_cast<char*>(scratch), static_cast<hipStream_t>(stream)));
    return F3DGS_OK;
}

}  // extern "C"
