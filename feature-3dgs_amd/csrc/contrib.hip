// contrib.hip — the contribution pass: one more walk over the tile lists of a finished forward call that answers "which
// Gaussians lie behind this region of the view?" (include/f3dgs.h: f3dgs_contributions).  No counterpart in the reference,
// whose only route from a 2D mask to the Gaussians is the blend backward with the masks as upstream gradient.
//
// Per (pixel, list entry) the blend weight w = alpha T is formed with the forward's own instruction sequence (render_common.h:
// splat_power2 on the conic scaled at staging, v_exp_f32, the 0.99 clamp, the power > 0 and alpha < 1/255 skips, T *= 1 - alpha)
// and the set of contributors is the forward's n_contrib - the T < 1e-4 termination is not decided a second time - so the
// weights are the forward's, bit for bit.  From them:
//   per pixel     alpha = 1 - T_final, the depth at which T crosses 0.5 (Q4: no background, 0 when it never does), the index
//                 and the weight of the entry of largest weight (strict >: the earliest of a tie);
//   per Gaussian  acc[g][k] += sum over pixels of w masks[k][pixel] (k < K), acc[g][K] += sum of w, wmax[g] = max(wmax[g], w).
//
// Decomposition of render_common.h: one 16x16 tile per workgroup, a wave per 8x8 quadrant, chunks of 64 list entries staged in
// the wave's LDS slice behind the forward's record / list prefetch pipeline and its wave-level footprint test (rect_hit: an
// entry it drops cannot reach 1/255 at any pixel of the quadrant, so it would be skipped sixty-four times anyway).
//
// The per-Gaussian sums leave the wave through registers only (no LDS atomics: DESIGN 8): the up to eight columns a lane
// carries are reduce-scattered over the wave - at each of the first log2(columns) lane-exchange steps a lane keeps half of its
// columns and hands the other half to its partner, then the one column left is summed over the remaining steps: 7 + 3 adds for
// eight columns instead of 6 x 8 - and the lanes 0 .. columns - 1 issue ONE global atomic for the wave and the entry, one dword
// each on consecutive addresses.  Nothing is issued for an entry no lane blends, nor for a column whose sum is zero.
//
// The walk is written once (walk_setup, walk_list) and has two users, which hand it what they do with a blended entry:
// contrib_kernel, and label_votes_kernel (f3dgs_label_votes) for the one-hot masks of an integer label map.  A third pass over
// a finished call's lists belongs here too: one instruction sequence forms every weight, under one set of flags.
#include "render_common.h"

namespace f3dgs {

namespace {

struct ContribChunk {
    float4 geo[64];    // mean_x, mean_y, conic_a', conic_b' (scaled, see splat_power2)
    float4 tail[64];   // conic_c', opacity, depth (0 where the walk does not carry it), Gaussian index (bits)
    uint32_t pos[64];  // 1-based list position
};

// a lane's pixel and its wave's piece of the tile's list
struct WalkLane {
    int iwx0, iwy0;        // first pixel of the wave's quadrant (wave-uniform)
    bool inside;
    size_t pid;
    float pxf, pyf;
    uint32_t last;         // the forward's own contributors: list positions up to n_contrib (an entry behind it never blended, see render_fwd.hip)
    uint32_t r_lo, r_hi;   // wave-uniform; r_hi clipped at the wave's largest `last`: empty where nothing blended
};

__device__ __forceinline__ WalkLane walk_setup(const WalkArgs& a, int lane, int wave) {
    WalkLane p;
    const uint32_t vb = xcd_remap(blockIdx.x, gridDim.x);
    const uint32_t tile = band_perm(vb, (uint32_t)(a.gx * a.gy), a.band_b0, a.band_tb);
    const int tx = tile % a.gx, ty = tile / a.gx;
    const uint2 rg = a.ranges ? a.ranges[tile] : make_uint2(0u, 0u);
    p.r_lo = __builtin_amdgcn_readfirstlane((int)rg.x);
    p.r_hi = __builtin_amdgcn_readfirstlane((int)rg.y);

    // pixel-centre rectangle of this wave's quadrant, for the wave-level footprint test (scalar integers, see sgpr_opaque)
    p.iwx0 = tx * TILE + (wave & 1) * 8, p.iwy0 = ty * TILE + (wave >> 1) * 8;
    const int x = p.iwx0 + (lane & 7), y = p.iwy0 + (lane >> 3);
    p.inside = x < a.W && y < a.H;
    p.pid = (size_t)y * a.W + x;
    p.pxf = (float)x, p.pyf = (float)y;
    p.last = (p.inside && p.r_lo < p.r_hi) ? a.n_contrib[p.pid] : 0u;
    p.r_hi = min(p.r_hi, p.r_lo + (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_max_u32(p.last)));
    return p;
}

// The walk of one wave over its list, T from 1: for every entry some lane blends, entry(g, w, T, Tn, depth) with the
// wave-uniform Gaussian index, the lane's weight (0 where the lane does not blend it), its T before and behind the entry,
// and the entry's depth (DEPTH; 0 otherwise: not loaded, not staged).  Returns the lane's final T.
template <bool DEPTH, class Entry>
__device__ __forceinline__ float walk_list(const WalkArgs& a, const WalkLane& p, ContribChunk& ck, int lane, Entry&& entry) {
    // (`last` a value: read through `p`, the `pos <= last` skip becomes a branch of its own around the read of `pos`)
    const uint32_t r_lo = p.r_lo, r_hi = p.r_hi, last = p.last;
    float T = 1.0f;
    // software pipeline of the blend forward: the splat records of chunk k+1 and the list ids of chunk k+2 are requested while
    // chunk k is walked
    uint32_t n_id = 0, f_id = 0;
    float4 n_q0 = make_float4(0, 0, 0, 0), n_q1 = n_q0;
    float n_depth = 0.f;
    if (r_lo + lane < r_hi) n_id = a.point_list[r_lo + lane];
    if (r_lo + 64 + lane < r_hi) f_id = a.point_list[r_lo + 64 + lane];
    if (r_lo + lane < r_hi) {
        const SplatRec* rp = a.rec + n_id;
        n_q0 = rp->q0; n_q1 = rp->q1;
        if constexpr (DEPTH) n_depth = rp->q2.y;
    }
    for (uint32_t base = r_lo; base < r_hi; base += 64) {
        const int cnt_in = (int)min(64u, r_hi - base);
        const bool hit = lane < cnt_in && rect_hit(n_q0.x, n_q0.y, n_q0.z, n_q0.w, n_q1.x, n_q1.y, (float)sgpr_opaque(p.iwx0),
                                                   (float)sgpr_opaque(p.iwx0 + 7), (float)sgpr_opaque(p.iwy0), (float)sgpr_opaque(p.iwy0 + 7));
        const unsigned long long hmask = __ballot(hit);
        const int cnt = __popcll(hmask);
        const int slot = __popcll(hmask & ((1ull << lane) - 1ull));
        __builtin_amdgcn_wave_barrier();
        if (hit) {
            ck.geo[slot] = make_float4(n_q0.x, n_q0.y, n_q0.z * CONIC_SCALE_AC, n_q0.w * CONIC_SCALE_B);   // see splat_power2
            ck.tail[slot] = make_float4(n_q1.x * CONIC_SCALE_AC, n_q1.y, n_depth, __uint_as_float(n_id));
            ck.pos[slot] = base - r_lo + lane + 1;
        }
        __builtin_amdgcn_wave_barrier();
        n_id = f_id;
        if (base + 64 + lane < r_hi) {
            const SplatRec* rp = a.rec + n_id;
            n_q0 = rp->q0; n_q1 = rp->q1;
            if constexpr (DEPTH) n_depth = rp->q2.y;
        }
        if (base + 128 + lane < r_hi) f_id = a.point_list[base + 128 + lane];

        for (int j = 0; j < cnt; j++) {
            const float4 g0 = ck.geo[j];
            const float4 g1 = ck.tail[j];
            const uint32_t pos = ck.pos[j];
            const float dx = g0.x - p.pxf, dy = g0.y - p.pyf;
            const float power = splat_power2(dx, dy, g0.z, g0.w, g1.x);
            const float alpha = fminf(ALPHA_MAX, g1.y * __builtin_amdgcn_exp2f(power));
            const bool ok = !(power > 0.0f) && !(alpha < ALPHA_MIN) && pos <= last;
            if (!__any(ok)) continue;
            const float w = ok ? alpha * T : 0.0f;
            const float Tn = ok ? T * (1.0f - alpha) : T;
            entry((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(g1.w)), w, T, Tn, g1.z);
            T = Tn;
        }
    }
    return T;
}

struct ContribArgs {
    WalkArgs walk;
    const float* masks;           // K x H x W
    float* acc;                   // P x (K + 1), added to
    float* wmax;                  // P, max-ed into (non-negative floats: their bit patterns order like unsigned integers)
    float* alpha;                 // H x W each
    float* median_depth;
    int* ids;
    float* id_weight;
    int K;
};

// value of lane (l ^ (1 << STEP)), all 64 lanes taking part
template <int STEP>
__device__ __forceinline__ float lane_xor(float v) {
    if constexpr (STEP == 0) return dpp_get<0xB1>(v);                     // quad_perm [1,0,3,2]
    else if constexpr (STEP == 1) return dpp_get<0x4E>(v);                // quad_perm [2,3,0,1]
    else if constexpr (STEP == 2) return dpp_get<0x1B>(dpp_get<0x141>(v));   // row_half_mirror (l ^ 7), then quad_perm [3,2,1,0] (l ^ 3)
    else if constexpr (STEP == 3) return dpp_get<0x128>(v);               // row_ror:8
    else {
        // v_permlane16_swap / v_permlane32_swap of a register with itself: one result holds the even rows (the low half)
        // twice, the other the odd rows (the high half) twice - whichever of the two is not the lane's own is its partner's
        const int x = __float_as_int(v);
        if constexpr (STEP == 4) {
            const auto sw = __builtin_amdgcn_permlane16_swap(x, x, false, false);
            return __int_as_float(sw[0] ^ sw[1] ^ x);
        } else {
            const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false);
            return __int_as_float(sw[0] ^ sw[1] ^ x);
        }
    }
}

// Sums v[c] over the 64 lanes for NC columns at once.  Returns, in EVERY lane, the wave's total of column contrib_column(lane).
template <int NC, int STEP = 0>
__device__ __forceinline__ float reduce_scatter(float (&v)[NC], int lane) {
    if constexpr (NC == 1) {
        float s = v[0];
        if constexpr (STEP <= 0) s += lane_xor<0>(s);
        if constexpr (STEP <= 1) s += lane_xor<1>(s);
        if constexpr (STEP <= 2) s += lane_xor<2>(s);
        s += lane_xor<3>(s);
        s += lane_xor<4>(s);
        s += lane_xor<5>(s);
        return s;
    } else {
        constexpr int HALF = NC / 2;
        const bool hi = (lane >> STEP) & 1;
        float k[HALF];
#pragma unroll
        for (int i = 0; i < HALF; i++) {
            const float keep = hi ? v[i + HALF] : v[i];
            const float send = hi ? v[i] : v[i + HALF];
            k[i] = keep + lane_xor<STEP>(send);
        }
        return reduce_scatter<HALF, STEP + 1>(k, lane);
    }
}
// the column reduce_scatter<NC> leaves in a lane: the low log2(NC) lane bits, reversed
template <int NC>
__device__ __forceinline__ int contrib_column(int lane) {
    int c = 0;
#pragma unroll
    for (int b = 0; (1 << b) < NC; b++) c = 2 * c + ((lane >> b) & 1);
    return c;
}
__device__ __forceinline__ uint32_t wave_max_bits(float w) {
    // weights are >= 0: the float order is the order of the bit patterns
    float m = w;
    m = fmaxf(m, lane_xor<0>(m));
    m = fmaxf(m, lane_xor<1>(m));
    m = fmaxf(m, lane_xor<2>(m));
    m = fmaxf(m, lane_xor<3>(m));
    m = fmaxf(m, lane_xor<4>(m));
    m = fmaxf(m, lane_xor<5>(m));
    return __float_as_uint(m);
}

// NC: columns of `acc` carried, K + 1 rounded up to a power of two (0: no per-Gaussian sums); PIX: the per-pixel outputs (only
// the median reads an entry's depth: the walk carries it for them alone)
template <int NC, bool PIX>
__global__ void __launch_bounds__(256) contrib_kernel(ContribArgs a) {
    constexpr int NV = NC > 0 ? NC : 1;
    __shared__ __attribute__((aligned(16))) ContribChunk chunks[4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const WalkLane p = walk_setup(a.walk, lane, wave);

    float mv[NV];      // the pixel's mask values; column K carries the weight itself, the padding columns nothing
    if constexpr (NC > 0) {
        const size_t HW = (size_t)a.walk.W * a.walk.H;
#pragma unroll
        for (int c = 0; c < NC; c++) mv[c] = c < a.K ? (p.inside ? a.masks[(size_t)c * HW + p.pid] : 0.0f) : (c == a.K ? 1.0f : 0.0f);
    }

    float med = 0.0f, best_w = 0.0f;
    int best = -1;
    const float T = walk_list<PIX>(a.walk, p, chunks[wave], lane, [&](uint32_t g, float w, float T, float Tn, float depth) {
        if constexpr (PIX) {
            const float keep = med;      // (a value, not the captured reference: the choice compiles to a select)
            med = (T >= 0.5f && Tn < 0.5f) ? depth : keep;     // T only moves at a blended entry, and crosses 0.5 once
            const bool better = w > best_w;
            best = better ? (int)g : best;
            best_w = better ? w : best_w;
        }
        if constexpr (NC > 0) {
            float v[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) v[c] = w * mv[c];
            const float s = reduce_scatter<NC>(v, lane);
            const int col = contrib_column<NC>(lane);
            if (lane < NC && col <= a.K && s != 0.0f) unsafeAtomicAdd(a.acc + (size_t)g * (a.K + 1) + col, s);
        }
        if (a.wmax) {
            const uint32_t m = wave_max_bits(w);
            if (lane == 0) atomicMax(reinterpret_cast<uint32_t*>(a.wmax) + g, m);
        }
    });

    if constexpr (PIX) {
        if (p.inside) {
            if (a.alpha) a.alpha[p.pid] = 1.0f - T;
            if (a.median_depth) a.median_depth[p.pid] = med;
            if (a.ids) a.ids[p.pid] = best;
            if (a.id_weight) a.id_weight[p.pid] = best_w;
        }
    }
}

template <bool PIX>
void launch_by_columns(const ContribArgs& a, bool sums, hipStream_t s) {
    const dim3 grid(a.walk.gx * a.walk.gy), block(256);
    if (!sums) hipLaunchKernelGGL((contrib_kernel<0, PIX>), grid, block, 0, s, a);
    else if (a.K + 1 <= 1) hipLaunchKernelGGL((contrib_kernel<1, PIX>), grid, block, 0, s, a);
    else if (a.K + 1 <= 2) hipLaunchKernelGGL((contrib_kernel<2, PIX>), grid, block, 0, s, a);
    else if (a.K + 1 <= 4) hipLaunchKernelGGL((contrib_kernel<4, PIX>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((contrib_kernel<8, PIX>), grid, block, 0, s, a);
}

// ---- the label vote (f3dgs_label_votes): acc over the one-hot masks of a label map, any number of labels, in one walk ---------
//
// A pixel has one label, so of the L mask columns a wave's 64 pixels touch at most 64: the D distinct valid labels of its
// quadrant, found once per wave and numbered 0 .. D - 1 (a lane's `slot`; -1 for a lane outside the frame or with a label
// outside [0, L), which only counts in the total).  Per blended entry the columns are reduce-scattered as in contrib_kernel:
// round 0 carries slots 0 .. 6 and the weight total; each further round - a wave-uniform loop, taken while slots are left -
// eight more.  The lane a column lands in issues the atomic to acc[g][label of the slot], the slot -> label table lying in the
// wave's LDS slice.  (Rounds of two and four columns for quadrants of one to three labels - most of a real label map - were
// measured against this form on the c3 frame and made no difference: 0.427 / 0.428 ms against 0.425 / 0.410 ms.)

struct VoteArgs {
    WalkArgs walk;
    const void* labels;           // H x W, F3DGS_LABELS_U8 / _I32 / _I64
    float* acc;                   // P x (L + 1), added to
    int L, format;
};

// the pixel's label, -1 where it lies outside [0, L) - compared on the full-width value, before it is narrowed
__device__ __forceinline__ int label_at(const void* labels, int format, size_t pid, int L) {
    long long v;
    if (format == F3DGS_LABELS_U8) v = static_cast<const unsigned char*>(labels)[pid];
    else if (format == F3DGS_LABELS_I32) v = static_cast<const int32_t*>(labels)[pid];
    else v = static_cast<const long long*>(labels)[pid];
    return (v >= 0 && v < (long long)L) ? (int)v : -1;
}

__global__ void __launch_bounds__(256) label_votes_kernel(VoteArgs a) {
    __shared__ __attribute__((aligned(16))) ContribChunk chunks[4];
    __shared__ int label_of[4][64];       // per wave: slot -> label
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int* const table = label_of[wave];
    const WalkLane p = walk_setup(a.walk, lane, wave);
    if (p.r_lo >= p.r_hi) return;         // nothing listed, or nothing blended (wave-uniform; no workgroup barrier anywhere below)

    // the quadrant's distinct valid labels, in the order of their first lane: at most 64 steps
    const int label = p.inside ? label_at(a.labels, a.format, p.pid, a.L) : -1;
    int slot = -1, D = 0;
    for (unsigned long long rem = __ballot(label >= 0); rem; D++) {
        const int cur = __shfl(label, __ffsll((long long)rem) - 1, 64);
        const bool same = label == cur;
        slot = same ? D : slot;
        if (lane == 0) table[D] = cur;
        rem &= ~__ballot(same);
    }
    D = __builtin_amdgcn_readfirstlane(D);
    __builtin_amdgcn_wave_barrier();
    // round 0 (slots 0 .. 6, then the total): the place in a row of acc of the column that lands in this lane, -1: none
    const int col8 = contrib_column<8>(lane);
    int dst0 = -1;
    if (lane < 8) dst0 = col8 == 7 ? a.L : col8 < D ? table[col8] : -1;
    const size_t stride = (size_t)a.L + 1;

    walk_list<false>(a.walk, p, chunks[wave], lane, [&](uint32_t g, float w, float, float, float) {
        float* const row = a.acc + (size_t)g * stride;
        float v[8];
#pragma unroll
        for (int c = 0; c < 7; c++) v[c] = slot == c ? w : 0.0f;
        v[7] = w;
        const float s = reduce_scatter<8>(v, lane);
        if (dst0 >= 0 && s != 0.0f) unsafeAtomicAdd(row + dst0, s);
        for (int s0 = 7; s0 < D; s0 += 8) {      // wave-uniform: D lies in a scalar register
#pragma unroll
            for (int c = 0; c < 8; c++) v[c] = slot == s0 + c ? w : 0.0f;
            const float t = reduce_scatter<8>(v, lane);
            if (lane < 8 && s0 + col8 < D && t != 0.0f) unsafeAtomicAdd(row + table[s0 + col8], t);
        }
    });
}

}  // namespace

hipError_t launch_label_votes(const WalkArgs& walk, const void* labels, int format, int L, float* acc, hipStream_t s) {
    const VoteArgs a = {walk, labels, acc, L, format};
    hipLaunchKernelGGL(label_votes_kernel, dim3(walk.gx * walk.gy), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_contributions(const WalkArgs& walk, int K, const float* masks, float* acc, float* wmax, float* alpha,
                                float* median_depth, int* ids, float* id_weight, hipStream_t s) {
    const ContribArgs a = {walk, masks, acc, wmax, alpha, median_depth, ids, id_weight, K};
    const bool pix = alpha || median_depth || ids || id_weight;
    if (pix) launch_by_columns<true>(a, acc != nullptr, s); else launch_by_columns<false>(a, acc != nullptr, s);
    return hipGetLastError();
}

}  // namespace f3dgs
