// pl_phase1.h — phase 1 of the pixel-lane blend backward in its bf16 shape (render_bwd_pl.hip): sixteen list entries against
// the 64 pixels of a quadrant, lane = pixel.  Kept in a header of its own so that tools/ubench/blend_stream.hip times the very
// instruction stream the kernel runs.
//
// Semantics per (entry, pixel): R/cuda_rasterizer/backward.cu:520-617 (R = submodules/diff-gaussian-rasterization-feature) -
// alpha recomputed as in the forward (forward.cu:336-377), T walked back to front, dL/dalpha from the colour / depth sums behind.
//
// What the schedule is about (round 6; measured with tools/ubench/blend_stream.hip): one wave issues at most one instruction per
// ~5 cycles whatever the dependencies, and the compiler placed every broadcast read of a splat record right in front of its first
// use - an LDS latency (64+ cycles, more under load) exposed once per entry.  SCHED selects who orders the block:
//   0  the compiler (round 5: entry after entry, the next record requested "early" in the source, late in the ISA)
//   1  three-stage software pipeline, rows pinned with sched_barrier: while entry i's exponent is evaluated (stage B), entry
//      i - 1 takes its tests, clamp and reciprocal (stage C1) and entry i - 2 its transmittance / colour-behind recurrences, the
//      bf16 split and the stores (stage C2); records are requested a whole iteration ahead, colours eight rows ahead.
#pragma once

#include "render_common.h"

namespace f3dgs {

typedef float p1_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 p1_bf16x2 __attribute__((ext_vector_type(2)));

// One staged list entry (shared by the four waves of a tile).  Phase 1 reads q0 and q1.xy a whole entry ahead and q2 (needed
// last) in the entry's own iteration.
struct PlRec {
    float4 q0;   // mean_x, mean_y, conic_a', conic_b'   (conic pre-scaled, see splat_power2)
    float4 q1;   // conic_c', opacity, Gaussian index (bits), unused
    float4 q2;   // red, green, blue, depth
};

// BF tile layout (32 KB per tile, aliased on PlShared::wt / ::st): quadrant q at byte BF_QUAD q, term t (0: w high, 1: w middle,
// 2: s high, 3: s middle) at + BF_TERM t; each (quadrant, term) image is [64 pixels][16 entries x bf16], 32 bytes per pixel row:
// the entries of one pixel are contiguous, so a lane of phase 1 (one pixel) stores an entry pair of a term with ONE ds_write_b32,
// and phase 2 reads its A fragments (entry = M, pixel = K) transposed with ds_read_b64_tr_b16.  The 8-byte slot of pixel p's
// entries 4 c .. 4 c + 3 is bf_slot(p, c): pixel row p ^ (4 bit3(p)) - the two 32-lane halves of a transposed read take rows 8
// apart, which would meet on the same banks - and slot c ^ bits 2..3 of p, which spreads a store's 32 lanes over all 16 slot
// positions of the 128-byte ds_write bank row (2-way, the least a 32-lane ds_write_b32 can be).  Proven below.
constexpr int BF_QUAD = 8192, BF_TERM = 2048, BF_SPAN = 1024;     // BF_SPAN: the 32 pixels (K = 32) of one matrix instruction

// byte offset, inside a (quadrant, term) image, of pixel p's entries 4 c .. 4 c + 3 (p = 8 y + x of the quadrant, lane of phase 1)
constexpr uint32_t bf_slot(uint32_t p, uint32_t c) { return 32u * (p ^ (((p >> 3) & 1u) << 2)) + 8u * (c ^ ((p >> 2) & 3u)); }
// phase 1: lane p's slot of entries 0..3 in quadrant q's tiles; the pair m (entries 2 m, 2 m + 1) of a term is at ^ 4 m
constexpr uint32_t bf_store_base(uint32_t q, uint32_t p) { return q * (uint32_t)BF_QUAD + bf_slot(p, 0); }
// phase 2: the address lane l supplies to read r (0, 1) of a 16x16x32 A fragment of span 0 (span ks at + BF_SPAN ks).  Lane
// 4 i + c of the 16-lane group g gives row i of the group's 4-pixel block, entries 4 c .. 4 c + 3; lane e of the group receives
// entry e at the block's four pixels 8 g + 4 r + i, i.e. the fragment's K slots 8 g + j (j = 4 r + i) hold the pixels 8 g + j
// (32 ks + 8 g + j in the quadrant) - the order of the resident B operand.  Read 1 is read 0 ^ 0x88.
constexpr uint32_t bf_tr_ofs(uint32_t l, uint32_t r) { return bf_slot(8u * (l >> 4) + 4u * r + ((l & 15u) >> 2), l & 3u); }

namespace bf_layout_proof {
constexpr uint32_t BF_IMG = 64 * 32;
// every (pixel, entry) element of an image written exactly once, and the store address form of phase 1
constexpr bool stores_cover_the_image() {
    int hits[BF_IMG / 2] = {};
    for (uint32_t p = 0; p < 64; p++)
        for (uint32_t e = 0; e < 16; e++) {
            const uint32_t a = (bf_store_base(0, p) ^ (4u * (e >> 1))) + 2u * (e & 1u);
            if (a != bf_slot(p, e >> 2) + 2u * (e & 3u) || a >= BF_IMG) return false;
            if (bf_store_base(3, p) - bf_store_base(0, p) != 3u * BF_QUAD) return false;
            hits[a / 2]++;
        }
    for (uint32_t i = 0; i < BF_IMG / 2; i++) if (hits[i] != 1) return false;
    return true;
}
// ds_write_b32 of an entry pair: bank (a / 4) mod 32, at most two lanes of a 32-lane half on one bank
constexpr bool stores_at_most_2way() {
    for (uint32_t m = 0; m < 8; m++)
        for (uint32_t h = 0; h < 2; h++) {
            int n[32] = {};
            for (uint32_t p = 32 * h; p < 32 * h + 32; p++) n[((bf_store_base(0, p) ^ (4u * m)) / 4) % 32]++;
            for (int b = 0; b < 32; b++) if (n[b] > 2) return false;
        }
    return true;
}
// ds_read_b64_tr_b16: 8-byte aligned, bank (a / 4) mod 64, the two dwords of the 32 lanes of a half on 64 different banks
constexpr bool reads_aligned_and_conflict_free() {
    for (uint32_t ks = 0; ks < 2; ks++)
        for (uint32_t r = 0; r < 2; r++)
            for (uint32_t h = 0; h < 2; h++) {
                int n[64] = {};
                for (uint32_t l = 32 * h; l < 32 * h + 32; l++) {
                    const uint32_t a = BF_SPAN * ks + bf_tr_ofs(l, r);
                    if (a % 8 != 0 || bf_tr_ofs(l, 1) != (bf_tr_ofs(l, 0) ^ 0x88u)) return false;
                    n[(a / 4) % 64]++; n[(a / 4 + 1) % 64]++;
                }
                for (int b = 0; b < 64; b++) if (n[b] != 1) return false;
            }
    return true;
}
// store -> read round trip: element j of lane l's fragment of span ks (the transposed read's gather: lane e of a 16-lane group
// takes element e & 3 of what lane 4 i + (e >> 2) addressed, i = j & 3, in read j >> 2) is entry l & 15 at pixel 32 ks + 8 (l >> 4)
// + j as phase 1 stored it, and the 2 x 64 x 8 fragment elements touch every element of the image once
constexpr bool round_trip() {
    int hits[BF_IMG / 2] = {};
    for (uint32_t ks = 0; ks < 2; ks++)
        for (uint32_t l = 0; l < 64; l++)
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t g = l >> 4, e = l & 15u, src = 16u * g + 4u * (j & 3u) + (e >> 2);
                const uint32_t a = BF_SPAN * ks + bf_tr_ofs(src, j >> 2) + 2u * (e & 3u);
                const uint32_t p = 32u * ks + 8u * g + j;
                if (a != (bf_store_base(0, p) ^ (4u * (e >> 1))) + 2u * (e & 1u)) return false;
                hits[a / 2]++;
            }
    for (uint32_t i = 0; i < BF_IMG / 2; i++) if (hits[i] != 1) return false;
    return true;
}
static_assert(stores_cover_the_image(), "phase-1 stores: one store per (pixel, entry), inside the image");
static_assert(stores_at_most_2way(), "phase-1 ds_write_b32: at most 2-way bank conflicts");
static_assert(reads_aligned_and_conflict_free(), "ds_read_b64_tr_b16: 8-byte aligned and conflict-free per 32-lane half");
static_assert(round_trip(), "A fragment = entry x (pixel 32 ks + 8 g + j): the K order of the resident B operand");
}  // namespace bf_layout_proof

__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(p1_f32x2{lo, hi}, p1_bf16x2));
}

// Pixel state of a lane that phase 1 reads but does not change.
struct P1Pixel {
    float pxf, pyf;          // pixel centre
    uint32_t last;           // the pixel's last contributor (1-based list position; 0: none)
    float dR, dG, dB, dD;    // dL/d{red, green, blue, depth} of the pixel (first channel window only)
};

// Sixteen entries rc[0..15] (list positions pos_hi, pos_hi - 1, ...) against this lane's pixel.  T, S: transmittance and
// "colour behind" carried along the walk.  tiles + sofs: this lane's slot of entries 0..3 in the quadrant's w-high image
// (sofs = bf_store_base(quadrant, lane)).
// Returns the rows (bit e = entry e) that blended at some pixel of the wave.
// NOLDS (tools/ubench/blend_stream.hip only): four records read once per chunk stand in for all sixteen (one extra vector
// instruction per entry moves the mean) and the stores are dropped: the vector-pipe stream alone.
// S32 (the hybrid shape of the first window): s leaves as ONE fp32 value - into the quadrant's fp32 tile at s_tile + (s_ofs ^ 16 e),
// the layout of the exact-fp32 shape (render_bwd_pl.hip: PlShared) - instead of two bf16 terms; w keeps its two terms.
template <bool GEO, int SCHED, bool NOLDS = false, bool S32 = false>
__device__ __forceinline__ uint32_t pl_phase1_bf16(const PlRec* rc, const P1Pixel& px, uint32_t pos_hi, float& T, float& S,
                                                   char* tiles, uint32_t sofs, char* s_tile = nullptr, uint32_t s_ofs = 0) {
    static_assert(!S32 || (GEO && !NOLDS), "the fp32 s tile belongs to the first window");
    static_assert(ALPHA_MAX == 0.99f, "literal in the clamp below");
    uint32_t tm = 0;
    struct Ent {
        float4 g;          // mean_x, mean_y, a', b'
        float2 co;         // c', opacity
        float4 col;        // r, g, b, depth
        float dx, dy, t1, t2, pw, G, qd, v, au, al, f;
        unsigned long long m1, m2, m3;
    };
    Ent en[4];             // ring: entry e lives in en[e & 3]
    // (the pair's even entry waits in w_even / s_even for its odd neighbour; rw, rs: the pair's middle w terms, rse, rso: of s)
    float Tb = 0.f, nSf = 0.f, wv = 0.f, dLa = 0.f, sv = 0.f, rw = 0.f, rs = 0.f, w_even = 0.f, s_even = 0.f, rse = 0.f, rso = 0.f;
    uint32_t h = 0, hl = 0, hh = 0, m = 0, hs = 0, ms = 0;
    (void)nSf; (void)dLa; (void)sv; (void)rs; (void)w_even; (void)hh; (void)s_even; (void)rse; (void)rso; (void)hs; (void)ms;

    uint32_t sink = 0;
    (void)sink;
    if constexpr (NOLDS) {
        // four records read once per chunk; an entry re-uses the record of entry e - 4 with its mean moved by one instruction
        // (so that nothing of the earlier evaluation can be re-used)
#pragma unroll
        for (int k = 0; k < 4; k++) { en[k].g = rc[k].q0; en[k].co = *reinterpret_cast<const float2*>(&rc[k].q1); en[k].col = rc[k].q2; }
    }
    auto load_geo = [&](int e) {
        Ent& x = en[e & 3];
        if constexpr (NOLDS) {
            x.g.x += 0.015625f;
        } else {
            x.g = rc[e].q0; x.co = *reinterpret_cast<const float2*>(&rc[e].q1);
        }
    };
    auto load_col = [&](int e) {
        if constexpr (GEO && !NOLDS) en[e & 3].col = rc[e].q2;
    };
    // stage B: exponent and exponential, colour dot product - nothing here depends on the walk
    auto stage_b = [&](int k, int e) {
        Ent& x = en[e & 3];
        switch (k) {
            case 0: x.dx = x.g.x - px.pxf; break;
            case 1: x.dy = x.g.y - px.pyf; break;
            case 2: x.t1 = x.g.w * x.dy; break;
            case 3: x.t2 = x.co.x * x.dy; break;
            case 4: x.t1 = fmaf(x.g.z, x.dx, x.t1); break;
            case 5: x.t2 = x.t2 * x.dy; break;
            case 6: x.pw = fmaf(x.t1, x.dx, x.t2); break;                  // = splat_power2(dx, dy, a', b', c')
            case 7: x.G = __builtin_amdgcn_exp2f(x.pw); break;
            case 8: if constexpr (GEO) x.qd = x.col.w * px.dD; break;
            case 9: if constexpr (GEO) x.qd = fmaf(x.col.z, px.dB, x.qd); break;
            case 10: if constexpr (GEO) x.qd = fmaf(x.col.y, px.dG, x.qd); break;
            case 11: if constexpr (GEO) x.qd = fmaf(x.col.x, px.dR, x.qd); break;
            default: break;
        }
    };
    // stage C1: the three tests as lane masks, clamp, reciprocal of 1 - alpha (exactly 1 for skipped pairs)
    auto stage_c1 = [&](int k, int e) {
        Ent& x = en[e & 3];
        switch (k) {
            case 0: x.v = x.co.y * x.G; break;                                   // op G, not yet clamped
            case 1: x.m1 = __ballot(pos_hi - (uint32_t)e < px.last); break;
            case 2: x.m2 = __ballot(!(x.pw > 0.0f)); break;
            case 3: x.m3 = __ballot(!(x.v < ALPHA_MIN)); break;
            case 5: {
                const unsigned long long okm = x.m1 & x.m2 & x.m3;
                if (okm) tm |= 1u << e;
                // exp2 may be inf where power > 0: selected away, never multiplied.  The clamp sits in the same block: behind an
                // opaque value the compiler puts a canonicalising v_max in front of the fminf
                asm("v_cndmask_b32_e64 %0, 0, %2, %3\n\tv_min_f32_e32 %1, 0x3f7d70a4, %0" : "=&v"(x.au), "=v"(x.al) : "v"(x.v), "s"(okm));
            } break;
            case 7: x.f = 1.f - x.al; break;
            case 8: x.f = __builtin_amdgcn_rcpf(x.f); break;
            default: break;
        }
    };
    // stage C2: the recurrences of the walk; on the odd entry of a pair the two-term bf16 split of the pair and its stores.  Each
    // v_cvt_pk_bf16_f32 converts one term of two entries (even entry in the low half), so a term of the pair leaves with one
    // ds_write_b32 (see bf_slot).  The middle term is the residual of the rounded fp32 value, exact: w - hi(w).
    auto stage_c2 = [&](int k, int e) {
        Ent& x = en[e & 3];
        char* const bp = tiles + (sofs ^ (uint32_t)(4 * (e >> 1)));       // this lane's pair e >> 1, term 0
        const bool odd = e & 1;
        if constexpr (GEO) {
            switch (k) {
                case 0: Tb = T * x.f; break;                              // transmittance in front of this splat
                case 1: nSf = S * -x.f; break;
                case 2: wv = x.al * Tb; break;
                case 3: dLa = fmaf(Tb, x.qd, nSf); break;                 // dL/dalpha
                case 4: S = fmaf(wv, x.qd, S); break;
                case 5: sv = x.au * dLa; break;
                case 6:
                    if (!odd) { w_even = wv; if constexpr (!S32) s_even = sv; }
                    else { h = pack_bf16(w_even, wv); hl = h << 16; }
                    break;
                case 7: if (odd) { rw = w_even - __uint_as_float(hl); hh = h & 0xFFFF0000u; } break;
                case 8: if (odd) { rs = wv - __uint_as_float(hh); if constexpr (!S32) hs = pack_bf16(s_even, sv); } break;
                case 9: if constexpr (!S32) if (odd) { hl = hs << 16; hh = hs & 0xFFFF0000u; } break;
                case 10: if constexpr (!S32) if (odd) { rse = s_even - __uint_as_float(hl); rso = sv - __uint_as_float(hh); } break;
                case 11: if (odd) { m = pack_bf16(rw, rs); if constexpr (!S32) ms = pack_bf16(rse, rso); } break;
                case 12:
                    if constexpr (S32) {
                        if (odd) {
                            *reinterpret_cast<uint32_t*>(bp) = h;
                            *reinterpret_cast<uint32_t*>(bp + BF_TERM) = m;
                        }
                        *reinterpret_cast<float*>(s_tile + (s_ofs ^ (uint32_t)(16 * e))) = sv;
                    } else if constexpr (NOLDS) {
                        if (odd) { asm volatile("" : "+v"(h), "+v"(m), "+v"(hs), "+v"(ms)); sink = h ^ hs; }
                    } else if (odd) {
                        *reinterpret_cast<uint32_t*>(bp) = h;
                        *reinterpret_cast<uint32_t*>(bp + BF_TERM) = m;
                        *reinterpret_cast<uint32_t*>(bp + 2 * BF_TERM) = hs;
                        *reinterpret_cast<uint32_t*>(bp + 3 * BF_TERM) = ms;
                    }
                    T = Tb;
                    break;
                default: break;
            }
        } else {
            // later channel windows: the weight only
            switch (k) {
                case 0: Tb = T * x.f; break;
                case 2: wv = x.al * Tb; break;
                case 6: if (odd) h = pack_bf16(w_even, wv); break;
                case 7: if (odd) hl = h << 16; break;
                case 8: if (odd) hh = h & 0xFFFF0000u; break;
                case 9: if (odd) rw = w_even - __uint_as_float(hl); break;
                case 10: if (odd) rs = wv - __uint_as_float(hh); break;
                case 11: if (odd) m = pack_bf16(rw, rs); break;
                case 12:
                    if constexpr (NOLDS) {
                        if (odd) { asm volatile("" : "+v"(h), "+v"(m)); sink = h; } else w_even = wv;
                    } else if (odd) {
                        *reinterpret_cast<uint32_t*>(bp) = h;
                        *reinterpret_cast<uint32_t*>(bp + BF_TERM) = m;
                    } else {
                        w_even = wv;
                    }
                    T = Tb;
                    break;
                default: break;
            }
        }
    };
    constexpr int ROWS = 13;

    if constexpr (SCHED == 0) {
        // the compiler's order: entry after entry, the next record requested at the top of the entry
        load_geo(0); load_col(0);
#pragma unroll
        for (int e = 0; e < 16; e++) {
            if (e + 1 < 16) { load_geo(e + 1); load_col(e + 1); }
#pragma unroll
            for (int k = 0; k < ROWS; k++) stage_b(k, e);
#pragma unroll
            for (int k = 0; k < ROWS; k++) stage_c1(k, e);
#pragma unroll
            for (int k = 0; k < ROWS; k++) stage_c2(k, e);
        }
    } else {
        load_geo(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 16 + 2; i++) {
            if (i + 1 < 16) load_geo(i + 1);
            if (i < 16) load_col(i);
#pragma unroll
            for (int k = 0; k < ROWS; k++) {
                if (i < 16) stage_b(k, i);
                if (i >= 1 && i - 1 < 16) stage_c1(k, i - 1);
                if (i >= 2) stage_c2(k, i - 2);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if constexpr (NOLDS) tm ^= __builtin_amdgcn_readfirstlane((int)sink) & 0x10000;
    return tm;
}

}  // namespace f3dgs
