// og_celt_packed.hpp -- forms of the 20 ms reconstruction kernel that work on PACKED words (two int16 coefficients per 32-bit word,
// the lower index in the low half) instead of unpacking a group of 8 coefficients to 32 bits and packing it again: the interleave
// gather by rows, the Haar steps, the stereo merge's sums and apply pass (og_celt_recon_pm.hpp), and the synthesis' ring and tail
// writes in 16-byte pieces (og_celt.hpp).  k_celt_recon_fb is bound by vector-instruction issue; every form here is
// the same arithmetic per coefficient in wrapping 32-bit integers, so the results are the general forms' bit for bit.
//
// Written once as portable word arithmetic over four primitives -- byte permute, 2-way int16 dot product, packed 16-bit add and
// subtract -- which the device takes from the instruction set (v_perm_b32, v_dot2_i32_i16, v_pk_add_u16, v_pk_sub_u16) and the host
// restates in C.  The device runs these forms only in the tight layout (OG_RECON_TIGHT); the host emulation keeps the general forms
// and tests/emul/og_tf_undo_packed_test.cpp runs both side by side (tests/test_tf_undo_packed.py; on the GPU
// tests/test_gpu_tf_undo_packed.py).
#pragma once
#include <stddef.h>
#include "og_celt_bands.hpp"

namespace og {

#if defined(OG_RECON_TIGHT) && !defined(OG_HOST_EMUL)
constexpr bool PM_PACKED = true;
#else
constexpr bool PM_PACKED = false;
#endif

// ---- the primitives ---------------------------------------------------------------------------------------------------------------
#ifdef OG_HOST_EMUL
// byte b of the result is byte (sel >> 8 b) & 7 of the eight bytes hi:lo (selectors 0 - 7 only: the plain byte picks of v_perm_b32)
OG_DEV u32 pk_perm(u32 hi, u32 lo, u32 sel) {
    const u64 v = (u64)hi << 32 | lo;
    u32 r = 0;
    for (int b = 0; b < 4; b++) r |= (u32)((v >> (8 * ((sel >> (8 * b)) & 7u))) & 0xffu) << (8 * b);
    return r;
}
// acc + a.lo * b.lo + a.hi * b.hi, wrapping, no clamp
OG_DEV i32 pk_dot2(u32 a, u32 b, i32 acc) {
    return (i32)((u32)acc + (u32)((i32)(i16)a * (i32)(i16)b) + (u32)(((i32)a >> 16) * ((i32)b >> 16)));
}
OG_DEV i32 pk_dot2_fits(u32 a, u32 b, i32 acc) { return pk_dot2(a, b, acc); } // (the caller shows that the sum stays inside 32 bits)
OG_DEV u32 pk_add16(u32 a, u32 b) { return ((a + b) & 0xffffu) | ((a & 0xffff0000u) + (b & 0xffff0000u)); }
OG_DEV u32 pk_sub16(u32 a, u32 b) { return ((a - b) & 0xffffu) | ((a & 0xffff0000u) - (b & 0xffff0000u)); }
#else
typedef unsigned short og_u16x2 __attribute__((ext_vector_type(2)));
OG_DEV u32 pk_perm(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
OG_DEV i32 pk_dot2(u32 a, u32 b, i32 acc) { return rs_dot2(a, b, acc); }
// The same for a sum that provably stays inside 32 bits, asked for in the instruction's saturating form -- which then never saturates.
// Why: without the clamp the compiler takes the two-operand form (v_dot2c_i32_i16), which accumulates in place, and a rounding
// constant as the accumulator is then copied into the destination before every single product.  The clamp exists only in the
// three-operand form, which reads the constant where it lies.
OG_DEV i32 pk_dot2_fits(u32 a, u32 b, i32 acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(og_i16x2, a), __builtin_bit_cast(og_i16x2, b), acc, true);
}
OG_DEV u32 pk_add16(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(og_u16x2, a) + __builtin_bit_cast(og_u16x2, b)); }
OG_DEV u32 pk_sub16(u32 a, u32 b) { return __builtin_bit_cast(u32, __builtin_bit_cast(og_u16x2, a) - __builtin_bit_cast(og_u16x2, b)); }
#endif
OG_DEV u32 pk_lolo(u32 a, u32 b) { return pk_perm(b, a, 0x05040100u); } // {a.lo, b.lo}
OG_DEV u32 pk_hihi(u32 a, u32 b) { return pk_perm(b, a, 0x07060302u); } // {a.hi, b.hi}
OG_DEV u32 pk_pair(i32 lo, i32 hi) { return ((u32)lo & 0xffffu) | (u32)hi << 16; } // two values truncated to 16 bits, as st8 packs them
// {EXTRACT16(lo >> 15), EXTRACT16(hi >> 15)}: bits 15 .. 30 of either
OG_DEV u32 pk_q15(i32 lo, i32 hi) { return (((u32)lo >> 15) & 0xffffu) | (((u32)hi << 1) & 0xffff0000u); }
// {EXTRACT16(lo >> s), EXTRACT16(hi >> s)}, arithmetic shifts
OG_DEV u32 pk_shr(i32 lo, i32 hi, int s) { return pk_pair(lo >> s, hi >> s); }

// ---- a group of 8 coefficients as four words ----------------------------------------------------------------------------------------
struct W4 { u32 w[4]; };
#ifdef OG_HOST_EMUL
template <typename T>
OG_DEV T pk_ld(const i16 *p) { // (the host reads through memcpy: no alignment is assumed, the test checks the claim itself)
    T v;
    memcpy(&v, p, sizeof(T));
    return v;
}
OG_DEV W4 ldw4(const i16 *p) { return pk_ld<W4>(p); }
OG_DEV void stw4(i16 *p, const W4 &r) { memcpy(p, &r, sizeof(r)); }
#else
typedef i32 og_v4i __attribute__((ext_vector_type(4)));
template <typename T>
OG_DEV T pk_ld(const i16 *p) { return *reinterpret_cast<const T *>(p); } // naturally aligned: see pk_gather
OG_DEV W4 ldw4(const i16 *p) { // p 16-byte aligned
    const og_v4i v = *reinterpret_cast<const og_v4i *>(p);
    return W4{{(u32)v.x, (u32)v.y, (u32)v.z, (u32)v.w}};
}
OG_DEV void stw4(i16 *p, const W4 &r) { *reinterpret_cast<og_v4i *>(p) = og_v4i{(i32)r.w[0], (i32)r.w[1], (i32)r.w[2], (i32)r.w[3]}; }
#endif

#ifdef OG_HOST_EMUL
struct W2 { u32 w[2]; };
#else
struct alignas(8) W2 { u32 w[2]; }; // (one 8-byte read)
#endif

// ---- Haar steps (haar1 celt.cpp:1202; haar_pair of og_celt_recon_pm.hpp) ----------------------------------------------------------------
// One butterfly on the word {a, b}: 23170 a + 23170 b + 16384 and 23170 a - 23170 b + 16384 are one dot product each with the
// rounding term as the accumulator (|23170 a +- 23170 b| + 16384 <= 23170 * 65536 + 16384 < 2^31: the sum fits); bits 15 .. 30 are the results.
constexpr u32 HAAR_SUM = 23170u | 23170u << 16, HAAR_DIF = 23170u | (u32)(u16)(-23170) << 16;
// the butterflies (x.lo, y.lo) and (x.hi, y.hi): the pairs of a step whose stride is the distance of the two WORDS (2 or 4
// coefficients inside a group, 8 between neighbouring groups).  The sums go back to x, the differences to y.
OG_DEV void pk_haar_words(u32 &x, u32 &y) {
    const u32 p = pk_lolo(x, y), q = pk_hihi(x, y);
    x = pk_q15(pk_dot2_fits(p, HAAR_SUM, 16384), pk_dot2_fits(q, HAAR_SUM, 16384));
    y = pk_q15(pk_dot2_fits(p, HAAR_DIF, 16384), pk_dot2_fits(q, HAAR_DIF, 16384));
}
OG_DEV void pk_haar8_1(W4 &r) { // stride 1: every word is a pair
    i32 s[4], d[4]; // (all products, then all words: a product's result is not ready for the very next instruction)
#pragma unroll
    for (int m = 0; m < 4; m++) {
        s[m] = pk_dot2_fits(r.w[m], HAAR_SUM, 16384);
        d[m] = pk_dot2_fits(r.w[m], HAAR_DIF, 16384);
    }
#pragma unroll
    for (int m = 0; m < 4; m++) r.w[m] = pk_q15(s[m], d[m]);
}
OG_DEV void pk_haar8_2(W4 &r) { pk_haar_words(r.w[0], r.w[1]); pk_haar_words(r.w[2], r.w[3]); }
OG_DEV void pk_haar8_4(W4 &r) { pk_haar_words(r.w[0], r.w[2]); pk_haar_words(r.w[1], r.w[3]); }
OG_DEV void pk_haar16(W4 &a, W4 &b) { // stride 8: two neighbouring groups
#pragma unroll
    for (int m = 0; m < 4; m++) pk_haar_words(a.w[m], b.w[m]);
}

// ---- the interleave gather by rows (interleave_hadamard celt.cpp:1183) -----------------------------------------------------------------
// Group gj of a band of N coefficients at x, interleaved with stride 1 << ls: the group's eight interleaved indices 8 gj + k are
// coefficient j = (8 gj + k) >> ls of row i = (8 gj + k) & (stride - 1) of the blocked layout, row i starting at
// x + row(i) n0, n0 = N >> ls, row(i) = ordery(stride, i) for a long block (`had`) and i otherwise.  For stride <= 8 that is
// 8 >> ls CONSECUTIVE coefficients from each of `stride` rows:
//   stride 2: j = 4 gj .. 4 gj + 3   two 8-byte reads     stride 4: j = 2 gj, 2 gj + 1   four 4-byte reads     stride 8: j = gj   eight 2-byte reads
// With x 16-byte aligned and N a multiple of 8 (every band of a 20 ms frame is 8 x its 5 ms width, and starts at 8 x its 5 ms edge),
// n0 is a multiple of 8 >> ls, so every read is naturally aligned (tests/emul/og_tf_undo_packed_test.cpp walks the band table).
// Any other stride takes the general element-by-element form.
static_assert(V_X % 8 == 0 && 960 % 8 == 0, "a channel's spectrum starts 16-byte aligned, its bands at multiples of 8 coefficients");
OG_DEV W4 pk_gather(const i16 *x, int N, int gj, int ls, bool had) {
    W4 r;
    if (ls == 2) {
        const int n0 = N >> 2;
        const i16 *p = x + 2 * gj;
        const u32 r0 = pk_ld<u32>(p + (had ? 3 : 0) * n0), r1 = pk_ld<u32>(p + (had ? 0 : 1) * n0);
        const u32 r2 = pk_ld<u32>(p + 2 * n0), r3 = pk_ld<u32>(p + (had ? 1 : 3) * n0);
        r.w[0] = pk_lolo(r0, r1);
        r.w[1] = pk_lolo(r2, r3);
        r.w[2] = pk_hihi(r0, r1);
        r.w[3] = pk_hihi(r2, r3);
    } else if (ls == 3) {
        const int n0 = N >> 3;
        const i16 *p = x + gj;
        const u32 rows = had ? 0x25163407u : 0x76543210u; // ordery(8, i) in nibble i, or the identity
#pragma unroll
        for (int m = 0; m < 4; m++)
            r.w[m] = (u32)pk_ld<u16>(p + (int)((rows >> (8 * m)) & 15u) * n0) | (u32)pk_ld<u16>(p + (int)((rows >> (8 * m + 4)) & 15u) * n0) << 16;
    } else if (ls == 1) {
        const int n0 = N >> 1;
        const i16 *p = x + 4 * gj;
        const W2 a = pk_ld<W2>(p + (had ? n0 : 0)), b = pk_ld<W2>(p + (had ? 0 : n0));
        r.w[0] = pk_lolo(a.w[0], b.w[0]);
        r.w[1] = pk_hihi(a.w[0], b.w[0]);
        r.w[2] = pk_lolo(a.w[1], b.w[1]);
        r.w[3] = pk_hihi(a.w[1], b.w[1]);
    } else {
        const int stride = 1 << ls, n0 = N >> ls;
        i32 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int inter = 8 * gj + k, j = inter >> ls, i = inter & (stride - 1);
            v[k] = x[(had ? ordery(stride, i) : i) * n0 + j];
        }
#pragma unroll
        for (int m = 0; m < 4; m++) r.w[m] = pk_pair(v[2 * m], v[2 * m + 1]);
    }
    return r;
}

// ---- stereo merge (stereo_merge celt.cpp:1113; pm_stereo_merge of og_celt_recon_pm.hpp) ------------------------------------------------
// a group's partial sums: xp += sum y x, side += sum y y -- wrapping sums of 16 x 16 products either way
OG_DEV void pk_merge_sums(const W4 &a, const W4 &b, i32 &xp, i32 &side) {
#pragma unroll
    for (int m = 0; m < 4; m++) {
        xp = pk_dot2(b.w[m], a.w[m], xp);
        side = pk_dot2(b.w[m], b.w[m], side);
    }
}
// The apply pass on a group (not the copy mode): l = EXTRACT16(MULT16_16_P15(mid, x)); x' = EXTRACT16(PSHR32(MULT16_16(lgain, l - r),
// kl + 1)), y' = EXTRACT16(PSHR32(MULT16_16(rgain, l + r), kr + 1)), y' negated when `inv`.  l - r and l + r feed MULT16_16, which
// takes their low 16 bits: the packed 16-bit difference and sum are those bits.  A product of one half of a word with a gain, plus
// its rounding term, is one dot product against {gain, 0} or {0, gain}: one 16 x 16 product, at most 2^30 in size, and a rounding
// term of at most 2^15 (the shifts are kl + 1, kr + 1 <= 16): the sums fit 32 bits.
OG_DEV void pk_merge_apply(W4 &a, W4 &b, i32 mid, i32 lgain, i32 rgain, int kl, int kr, bool inv) {
    const u32 m_lo = (u32)mid & 0xffffu, m_hi = (u32)mid << 16;
    const u32 l_lo = (u32)lgain & 0xffffu, l_hi = (u32)lgain << 16, r_lo = (u32)rgain & 0xffffu, r_hi = (u32)rgain << 16;
    const i32 rl = (1 << (kl + 1)) >> 1, rr = (1 << (kr + 1)) >> 1;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const u32 l = pk_q15(pk_dot2_fits(a.w[m], m_lo, 16384), pk_dot2_fits(a.w[m], m_hi, 16384));
        const u32 d = pk_sub16(l, b.w[m]), s = pk_add16(l, b.w[m]);
        a.w[m] = pk_shr(pk_dot2_fits(d, l_lo, rl), pk_dot2_fits(d, l_hi, rl), kl + 1);
        const u32 y = pk_shr(pk_dot2_fits(s, r_lo, rr), pk_dot2_fits(s, r_hi, rr), kr + 1);
        b.w[m] = inv ? pk_sub16(0u, y) : y;
    }
}
OG_DEV W4 pk_neg(const W4 &a) { return W4{{pk_sub16(0u, a.w[0]), pk_sub16(0u, a.w[1]), pk_sub16(0u, a.w[2]), pk_sub16(0u, a.w[3])}}; }

// ---- the synthesis' history ring and overlap tail in 16-byte pieces (celt_synthesis, og_celt.hpp) ----------------------------------------
// The ring head is a multiple of 8 samples (it starts at 0 and moves by a frame, 120 << LM samples, at a time) and the ring holds
// 2,048, so a piece of 4 samples from a head + 4 p never straddles the wrap and is 16-byte aligned in the ring (CeltState aligns
// it to 128 bytes); the synthesis buffer and the overlap tail are 16-byte aligned too.
static_assert(RING % 8 == 0 && 120 % 8 == 0 && OVERLAP / 2 % 4 == 0, "ring pieces of 4 samples: whole, and never across the wrap");
static_assert(offsetof(CeltState, ring) % 16 == 0 && offsetof(CeltState, tail) % 16 == 0 && sizeof(CeltState) % 16 == 0 &&
              sizeof(((CeltState *)nullptr)->tail[0]) % 16 == 0, "the ring and the tails are 16-byte aligned");
static_assert(V_SYN % 8 == 0, "the synthesis buffer is 16-byte aligned in the working set");
struct P4 { i32 v[4]; };
OG_DEV P4 pk_ld4(const i32 *p) {
#ifdef OG_HOST_EMUL
    P4 r;
    memcpy(&r, p, sizeof(r));
    return r;
#else
    const og_v4i v = *reinterpret_cast<const og_v4i *>(p);
    return P4{{v.x, v.y, v.z, v.w}};
#endif
}
OG_DEV void pk_st4(i32 *p, const P4 &r) {
#ifdef OG_HOST_EMUL
    memcpy(p, &r, sizeof(r));
#else
    *reinterpret_cast<og_v4i *>(p) = og_v4i{r.v[0], r.v[1], r.v[2], r.v[3]};
#endif
}
// out_syn[0 .. n) to the ring at `pos`, out_syn[n .. n + OVERLAP / 2) to the tail (n a multiple of 8, pos a multiple of 8)
OG_DEV void pk_ring_tail_store(i32 *ring, i32 *tail, const i32 *sy, int pos, int n) {
    OG_FOR_LANES(p, n / 4) pk_st4(&ring[(pos + 4 * p) & RING_MASK], pk_ld4(&sy[4 * p]));
    OG_FOR_LANES(p, OVERLAP / 2 / 4) pk_st4(&tail[4 * p], pk_ld4(&sy[n + 4 * p]));
}

} // namespace og
