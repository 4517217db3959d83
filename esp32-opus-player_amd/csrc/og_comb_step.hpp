// og_comb_step.hpp -- the steps of the in-place pitch comb filter (comb_filter, og_celt.hpp) as the device runs them: up to 64
// consecutive samples per step, one per lane, never more than the lag allows.  k_celt_recon_fb is bound by vector-instruction issue
// (DESIGN.md 6n), so a step is the filter's arithmetic and as little else as the instruction set permits:
//   * the tap gains past the cross-fade are the wave's and stay in scalar registers (mul16x32_q15_u);
//   * a lane that holds no sample of the step computes with whatever it reads -- only its store is left out -- so nothing is
//     initialised for it and no read is predicated; every read, a dead lane's included, stays inside the buffer or the ring;
//   * where a step's 68-sample window lies (buffer, ring, across) is the wave's: each class reads its five taps at constant offsets
//     from ONE lane address that is the sum of a per-call lane term and a scalar;
//   * a cross-fade step takes its window word through a 32-bit lane offset from the table's scalar address.
// Written once over a memory policy M: the device's (CombDev, below) takes the instruction forms, the test's
// (tests/emul/og_comb_step_test.cpp) runs the 64 lanes one after the other on the host, checks every read's bounds and is held,
// sample for sample, against comb_filter's OG_HOST_EMUL loop (tests/test_comb_step.py).  What M provides:
//   lane_begin() / lane_end()   the lanes this caller runs (the device: its own)
//   y0(p0, lane)                buffer sample p0 + lane                                   (p0 + lane < SYN_LEN)
//   buf_taps(i0, lane)          CombTaps of buffer samples i0 + lane .. i0 + lane + 4     (i0 >= 0)
//   ring_taps(h0, lane)         CombTaps of ring words h0 + lane .. h0 + lane + 4         (h0 + 67 <= RING_MASK)
//   mixed_taps(first, lane, last_live)  the same window where it crosses from the ring into the buffer or over the ring's end
//   win(i)                      rom_win120[i]                                             (0 <= i < OVERLAP)
//   store(p0, lane, y)          buffer sample p0 + lane = y (a live lane)
//   sync()                      the steps are ordered
#pragma once
#include "og_common.hpp"
#include "og_state.hpp"

namespace og {

// e[0] .. e[4] of a lane: x[p - T - 2] .. x[p - T + 2]
struct CombTaps { i32 e[5]; };
struct CombGains { i32 g00, g01, g02, g10, g11, g12; };

// One call of the filter (comb_filter celt.cpp:848) on N samples: from lag T0, gain g0, tapset tap0 to T1, g1, tap1.
//   * tap gains: gains[tapset][0..2] Q15 (celt.cpp:854) times the filter's gain, rounded;
//   * a call whose two filters are the same has no cross-fade; with g1 == 0 only the cross-fade changes the signal;
//   * every tap that COUNTS lies >= T - 2 samples back: that many samples can be filtered without looking at each other's results.
//     A filter whose gain is zero contributes exactly zero (its tap gains are zero, so is every product), so its lag does not
//     limit the step and its taps are not fetched -- a frame that switches the post-filter on cross-fades from "off" at the
//     minimum lag 15, which would cut the cross-fade into steps of 13.  Past the cross-fade only T1 counts.
struct CombCall {
    int T0, T1, overlap, end, chunk_fade, chunk_rest;
    bool use0, use1;
    CombGains g;
};
OG_DEV CombCall comb_call(int T0, int T1, int N, i32 g0, i32 g1, int tap0, int tap1) {
    CombCall q;
    q.T0 = T0 = OG_MAX(T0, 15);
    q.T1 = T1 = OG_MAX(T1, 15);
    const i32 ga0 = tap0 == 0 ? 10048 : tap0 == 1 ? 15200 : 26208, ga1 = tap0 == 0 ? 7112 : tap0 == 1 ? 8784 : 3280, ga2 = tap0 == 0 ? 4248 : 0;
    const i32 gb0 = tap1 == 0 ? 10048 : tap1 == 1 ? 15200 : 26208, gb1 = tap1 == 0 ? 7112 : tap1 == 1 ? 8784 : 3280, gb2 = tap1 == 0 ? 4248 : 0;
    q.g.g00 = tr16(mul16_p15(g0, ga0)); q.g.g01 = tr16(mul16_p15(g0, ga1)); q.g.g02 = tr16(mul16_p15(g0, ga2));
    q.g.g10 = tr16(mul16_p15(g1, gb0)); q.g.g11 = tr16(mul16_p15(g1, gb1)); q.g.g12 = tr16(mul16_p15(g1, gb2));
    q.overlap = (g0 == g1 && T0 == T1 && tap0 == tap1) ? 0 : OVERLAP;
    q.use0 = g0 != 0;
    q.use1 = g1 != 0;
    q.chunk_fade = OG_MIN(q.use0 ? T0 : 1 << 20, q.use1 ? T1 : 1 << 20) - 2;
    q.chunk_rest = T1 - 2;
    q.end = g1 == 0 ? q.overlap : N;
    return q;
}

// where the 68-sample window of a step lies whose lane 0 reads sample `first` (< 0: history, relative to the ring head)
enum { COMB_WIN_BUF = 0, COMB_WIN_RING = 1, COMB_WIN_MIXED = 2 };
OG_DEV int comb_win_class(int first, int ring_pos, int ring_mask) {
    if (first >= 0) return COMB_WIN_BUF;
    const int head = (ring_pos + first) & ring_mask;
    return (first + 67 < 0 && head + 67 <= ring_mask) ? COMB_WIN_RING : COMB_WIN_MIXED;
}
// a step's length: any run of at most T - 2 samples is independent of its own results
// (OG_SCALAR: the value is the wave's and is to stay in scalar registers where the compiler sees a cheaper vector form -- a
// three-way minimum exists only there, and a lane offset added first makes a 64-bit vector address of a scalar one)
#ifdef OG_HOST_EMUL
#define OG_SCALAR(x) ((void)0)
#else
#define OG_SCALAR(x) asm("" : "+s"(x))
#endif
OG_DEV int comb_step_len(int base, int overlap, int chunk_fade, int chunk_rest, int end) {
    int chunk = OG_MIN(base < overlap ? chunk_fade : chunk_rest, 64);
    OG_SCALAR(chunk);
    return OG_MIN(chunk, end - base);
}

// MULT16_32_Q15 whose 16-bit operand is the wave's, already sign-extended: it stays in a scalar register (v_mad_i64_i32 is VOP3
// and reads one; mul16x32_q15's "v" costs a v_mov_b32 per product wherever the gain lives in one)
#ifdef OG_HOST_EMUL
OG_DEV i32 mul16x32_q15_u(i32 a, i32 b) { return (i32)(((i64)a * (i64)b) >> 15); }
#else
OG_DEV i32 mul16x32_q15_u(i32 a, i32 b) {
    i64 p;
    u64 carry;
    asm("v_mad_i64_i32 %0, %1, %2, %3, 0" : "=v"(p), "=s"(carry) : "s"(a), "v"(b));
    return (i32)(p >> 15);
}
#endif

// past the cross-fade: y0 + g10 x[p - T1] + g11 (x[p - T1 + 1] + x[p - T1 - 1]) + g12 (x[p - T1 + 2] + x[p - T1 - 2])
OG_DEV i32 comb_y_rest(i32 y0, const CombTaps &a, i32 g10, i32 g11, i32 g12) {
    return clampsym(y0 + mul16x32_q15_u(g10, a.e[2]) + mul16x32_q15_u(g11, a.e[3] + a.e[1]) + mul16x32_q15_u(g12, a.e[4] + a.e[0]), SIG_SAT);
}
// A cross-fade sample: window entry wf, f = wf^2, the old filter's gains times 32767 - f and the new one's times f, each product
// its own truncation as in the reference.  (wf is a table entry, 0 .. 32767: f and 32767 - f are 0 .. 32767 and a gain product is
// no larger than its gain, so every EXTRACT16 of the general form is the identity here.)  `in_fade` false -- a lane of the
// cross-fade's last step that lies behind it: the old filter's three products are products with zero, the new one's gains are g1x.
OG_DEV i32 comb_y_fade(i32 y0, const CombTaps &a, const CombTaps &b, i32 wf, bool in_fade, const CombGains &g) {
    const i32 f = mul16_q15(wf, wf);
    const i32 nf = in_fade ? 32767 - f : 0;
    const i32 G00 = mul16_q15(nf, g.g00), G01 = mul16_q15(nf, g.g01), G02 = mul16_q15(nf, g.g02);
    const i32 F10 = mul16_q15(f, g.g10), F11 = mul16_q15(f, g.g11), F12 = mul16_q15(f, g.g12);
    const i32 G10 = in_fade ? F10 : g.g10, G11 = in_fade ? F11 : g.g11, G12 = in_fade ? F12 : g.g12;
    return clampsym(y0 + mul16x32_q15(G00, b.e[2]) + mul16x32_q15(G01, b.e[3] + b.e[1]) + mul16x32_q15(G02, b.e[4] + b.e[0]) +
                        mul16x32_q15(G10, a.e[2]) + mul16x32_q15(G11, a.e[3] + a.e[1]) + mul16x32_q15(G12, a.e[4] + a.e[0]),
                    SIG_SAT);
}

// the five taps of `lane` at lag T in the step that starts at buffer sample p0 (lanes up to last_live hold a sample)
template <class M>
OG_DEV CombTaps comb_window(M &m, int lane, int p0, int T, int last_live, int ring_pos, int ring_mask) {
    const int first = p0 - T - 2;
    const int cls = comb_win_class(first, ring_pos, ring_mask);
    if (cls == COMB_WIN_BUF) return m.buf_taps(first, lane);
    if (cls == COMB_WIN_RING) return m.ring_taps((ring_pos + first) & ring_mask, lane);
    return m.mixed_taps(first, lane, last_live);
}

// The cross-fade's steps, base 0 up to the first step that starts at or behind `overlap`; which of the two filters has a gain is
// the wave's and the template's: a filter without one fetches no taps, its products -- with gains of zero -- read the other's.
template <bool USE0, bool USE1, class M>
OG_DEV int comb_fade_steps(M &m, int off, const CombCall &q, int ring_pos, int ring_mask) {
    static_assert(USE0 || USE1, "a call without gains does not filter");
    const int T0 = q.T0, T1 = q.T1, overlap = q.overlap;
    const CombGains &g = q.g;
    int base = 0;
    for (int lim; base < overlap && base < q.end; base += lim) {
        lim = comb_step_len(base, overlap, q.chunk_fade, q.chunk_rest, q.end);
        m.sync();
        const int p0 = off + base;
        const bool mixed = base + 64 > overlap; // (a lane behind the cross-fade: only possible in its last step)
        for (int lane = m.lane_begin(); lane < m.lane_end(); lane++) {
            const i32 y0 = m.y0(p0, lane);
            const i32 wf = m.win(OG_MIN(base + lane, overlap - 1));
            const CombTaps a = USE1 ? comb_window(m, lane, p0, T1, lim - 1, ring_pos, ring_mask) : comb_window(m, lane, p0, T0, lim - 1, ring_pos, ring_mask);
            const CombTaps b = !USE1 ? a : USE0 ? comb_window(m, lane, p0, T0, lim - 1, ring_pos, ring_mask) : a;
            const i32 y = mixed ? comb_y_fade(y0, a, b, wf, base + lane < overlap, g) : comb_y_fade(y0, a, b, wf, true, g);
            if (lane < lim) m.store(p0, lane, y);
        }
    }
    return base;
}

// One call of the filter on buffer samples [off, off + q.end): the cross-fade over the first q.overlap of them (0: none), then the
// new filter alone.  (q.use1 holds wherever q.end > q.overlap.)
template <class M>
OG_DEV void comb_steps(M &m, int off, const CombCall &q, int ring_pos, int ring_mask) {
    int base = 0;
    if (q.overlap > 0) {
        if (q.use0 && q.use1)
            base = comb_fade_steps<true, true>(m, off, q, ring_pos, ring_mask);
        else if (q.use1)
            base = comb_fade_steps<false, true>(m, off, q, ring_pos, ring_mask);
        else
            base = comb_fade_steps<true, false>(m, off, q, ring_pos, ring_mask);
    }
    for (int lim; base < q.end; base += lim) {
        lim = comb_step_len(base, q.overlap, q.chunk_fade, q.chunk_rest, q.end);
        m.sync();
        const int p0 = off + base;
        for (int lane = m.lane_begin(); lane < m.lane_end(); lane++) {
            const i32 y0 = m.y0(p0, lane);
            const CombTaps a = comb_window(m, lane, p0, q.T1, lim - 1, ring_pos, ring_mask);
            const i32 y = comb_y_rest(y0, a, q.g.g10, q.g.g11, q.g.g12);
            if (lane < lim) m.store(p0, lane, y);
        }
    }
}

// (a census program's hook into comb_filter -- tests/emul/og_comb_census_main.cpp; nothing anywhere else)
#ifndef OG_COMB_CENSUS
#define OG_COMB_CENSUS(q, off, ring_pos) ((void)0)
#endif

#ifndef OG_HOST_EMUL
// The device's memory: explicit address spaces (two generic pointers would be folded back into one flat load), every address a
// per-call lane term plus a scalar, so that a step costs one vector add per window and the loads take their constant offsets.
#define OG_AS_LDS __attribute__((address_space(3)))
#define OG_AS_GLB __attribute__((address_space(1)))
struct CombDev {
    u32 buf_lane;                 // LDS byte address of buffer sample `lane`
    u32 lane4;                    // 4 * lane
    const OG_AS_GLB char *ring;   // the channel's history ring (the wave's: scalar registers)
    const OG_AS_GLB char *win120; // rom_win120
    int ring_pos;
    int ring_mask;
    OG_MEMBER int lane_begin() const { return OG_LANE; }
    OG_MEMBER int lane_end() const { return OG_LANE + 1; }
    OG_MEMBER static void sync() { OG_SYNC(); }
    OG_MEMBER const OG_AS_LDS i32 *buf_at(int i0) const { return (const OG_AS_LDS i32 *)(buf_lane + 4u * (u32)i0); }
    OG_MEMBER i32 y0(int p0, int) const { return *buf_at(p0); }
    OG_MEMBER void store(int p0, int, i32 y) const { *(OG_AS_LDS i32 *)(buf_lane + 4u * (u32)p0) = y; }
    OG_MEMBER CombTaps buf_taps(int i0, int) const {
        const OG_AS_LDS i32 *e = buf_at(i0);
        return CombTaps{{e[0], e[1], e[2], e[3], e[4]}};
    }
    OG_MEMBER CombTaps ring_taps(int h0, int) const {
        const OG_AS_GLB char *r0 = ring + 4u * (u32)h0;
        OG_SCALAR(r0);
        const OG_AS_GLB i32 *e = (const OG_AS_GLB i32 *)(r0 + lane4);
        return CombTaps{{e[0], e[1], e[2], e[3], e[4]}};
    }
    OG_MEMBER i32 win(int i) const { return *(const OG_AS_GLB i16 *)(win120 + 2u * (u32)i); }
    OG_MEMBER i32 tap_at(int idx) const { // buffer or ring by the sample's sign: the buffer read is unconditional, its index clamped
        i32 v = *(const OG_AS_LDS i32 *)(buf_lane - lane4 + 4u * (u32)OG_MAX(idx, 0));
        if (idx < 0) v = *(const OG_AS_GLB i32 *)(ring + 4u * (u32)((ring_pos + idx) & ring_mask));
        return v;
    }
    // Lane l fetches e[4] of its window only (clamped to the step's last live sample); the other four arrive by shifting that
    // register one lane at a time (DPP wave_shr:1), with e[3] .. e[0] of lane 0 (fetched by lanes 0 .. 3) fed in at lane 0.
    OG_MEMBER CombTaps mixed_taps(int first, int lane, int last_live) const {
        CombTaps t;
        t.e[4] = tap_at(first + OG_MIN(lane, last_live) + 4);
        const i32 w = tap_at(first + (lane & 3));
        t.e[3] = __builtin_amdgcn_update_dpp(__builtin_amdgcn_readlane(w, 3), t.e[4], 0x138, 0xf, 0xf, false);
        t.e[2] = __builtin_amdgcn_update_dpp(__builtin_amdgcn_readlane(w, 2), t.e[3], 0x138, 0xf, 0xf, false);
        t.e[1] = __builtin_amdgcn_update_dpp(__builtin_amdgcn_readlane(w, 1), t.e[2], 0x138, 0xf, 0xf, false);
        t.e[0] = __builtin_amdgcn_update_dpp(__builtin_amdgcn_readlane(w, 0), t.e[1], 0x138, 0xf, 0xf, false);
        return t;
    }
};
#endif

} // namespace og
