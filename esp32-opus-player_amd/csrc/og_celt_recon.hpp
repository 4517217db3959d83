// og_celt_recon.hpp -- the split CELT path's second stage, one frame per WAVE: the PVQ leaf pass with its rotations, the band loop's
// vector half (the general band walk here, the phase-major one of 20 ms frames in og_celt_recon_pm.hpp), synthesis and stream
// bookkeeping; and the third stage's entry, celt_post.  (og_celt_rec.hpp says why the frame splits, and holds the record.)
#pragma once
#include "og_celt.hpp"
#include "og_celt_rec.hpp"

namespace og {

// One PVQ leaf, lane-private (alg_unquant celt.cpp:782): codeword index -> signed pulse vector (cwrsi :2545),
// scaled to the leaf's gain (normalise_residual :745), spreading rotation undone (exp_rotation :707, dir = -1),
// collapse mask (extract_collapse_mask :760).  Everything is a serial chain per leaf, so the frame's leaves run
// one per lane; the result is written in place at S.v[pos .. pos+n).  Returns the collapse mask.
// The spreading rotation exp_rotation1 (celt.cpp:684) sweeps i = 0 .. len-stride-1 forward, then len-2*stride-1 .. 0 backward, over
// pairs (i, i+stride).  Pairs with different i mod stride never touch the same element, so each residue class ("chain") is walked
// on its own, carrying the element both consecutive steps share in a register: one LDS read and one write per step.  A wave runs
// the walk for 64 leaves in lock-step and pays for the longest: (a) a step's two outputs are each one v_dot2_i32_i16 -- c x1 + s x2
// + 16384 with the pair (x1, x2) packed in one register -- and a shift; (b) four steps at a time, their four new elements requested
// together before the first result is stored (a store to the spectrum keeps the compiler from moving the next element's read above
// it, so step by step every element costs an LDS round trip); (c) the backward sweep starts where the forward one counted to (no
// remainder to divide out).  The host emulation runs the same walk (tests/test_rotation_chain.py holds it against the two plain
// sweeps): only the two instructions are spelled out for it.
#ifdef OG_HOST_EMUL
OG_DEV i32 rot_dot2(u32 pair, u32 coef, i32 half) { // (lo . lo + hi . hi + half) >> 15, the sum in wrapping 32-bit arithmetic
    return (i32)((u32)mul16((i32)pair, (i32)coef) + (u32)mul16((i32)(pair >> 16), (i32)(coef >> 16)) + (u32)half) >> 15;
}
OG_DEV u32 rot_pack(i32 lo, i32 hi) { return ((u32)lo & 0xffffu) | (u32)hi << 16; } // low halves of both
#else
OG_DEV i32 rot_dot2(u32 pair, u32 coef, i32 half) {
    i32 r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(pair), "v"(coef), "v"(half));
    return r >> 15;
}
OG_DEV u32 rot_pack(i32 lo, i32 hi) { return __builtin_amdgcn_perm((u32)hi, (u32)lo, 0x05040100u); } // low halves of both
#endif
// one chain r, r + stride, r + 2 stride, .. of exp_rotation1 (celt.cpp:684): forward, then backward
OG_DEV void rotate_chain(i16 *const p0, int r, int len, int stride, u32 k_a, u32 k_b) {
    const i32 half = 16384;
    // forward along the chain: pairs (i, i + stride) while i < len - stride
    int i = r, steps = 0;
    i32 x1 = p0[i];
    for (; i + 3 * stride < len - stride; i += 4 * stride, steps += 4) {
        const i32 e1 = p0[i + stride], e2 = p0[i + 2 * stride], e3 = p0[i + 3 * stride], e4 = p0[i + 4 * stride];
        u32 pk = rot_pack(x1, e1);
        const i32 o0 = rot_dot2(pk, k_a, half);
        x1 = rot_dot2(pk, k_b, half);
        pk = rot_pack(x1, e2);
        const i32 o1 = rot_dot2(pk, k_a, half);
        x1 = rot_dot2(pk, k_b, half);
        pk = rot_pack(x1, e3);
        const i32 o2 = rot_dot2(pk, k_a, half);
        x1 = rot_dot2(pk, k_b, half);
        pk = rot_pack(x1, e4);
        const i32 o3 = rot_dot2(pk, k_a, half);
        x1 = rot_dot2(pk, k_b, half);
        p0[i] = (i16)o0;
        p0[i + stride] = (i16)o1;
        p0[i + 2 * stride] = (i16)o2;
        p0[i + 3 * stride] = (i16)o3;
    }
    for (; i < len - stride; i += stride, steps++) {
        const u32 pk = rot_pack(x1, p0[i + stride]);
        p0[i] = (i16)rot_dot2(pk, k_a, half);
        x1 = rot_dot2(pk, k_b, half);
    }
    p0[i] = (i16)x1;
    // backward: pairs (i, i + stride) from the chain's highest i <= len - 2 stride - 1 down to r -- one pair fewer than forward
    if (steps >= 2) {
        i -= 2 * stride; // (forward ended on the chain's last element, r + steps * stride)
        i32 x2 = p0[i + stride];
        for (; i - 3 * stride >= 0; i -= 4 * stride) {
            const i32 e1 = p0[i], e2 = p0[i - stride], e3 = p0[i - 2 * stride], e4 = p0[i - 3 * stride];
            u32 pk = rot_pack(e1, x2); // (x1, x2) = (element i, carried): second output goes to i + stride, first is carried down
            const i32 o0 = rot_dot2(pk, k_b, half);
            x2 = rot_dot2(pk, k_a, half);
            pk = rot_pack(e2, x2);
            const i32 o1 = rot_dot2(pk, k_b, half);
            x2 = rot_dot2(pk, k_a, half);
            pk = rot_pack(e3, x2);
            const i32 o2 = rot_dot2(pk, k_b, half);
            x2 = rot_dot2(pk, k_a, half);
            pk = rot_pack(e4, x2);
            const i32 o3 = rot_dot2(pk, k_b, half);
            x2 = rot_dot2(pk, k_a, half);
            p0[i + stride] = (i16)o0;
            p0[i] = (i16)o1;
            p0[i - stride] = (i16)o2;
            p0[i - 2 * stride] = (i16)o3;
        }
        for (; i >= 0; i -= stride) {
            const u32 pk = rot_pack(p0[i], x2);
            p0[i + stride] = (i16)rot_dot2(pk, k_b, half);
            x2 = rot_dot2(pk, k_a, half);
        }
        p0[r] = (i16)x2;
    }
}
OG_DEV void rotate1_lane(i16 *xv, int x, int len, int stride, i32 c, i32 s) { // exp_rotation1 celt.cpp:684
    const u32 k_a = rot_pack(c, -s), k_b = rot_pack(s, c); // first output: c x1 - s x2; second (carried on): s x1 + c x2
    for (int r = 0; r < stride; r++) {
        if (r >= len - stride) break; // (the chains are in order: no later one has a pair either)
        rotate_chain(xv + x, r, len, stride, k_a, k_b);
    }
}

// A leaf's spreading rotation, put off to the wave pass below (on == false: the leaf has none).
struct RotJob {
    int x, blen, logB, stride2; // first coefficient, block length, log2 of the block count, the wide stride (0: only stride 1)
    i32 c, s;
    bool on;
};
#ifndef OG_HOST_EMUL // (needs 64 lanes)
// The rotations of the (up to 64) leaves the lanes of a wave have just decoded, by the WHOLE wave.  One leaf per lane costs the wave
// its largest rotated leaf's 4 N serial steps with eight lanes busy (a frame of the bench payloads rotates 8 of its 48 leaves:
// 103 steps for the largest on average).  But exp_rotation (celt.cpp:707) is B independent blocks, and its wide-stride sweep
// is `stride2` independent chains per block (rotate1_lane): here every (leaf, block, chain) of the wide sweeps gets a lane of its
// own (6 steps for the longest chain instead of 50), then every (leaf, block) one for the stride-1 sweep, which is serial (47
// steps).  How an item finds its leaf: the leaves' item counts are prefix-summed over the wave; a leaf's lane marks the first
// of its items in a 64-byte row of LDS with its own number, a prefix maximum over that row names every item's leaf, and the
// leaf's job comes over the lane crossbar.  All 64 lanes call this together.
OG_DEV void pvq_rotate_wave(i16 *xv, const RotJob &j, u8 *marker) {
    if (!__any(j.on)) return;
    const int lane = OG_LANE;
    const int w_geo = j.x | j.blen << 16, w_par = j.logB | j.stride2 << 8;
    const int w_cs = (int)((u32)(u16)j.c | (u32)(u16)j.s << 16);
    for (int pass = 0; pass < 2; pass++) { // the wide stride first (exp_rotation with dir = -1)
        int chains = 0;
        if (j.on) chains = pass == 0 ? (j.stride2 ? OG_MAX(0, OG_MIN(j.stride2, j.blen - j.stride2)) : 0) : (j.blen >= 2);
        const int cnt = chains << j.logB; // items: chain r of block b is item r << logB | b
        const int incl = wave_scan_add(cnt), excl = incl - cnt;
        const int total = __builtin_amdgcn_readlane(incl, 63);
        for (int base = 0; base < total; base += 64) {
            marker[lane] = 0;
            OG_LSYNC();
            if (cnt > 0 && excl < base + 64 && incl > base) marker[OG_MAX(excl - base, 0)] = (u8)(lane + 1);
            OG_LSYNC();
            const int leaf = wave_scan_max((int)marker[lane]) - 1; // (>= 0: item `base` belongs to some leaf)
            const int item = base + lane;
            const bool work = item < total;
            const int src = leaf < 0 ? lane : leaf;
            const int g = __shfl(w_geo, src), q = __shfl(w_par, src), cs = __shfl(w_cs, src), first = __shfl(excl, src);
            if (work) {
                const int logB = q & 255, sub = item - first, b = sub & ((1 << logB) - 1), r = sub >> logB;
                const int blen = g >> 16;
                const i32 c = (i32)(i16)(cs & 0xffff), sn = (i32)(i16)(cs >> 16);
                i16 *const p0 = xv + (g & 0xffff) + b * blen;
                const i32 cc = pass == 0 ? sn : c, ss = pass == 0 ? c : sn; // exp_rotation1(.., stride2, s, c), then (.., 1, c, s)
                rotate_chain(p0, r, blen, pass == 0 ? q >> 8 : 1, rot_pack(cc, -ss), rot_pack(ss, cc));
            }
            OG_LSYNC();
        }
    }
}
#endif

// U(a, b) for the leaf pass.  64 lanes walking 64 different leaves ask for 64 unrelated entries per step: from global
// memory that is one cache line per lane and the texture path serialises them (measured: a third of the walk at best, with
// the dense table evicted from L1 by the streaming traffic all the time).  Here rows 0..3 are closed forms and rows 4..14
// sit in LDS, stored by ROW with every column (rom_pvq_rr / rom_pvq_rb, 2.8 KB over the folding-history, pulse and scratch rows,
// none of which is in use during the leaf pass): U(r, c) = rr[rb[r] + c] for r = 4 .. 14 and any c.  Round 2 stored columns (one base per dimension n,
// fetched a step ahead); what the walk spends its time on since zero runs are skipped is the SEARCH for the next pulse's
// dimension at a fixed number of pulses k, i.e. along rows k and k + 1: with rows, a probe is two independent reads off two
// bases that change only when k does (a column base per probe made it two dependent round trips), a pulse's size candidates
// (rows 4..7 at column n) need no base at all, and the two entries of a step with n <= k are neighbours in row n.
#ifdef OG_RECON_TIGHT
// (og_state.hpp: rows 4 - 8 behind X, rows 9 - 11 and 12 - 14 in the two 320-byte tops of the spectrum that no band reaches -- a row's
// base is an offset from the table's first word, negative for those)
constexpr int PVQ_MAIN_LEN = ROM_PVQ_RB9, PVQ_TOP0_OFF = (X_TOP0 - V_NORM) / 2, PVQ_TOP1_OFF = (X_TOP1 - V_NORM) / 2;
static_assert((ROM_PVQ_RB12 - ROM_PVQ_RB9) * 2 <= 160 && (ROM_PVQ_RR_LEN - ROM_PVQ_RB12) * 2 + 32 <= 160, "the short rows (and the rotation marker) fit the tops");
#else
constexpr int PVQ_MAIN_LEN = ROM_PVQ_RR_LEN;
#endif
struct PvqLds {
    u32 rr[PVQ_MAIN_LEN];
    i16 rb[16];
    OG_MEMBER u32 at(int i) const { return reinterpret_cast<const u32 *>(this)[i]; } // entry i of the table (row base + column)
};
OG_DEV int pvq_lds_index(int t) { // where entry t of rom_pvq_rr lies, as an index from the table's first word
#ifdef OG_RECON_TIGHT
    return t < ROM_PVQ_RB9 ? t : t < ROM_PVQ_RB12 ? t - ROM_PVQ_RB9 + PVQ_TOP0_OFF : t - ROM_PVQ_RB12 + PVQ_TOP1_OFF;
#else
    return t;
#endif
}
#ifdef OG_RECON_TIGHT
static_assert(sizeof(PvqLds) <= (V_JOBM - V_NORM) * 2, "the PVQ table's long rows end before the jobs' collapse masks");
#else
static_assert(sizeof(PvqLds) <= (V_TOTAL - V_NORM) * 2, "the PVQ table overlays the folding-history, pulse and scratch rows");
#endif
OG_DEV PvqLds &pvq_lds() { return *reinterpret_cast<PvqLds *>(&S.v[V_NORM]); }
OG_DEV void pvq_tab_load() { // (the caller synchronises)
    u32 *const dst = reinterpret_cast<u32 *>(&pvq_lds());
#ifdef OG_HOST_EMUL
    OG_FOR_LANES(t, ROM_PVQ_RR_LEN) dst[pvq_lds_index(t)] = rom_pvq_rr[t];
    OG_FOR_LANES(t, 16) pvq_lds().rb[t] = (i16)pvq_lds_index(rom_pvq_rb[t]);
#else
    // every load requested before the first store waits for its data (a load - wait - store loop pays the L2's latency per pass)
    constexpr int NRR = (ROM_PVQ_RR_LEN + OG_NLANES - 1) / OG_NLANES;
    u32 rr[NRR];
#pragma unroll
    for (int k = 0; k < NRR; k++) rr[k] = rom_pvq_rr[OG_MIN(OG_LANE + k * OG_NLANES, ROM_PVQ_RR_LEN - 1)];
    const u16 rb = rom_pvq_rb[OG_LANE & 15];
#pragma unroll
    for (int k = 0; k < NRR; k++)
        if (OG_LANE + k * OG_NLANES < ROM_PVQ_RR_LEN) dst[pvq_lds_index(OG_LANE + k * OG_NLANES)] = rr[k];
    if (OG_LANE < 16) pvq_lds().rb[OG_LANE] = (i16)pvq_lds_index((int)rb);
#endif
}
// U(r, h) for a row r <= 3 (<= h), given U(2, h) and U(3, h); written without branches on purpose: the lanes of a wave
// ask for different rows, and as control flow every row would cost the wave a pass of its own
OG_DEV u32 pvq_row_sel(int r, u32 v2, u32 v3) {
    u32 v = (u32)(r >= 1);
    v = r == 2 ? v2 : v;
    return r == 3 ? v3 : v;
}
// U(3, h) = 2 h (h - 1) + 1 and the integer root the k = 2 zero run needs.  On the GPU: one 24-bit multiply-add (the compiler's own
// form of the expression is two masks and a full 32-bit multiply), and the bare v_sqrt_f32 -- one ulp, where the precise sqrtf is a
// dozen instructions of rounding fix-ups: its argument is below 2^15 here (tq <= 176^2), where neighbouring integers' roots are
// 0.0028 apart at least and a float's ulp is 2^-16, so the truncated result is the root's floor, or one less when the root is an
// integer -- which the caller's upward correction covers.  (tests/test_gpu_device_forms.py runs both on the GPU over their whole
// domain, h < 2^11 and tq <= 176^2: on an MI355X the root came out as the floor everywhere)
#ifdef OG_HOST_EMUL
OG_DEV u32 pvq_u3(u32 h) { return 2u * h * (h - 1u) + 1u; }
OG_DEV int pvq_isqrt_near(u32 tq) { return (int)__builtin_sqrtf((float)tq); }
#else
OG_DEV u32 pvq_u3(u32 h) { // h < 2^11
    u32 r;
    const u32 a = h << 1, b = h - 1u;
    asm("v_mad_u32_u24 %0, %1, %2, 1" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
OG_DEV int pvq_isqrt_near(u32 tq) { return (int)__builtin_amdgcn_sqrtf((float)tq); }
#endif
// Which of a leaf's blocks (of `blen` coefficients each) coefficient j lies in, without a division per pulse: j / blen is
// (j * M) >> 16 for M = floor(65536 / blen) + 1 -- or that plus one -- whenever j < 176 and blen <= 176 (the error j (M - 65536 /
// blen) / 65536 stays below 1 / blen; tests/test_pvq_walk_sites.py walks every j, blen and both M).  On the GPU M comes from the
// reciprocal instruction: one ulp, and 65536 / blen is an integer (exactly represented, blen a power of two) or at least
// 1 / blen away from one, which is 80 times the error of the product -- so the truncation is the floor.  (Which M the GPU takes,
// and pvq_block_of with it for every j and blen: tests/test_gpu_device_forms.py; the smaller one everywhere on an MI355X.)
#ifdef OG_HOST_EMUL
OG_DEV u32 pvq_block_mul(int blen) { return blen > 0 ? 65536u / (u32)blen + 1u : 0u; }
OG_DEV int pvq_block_of(int j, u32 mul) { return (int)(((u32)j * mul) >> 16); }
#else
OG_DEV u32 pvq_block_mul(int blen) { return (u32)(65536.0f * __builtin_amdgcn_rcpf((float)blen)) + 1u; }
OG_DEV int pvq_block_of(int j, u32 mul) { return (int)(__umul24((u32)j, mul) >> 16); } // (175 * 65537 < 2^24)
#endif
OG_DEV int pvq_row_base(const PvqLds &T, int r) { return (int)T.rb[r < 4 ? 4 : (r > 14 ? 14 : r)]; } // (rows outside 4..14 are not table rows)

// `xv`: the spectrum arena of the leaf's frame (the calling wave's own working set -- or another wave's when the leaves of the
// workgroup's frames are pooled, og_recon.hip); `T`: the table copy to walk.
// `defer`: the leaf's rotation is not done here but described there, for pvq_rotate_wave (the caller cleared defer->on)
OG_DEV u32 pvq_leaf_lane(i16 *xv, const PvqLds &T, int n, int k, u32 i, int pos, int B, i32 gain, int spread, RotJob *defer = nullptr) {
    const int N = n, K = k, x = pos;
    const int logB = ilog2(B), blen = N >> logB; // B is a power of two
    i32 yy = 0;
    // The collapse mask -- which of the B blocks hold a pulse -- is gathered where the pulses are stored: the walk stores every
    // non-zero itself, so the spectrum need not be read back for it.
    const u32 bmul = pvq_block_mul(blen);
    u32 cm = 0;
    // cwrsi celt.cpp:2545.  The reference has two code paths (k >= n: "lots of pulses", k < n: "lots of dimensions")
    // that differ only in how they walk its triangular table; with U(a, b) available for any pair both are
    //   s = (i >= U(n, k+1));  i -= s ? U(n, k+1) : 0;  k' = max { k' <= k : U(n, k') <= i };  value = +-(k - k');  i -= U(n, k')
    // The lanes of a wave decode different leaves and the wave waits for its longest one -- a leaf of many dimensions and
    // few pulses: its runs of zeros are skipped in one go (below), so a step of such a leaf places a pulse.  Steps with n <= k
    // take the general form below it.  The spectrum was cleared before the leaf pass: zeros are not stored.
    OG_MARK(56);
    int b0 = pvq_row_base(T, k), b1 = pvq_row_base(T, k + 1); // where rows k and k + 1 start (while they are table rows)
    while (n > 2) {
        if (k == 0) break; // every pulse is placed: what is left of the leaf stays zero
        u32 h = (u32)n, v2 = 2u * h - 1u, v3 = pvq_u3(h); // U(2, n), U(3, n)
        const bool sparse = n > k;
        u32 p0, p1;         // U(n, k), U(n, k + 1)
        int bn = 0;         // (n <= k) where row n starts
        bool tab = false;   // (n <= k) row n is a table row (n == 3: closed form)
        if (sparse) {
            const u32 c0 = T.at(k >= 4 ? b0 + n : 0), c1 = T.at(k >= 3 ? b1 + n : 0);
            p0 = k >= 4 ? c0 : pvq_row_sel(k, v2, v3);
            p1 = k >= 3 ? c1 : pvq_row_sel(k + 1, v2, v3);
            // A sparse leaf (many dimensions, few pulses) is mostly runs of zeros, and the wave waits for its longest leaf: the run is
            // skipped in one go.  With V(a) = U(a, k) + U(a, k + 1) the dimensions n, n-1, .., a+1 all decode to zero exactly when
            //     V(n) - V(a) <= 2 i < V(n) + V(a)          (one comparison: V(a) >= m, see below)
            // (the zero steps subtract U(n, k), U(n-1, k), ..: their sum down to a+1 is (V(n) - V(a)) / 2 by the recurrence
            // U(t, k+1) = U(t-1, k+1) + U(t, k) + U(t-1, k); the other bound is the one that keeps every step's sign test false);
            // V grows with a, so the smallest such a is found by bisection along rows k and k + 1.  Then i -= (V(n) - V(a)) / 2 and
            // the walk goes on at dimension a -- with a pulse, unless the search range ended there.
            // (tools/pvq_zero_run.py checks the identity against the step-by-step walk.)  Everything fits 32 bits: V(n) is the
            // size of a legal codebook, i < V(n), and with t = V(n) - i the two bounds in one read
            //     V(a) >= m,   m = i >= t ? i - t + 1 : t - i          (= d >= 0 ? d + 1 : -d for d = 2 i - V(n))
            // (skipped whenever n > k.  Measured, k_celt_recon_fb alone / pipelined step: no skip 1.869 / 2.525 ms, this 1.825 / 2.49,
            // only from n > 2 k on 1.891, 3 k 1.899, 4 k 1.898; the wave's walk is 34 steps on average without, 10 with)
            if (k <= 13 && n > k && n > 3) {
                const u32 Vn = p0 + p1, t = Vn - i, m = i >= t ? i - t + 1u : t - i;
                const int lo0 = k + 1 > 2 ? k + 1 : 2;
                int a;
                u32 t0 = p0, t1 = p1; // U(k, a), U(k + 1, a) of the dimension a the run ends at: the step below needs no second look
                if (k <= 2) { // V(a, 1) = 2 a and V(a, 2) = 2 a^2: solved, not searched (m <= V(n) <= 2 * 176^2)
                    const u32 tq = (m + 1u) >> 1;
                    int r = (int)tq;
                    if (k == 2) {
                        r = pvq_isqrt_near(tq);  // the root's floor, or one less (tq <= 176^2): its ceiling after
                        r += (u32)(r * r) < tq; // the correction
                    }
                    a = r > lo0 ? r : lo0;
                    const u32 u2 = 2u * (u32)a - 1u;
                    t0 = k == 1 ? 1u : u2;
                    t1 = k == 1 ? u2 : pvq_u3((u32)a);
                } else {
                    int lo = lo0, hi = n;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        const u32 m0 = T.at(k >= 4 ? b0 + mid : 0), m1 = T.at(b1 + mid);
                        const u32 a0 = k >= 4 ? m0 : pvq_u3((u32)mid); // (row 3 in closed form)
                        if (a0 + m1 >= m) {
                            hi = mid;
                            t0 = a0;
                            t1 = m1;
                        } else
                            lo = mid + 1;
                    }
                    a = lo;
                }
                if (a < n) { // (a > k: the step below is still one with more dimensions than pulses)
                    i -= (Vn - (t0 + t1)) >> 1;
                    pos += n - a;
                    n = a;
                    if (n <= 2) break;
                    h = (u32)n;
                    v2 = 2u * h - 1u;
                    v3 = pvq_u3(h);
                    p0 = t0;
                    p1 = t1;
                }
            }
        } else { // n <= k: everything this step reads lies in row n, whose columns are all in LDS (n == 3: U(3, c) = 2 c (c - 1) + 1)
            const u32 hk = (u32)k;
            bn = pvq_row_base(T, n);
            tab = n >= 4;
            const u32 a0 = T.at(tab ? bn + k : 0), a1 = T.at(tab ? bn + k + 1 : 0);
            p0 = tab ? a0 : pvq_u3(hk);
            p1 = tab ? a1 : pvq_u3(hk + 1u);
        }
        const int s = -(int)(i >= p1);
        i -= p1 & (u32)s;
        if (p0 <= i && s == 0) {
            i -= p0;
        } else { // a pulse: the largest k' < k with U(n, k') <= i (U(n, 0) = 0 <= i; U(n, k) > i here)
            // ONE bisection for every lane of the wave (a wave of unrelated leaves has takers for each form of this search at
            // nearly every step, and runs one loop after the other, each to its own deepest lane: DESIGN 6g).  A lane with n <= k
            // searches along row n, columns 0 .. k - 1.  A lane with n > k searches the rows at column n, and only the table
            // rows 4 .. k - 1 (rows from k on are not looked at: a row ends where its entries leave 32 bits, and only U(k, n) and
            // the entries below it are known to exist): "3" stands for "no table row passes", and then the closed forms of rows
            // 1 .. 3 are compared at once below the loop.  What differs between the two kinds is a probe's address.
            u32 plo = 0;
            const bool tabp = sparse || tab; // the probes read the table (not so: row 3 in closed form)
            const int off = sparse ? n : bn;
            int lo = sparse ? OG_MIN(3, k - 1) : 0, hi = k - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1; // >= 1 (n > k: >= 4)
                const int rbm = pvq_row_base(T, mid);
                const u32 tm = T.at(tabp ? (sparse ? rbm : mid) + off : 0);
                const u32 pm = tabp ? tm : pvq_u3((u32)mid);
                if (pm <= i) {
                    lo = mid;
                    plo = pm;
                } else
                    hi = mid - 1;
            }
            int kk = lo;
            if (sparse && lo <= 3) { // U(., n) grows with the row: the last of rows 1 .. 3 (below k) that passes, or none
                const u32 cand[3] = {1u, v2, v3};
                kk = 0;
#pragma unroll
                for (int r = 1; r <= 3; r++) {
                    const bool ok = r < k && cand[r - 1] <= i;
                    kk = ok ? r : kk;
                    plo = ok ? cand[r - 1] : plo;
                }
            }
            const int val = (k - kk + s) ^ s;
            k = kk;
            i -= plo;
            xv[pos] = (i16)val; // (never zero: k' < k)
            cm |= 1u << pvq_block_of(pos - x, bmul);
            yy += val * val;
            b0 = pvq_row_base(T, k); // (rows k and k + 1, for the steps with more dimensions than pulses)
            b1 = pvq_row_base(T, k + 1);
        }
        pos++;
        n--;
    }
    {
        const u32 p = 2 * (u32)k + 1;
        int s = -(int)(i >= p);
        i -= p & (u32)s;
        const int k0 = k;
        k = (int)((i + 1) >> 1);
        if (k) i -= 2 * (u32)k - 1;
        int val = (k0 - k + s) ^ s;
        xv[pos] = (i16)val;
        cm |= (u32)(val != 0) << pvq_block_of(pos - x, bmul);
        pos++;
        yy += val * val;
        s = -(int)i;
        val = (k + s) ^ s;
        xv[pos] = (i16)val;
        cm |= (u32)(val != 0) << pvq_block_of(pos - x, bmul);
        yy += val * val;
    }
#ifdef OG_PVQ_WALK_TAP // (host emulation, tests/emul/og_pvq_walk_kat.cpp: the pulses and their energy, before they are scaled)
    OG_PVQ_WALK_TAP(xv + x, N, yy);
#endif
    // collapse mask: the blocks seen above (coefficients past B * blen, if any, belong to no block)
    OG_MARK(57);
    cm = B > 1 ? cm & ((1u << B) - 1u) : 1u;
    // scale the pulses in place
    OG_MARK(58);
    const int kk = ilog2(yy) >> 1;
    const i32 t = vshr32(yy, 2 * (kk - 7));
    const i32 g = tr16(mul16_p15(rsqrt_norm(t), gain));
    for (int j = 0; j < N; j++) xv[x + j] = (i16)pshr32(mul16(g, xv[x + j]), kk + 1);
    OG_MARK(59);
    if (2 * K < N && spread != 0) {
        const int factor = spread == 1 ? 15 : (spread == 2 ? 10 : 5);
        const i32 rg = tr16(mul32_q31(mul16(32767, N), celt_rcp(N + factor * K))); // celt_div celt.h:367
        const i32 theta = tr16(mul16_q15(rg, rg) >> 1);
        const i32 c = cos_norm(theta), s = cos_norm(sub16(32767, theta));
        int stride2 = 0;
        if (N >= 8 * B) {
            stride2 = 1;
            while ((stride2 * stride2 + stride2) * B + (B >> 2) < N) stride2++;
        }
        if (defer) {
            defer->x = x;
            defer->blen = blen;
            defer->logB = logB;
            defer->stride2 = stride2;
            defer->c = c;
            defer->s = s;
            defer->on = true;
            return cm;
        }
        for (int blk2 = 0; blk2 < B; blk2++) {
            if (stride2) rotate1_lane(xv, x + blk2 * blen, blen, stride2, s, c);
            rotate1_lane(xv, x + blk2 * blen, blen, 1, c, s);
        }
    }
    return cm;
}

// The collapse mask of a PVQ leaf goes, pre-shifted, into its JOB's word (S.job_mask_row(): 2 x band + decode slot; cleared by
// recon_begin) -- a job's mask is the OR of its leaves' (cm(job) |= cm(leaf) << off, see parse_tree).  Round 5: a row of one mask
// per LEAF (416 x u16) was a tenth of the reconstruction kernel's LDS; the lanes of a round's leaves OR into the row together.
OG_DEV void job_mask_or(int job, u32 m) {
#ifdef OG_HOST_EMUL
    S.job_mask_row()[job] |= m;
#else
    __hip_atomic_fetch_or(&S.job_mask_row()[job], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
}

// The record's word stream is consumed strictly in order: a 64-word window in LDS, refilled by one coalesced load.
constexpr int REC_WORDS_CAP = (REC_MAX_WORDS + 64) / 64 * 64; // size of ParseRec::words
struct RecCur { // read positions in the record: next word, first word of the window in LDS (-64: none), next PVQ leaf
    const u32 *words;
    int w, base, leaf;
};
OG_DEV u32 rec_word(RecCur &cur) {
    if ((unsigned)(cur.w - cur.base) >= 64u) { // the window moves to the word wanted (the sequential walk: every 64 words)
        OG_STAT(26, 1);                             // window refills at the point of use
        OG_LSYNC();
        OG_FOR_LANES(l, 64) S.word_window()[l] = cur.words[OG_MIN(cur.w + l, REC_WORDS_CAP - 1)];
        OG_LSYNC();
        cur.base = cur.w;
    }
    const u32 w = (u32)OG_UNI(S.word_window()[cur.w - cur.base]);
    cur.w++;
    return w;
}

// Four consecutive words (a band's header): when they lie inside the current window -- 15 times out of 16 -- the four LDS
// reads have no refill check between them and issue together (one latency instead of four).
OG_DEV void rec_word4(RecCur &cur, u32 &w0, u32 &w1, u32 &w2, u32 &w3) {
    const int at = cur.w - cur.base;
    if (at >= 0 && at <= 60) {
        const u32 *win = S.word_window();
        const u32 a = win[at], b = win[at + 1], c = win[at + 2], d = win[at + 3];
        w0 = (u32)OG_UNI(a);
        w1 = (u32)OG_UNI(b);
        w2 = (u32)OG_UNI(c);
        w3 = (u32)OG_UNI(d);
        cur.w += 4;
        return;
    }
    w0 = rec_word(cur);
    w1 = rec_word(cur);
    w2 = rec_word(cur);
    w3 = rec_word(cur);
}

// The noise generator jumped ahead by j + 1 steps: s -> a s + c.  The jumps by 1 .. 192 steps are constants (rom_lcg_jump,
// tools/gen_rom_tables.py): a noise sample reads its pair from there, one multiply-add per coefficient.
// (Rounds 2 - 3 kept the wave's six values in this object; the compiler put the object in scratch memory and turned at()'s
// selects into indexed loads from it -- two trips to memory per sample where this is one, and the kernel's only scratch
// traffic: 2 KB per frame written and read back through HBM.)
struct LcgTab {
    OG_MEMBER u32 at(u32 seed, int j) const { // seed advanced by (j + 1) steps, 0 <= j < 192
        const u32 a = rom_lcg_jump[2 * j], c = rom_lcg_jump[2 * j + 1];
        return a * seed + c;
    }
#if defined(OG_RECON_TIGHT) && !defined(OG_HOST_EMUL)
    // The 20 ms kernel: a lane loop's first pass has j = the lane's index, the same pair for every fill leaf of the frame.  hold()
    // requests it once (two registers, nothing indexed: see above); entries from 64 on stay loads at their use.
    u32 a_lane, c_lane;
    OG_MEMBER void hold() {
        a_lane = rom_lcg_jump[2 * OG_LANE];
        c_lane = rom_lcg_jump[2 * OG_LANE + 1];
    }
    OG_MEMBER u32 at_lane(u32 seed, int j) const { // at(seed, j) for j = lane + a multiple of 64, after hold()
        if (j < OG_NLANES) return a_lane * seed + c_lane;
        return at(seed, j);
    }
#else
    OG_MEMBER void hold() {}
    OG_MEMBER u32 at_lane(u32 seed, int j) const { return at(seed, j); }
#endif
};

// anti_collapse (celt.cpp:1010) for the reconstruction kernel of 20 ms frames.  The shared form (og_celt_bands.hpp) derives a band's
// noise amplitude r -- a division, an exp2, a reciprocal square root -- in every lane alike, up to 42 times one after the other (the
// values come from LDS rows: vector work, not scalar), and steps the noise generator with its squaring loop per lane: a frame with
// anti-collapse (one in sixteen of the bench payloads) cost the wave 60 % more than one without.  Here lane (channel, band) derives
// its own r, one pass for all of them, into a scratch row (anti_collapse_r); the fills read it back and jump the generator by the
// frame's table -- band by band here, in whole-wave passes in the 20 ms kernel's own layout (og_celt_recon_pm.hpp).
OG_DEV i16 *anti_collapse_r(int LM, int C, int start, int end) { // -> r of (channel c, band i) at [c * NBANDS + i]
    i16 *const rrow = &S.v[V_TMP]; // (the band loop's scratch row: free by now)
    OG_LSYNC();
    OG_FOR_LANES(l, C * NBANDS) {
        const int c = l >= NBANDS ? 1 : 0, i = l - c * NBANDS;
        i32 r = 0;
        if (i >= start && i < end) {
            const int N0 = rom_eband[i + 1] - rom_eband[i];
            const int depth = (int)(udiv((u32)(1 + S.pulses_row()[i]), (u32)N0) >> LM);
            const i32 thresh32 = celt_exp2(-shl16(depth, 10 - BITRES)) >> 1;
            const i32 thresh = tr16(mul16x32_q15(16384, OG_MIN(32767, thresh32)));
            i32 t = N0 << LM;
            const int shift = ilog2(t) >> 1;
            t = shl32(t, (7 - shift) << 1);
            const i32 sqrt_1 = rsqrt_norm(t);
            i32 prev1 = S.logE1_row()[c * NBANDS + i], prev2 = S.logE2_row()[c * NBANDS + i];
            if (C == 1) {
                prev1 = OG_MAX(prev1, (i32)S.logE1_row()[NBANDS + i]);
                prev2 = OG_MAX(prev2, (i32)S.logE2_row()[NBANDS + i]);
            }
            i32 Ediff = (i32)S.bandE_row()[c * NBANDS + i] - OG_MIN(prev1, prev2);
            Ediff = OG_MAX(0, Ediff);
            if (Ediff < 16384) {
                const i32 r32 = celt_exp2(-tr16(Ediff)) >> 1;
                r = tr16(2 * OG_MIN(16383, r32));
            }
            if (LM == 3) r = tr16(mul16_q14(23170, OG_MIN(23169, r)));
            r = tr16(OG_MIN(thresh, r) >> 1);
            r = tr16(mul16_q15(sqrt_1, r) >> shift);
        }
        rrow[l] = (i16)r;
    }
    OG_LSYNC();
    return rrow;
}
#ifndef OG_RECON_TIGHT // (the 20 ms kernel's own: og_celt_recon_pm.hpp)
OG_DEV void anti_collapse_pm(const LcgTab &lcg, int LM, int C, int size, int start, int end, u32 seed) {
    const i16 *const rrow = anti_collapse_r(LM, C, start, end);
    for (int i = start; i < end; i++) {
        const int N0 = rom_eband[i + 1] - rom_eband[i];
        for (int c = 0; c < C; c++) {
            const i32 r = (i32)OG_UNI(rrow[c * NBANDS + i]);
            const int x = V_X + c * size + (rom_eband[i] << LM);
            int renorm = 0;
            const u32 mask = (u32)OG_UNI(S.cmask_row()[i * C + c]);
            for (int k = 0; k < 1 << LM; k++) {
                if (!(mask & (1u << k))) {
                    OG_LSYNC();
                    OG_FOR_LANES(j, N0) S.v[x + (j << LM) + k] = (i16)((lcg.at(seed, j) & 0x8000) ? r : -r);
                    seed = lcg_skip(seed, (u32)N0);
                    renorm = 1;
                }
            }
            if (renorm) renormalise(x, N0 << LM, 32767);
        }
    }
}
#endif

// The leaves of one job (quant_partition celt.cpp:1382 flattened by the parse kernel), vector half.  The leaves with
// pulses are complete already (pvq_leaf_lane) and only contribute their collapse masks, which the leaf pass ORed, pre-shifted,
// into the job's word of S.job_mask_row() (`job`: 2 x band + decode slot).  A leaf without pulses is zeroed, noise-filled or folded from the lower band
// (celt.cpp:1481-1520).  `jw`: the job's header word.  Returns the job's collapse mask.
OG_DEV u32 recon_job_leaves(RecCur &cur, const LcgTab &lcg, u32 jw, u32 &seed_io, int x_job, int low_job, i32 fill_job, int job) {
    const int n_fill = (int)(jw & 31), n_pvq = (int)(jw >> JW_NPVQ_SHIFT) & 31;
    u32 cm_job = n_pvq ? (u32)OG_UNI(S.job_mask_row()[job]) : 0u;
    for (int f = 0; f < n_fill; f++) {
        OG_MARK(7);
        const u32 w = rec_word(cur), w1 = rec_word(cur);
        const int off = (int)(w >> LW_OFF_SHIFT) & 15, B = ((int)(w >> LW_B_SHIFT) & 15) + 1, N = (int)(w >> LW_N_SHIFT) & 255;
        const int x = V_X + (int)(w1 & 2047);
        const i32 gain = (i32)((w1 >> 11) & 0xffff);
        const u32 cm_mask = (u32)((1ull << B) - 1);
        const i32 fill = (i32)((u32)(fill_job >> off) & cm_mask);
        OG_STAT(10, fill == 0);                     // fill leaves left zero
        OG_STAT(11, fill != 0 && low_job < 0);      // ... noise
        OG_STAT(12, fill != 0 && low_job >= 0);     // ... folded
        if (fill) { // (no fill: the leaf stays zero, as the spectrum was initialised)
            const u32 seed = seed_io;
            u32 cm;
            OG_LSYNC();
            if (low_job < 0) { // noise
                OG_FOR_LANES(j, N) S.v[x + j] = (i16)((i32)lcg.at_lane(seed, j) >> 20);
                cm = cm_mask;
            } else { // folded spectrum, +-1/256 dither
                const int low = low_job + (x - x_job);
                OG_FOR_LANES(j, N) S.v[x + j] = (i16)(S.v[low + j] + ((lcg.at_lane(seed, j) & 0x8000) ? 4 : -4));
                cm = (u32)fill;
            }
            seed_io = lcg_skip(seed, (u32)N);
            renormalise(x, N, gain);
            cm_job |= cm << off;
        }
        OG_MARK(6);
    }
    return cm_job;
}

// Haar / Hadamard helpers with power-of-two strides taken as shifts (no integer division in the lane loops)
OG_DEV void haar1_p2(int x, int N0, int log_stride) { // haar1 celt.cpp:1202, stride = 1 << log_stride
    N0 >>= 1;
    const int stride = 1 << log_stride;
    OG_LSYNC();
    OG_FOR_LANES(id, N0 << log_stride) {
        const int j = id >> log_stride, i = id & (stride - 1);
        const int a = x + stride * 2 * j + i, b = a + stride;
        const i32 t1 = mul16(23170, S.v[a]), t2 = mul16(23170, S.v[b]);
        S.v[a] = (i16)pshr32(t1 + t2, 15);
        S.v[b] = (i16)pshr32(t1 - t2, 15);
    }
    OG_LSYNC();
}
// (de)interleave_hadamard celt.cpp:1162 / :1183; stride = 1 << log_stride.  Lanes enumerate the interleaved index.
OG_DEV void hadamard_p2(int x, int N0, int log_stride, int hadamard, int dir) {
    const int stride = 1 << log_stride, N = N0 << log_stride;
    OG_LSYNC();
    OG_FOR_LANES(inter, N) {
        const int j = inter >> log_stride, i = inter & (stride - 1);
        const int blocked = (hadamard ? ordery(stride, i) : i) * N0 + j;
        if (dir == 0)
            S.v[V_TMP + blocked] = S.v[x + inter];
        else
            S.v[V_TMP + inter] = S.v[x + blocked];
    }
    OG_LSYNC();
    OG_FOR_LANES(id, N) S.v[x + id] = S.v[V_TMP + id];
    OG_LSYNC();
}

// quant_band celt.cpp:1526, vector half; N > 1.  `scale`: sqrt(N) for the folding history (from the record).
OG_DEV u32 recon_band_mono(RecCur &cur, u32 jw, const LcgTab &lcg, int tf_change, u32 &seed, int x, int N, int B, int low, int low_out,
                           i32 scale, int low_scratch, i32 fill, int job) {
    const int N0 = N, longBlocks = B == 1;
    int logB = ilog2(B), time_divide = 0, recombine = 0;
    int N_B = N >> logB;
    OG_STAT(1, 1);                                  // jobs
    OG_STAT(2, (jw & JW_NEED_LOW) && low >= 0);     // jobs that prepare a folding source
    OG_STAT(3, (int)(jw & 31));                     // fill leaves
    OG_STAT(4, (int)(jw >> JW_NPVQ_SHIFT) & 31);    // PVQ leaves
    OG_STAT(5, tf_change != 0);                     // jobs with a tf change
    OG_STAT(6, B > 1);                              // jobs in short-block frames
    if (!(jw & JW_NEED_LOW)) low = -1; // no leaf of this job folds: skip the whole preparation of the folding source
    if (tf_change > 0) recombine = tf_change;
    if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {
        OG_LSYNC();
        OG_FOR_LANES(j, N) S.v[low_scratch + j] = S.v[low + j];
        OG_LSYNC();
        low = low_scratch;
    }
    for (int k = 0; k < recombine; k++) {
        if (low >= 0) haar1_p2(low, N >> k, k);
        int lo = fill & 0xF, hi = fill >> 4; // bit_interleave_table celt.cpp:1560
        int tl = (lo & 3 ? 1 : 0) | (lo & 12 ? 2 : 0), th = (hi & 3 ? 1 : 0) | (hi & 12 ? 2 : 0);
        fill = tl | th << 2;
    }
    logB -= recombine;
    N_B <<= recombine;
    while ((N_B & 1) == 0 && tf_change < 0) {
        if (low >= 0) haar1_p2(low, N_B, logB);
        fill |= fill << (1 << logB);
        logB++;
        N_B >>= 1;
        time_divide++;
        tf_change++;
    }
    const int logB0 = logB, N_B0 = N_B, B0 = 1 << logB0;
    if (B0 > 1 && low >= 0) hadamard_p2(low, N_B >> recombine, logB0 + recombine, longBlocks, 0);
    OG_MARK(6);
    u32 cm = recon_job_leaves(cur, lcg, jw, seed, x, low, fill, job);
    OG_MARK(8);
    if (B0 > 1) hadamard_p2(x, N_B >> recombine, logB0 + recombine, longBlocks, 1);
    OG_STAT(7, B0 > 1);                             // jobs that undo a Hadamard interleave on x
    OG_STAT(8, time_divide + recombine);            // Haar passes on x
    OG_STAT(9, low_out >= 0);                       // jobs that write folding history
    N_B = N_B0;
    for (int k = 0; k < time_divide; k++) {
        logB--;
        N_B <<= 1;
        cm |= cm >> (1 << logB);
        haar1_p2(x, N_B, logB);
    }
    for (int k = 0; k < recombine; k++) {
        u32 c4 = cm & 0xF; // bit_deinterleave_table celt.cpp:1606
        cm = ((c4 & 1) * 0x03) | ((c4 >> 1 & 1) * 0x0C) | ((c4 >> 2 & 1) * 0x30) | ((c4 >> 3 & 1) * 0xC0);
        haar1_p2(x, N0 >> k, k);
    }
    logB += recombine;
    OG_MARK(9);
    if (low_out >= 0) {
        OG_LSYNC();
        OG_FOR_LANES(j, N0) S.v[low_out + j] = (i16)mul16_q15(scale, S.v[x + j]);
        OG_LSYNC();
    }
    return cm & ((1u << (1 << logB)) - 1);
}

// quant_all_bands celt.cpp:1754, vector half: an interpreter of the record's word stream
OG_DEV void recon_all_bands(const u32 *words, u32 need_norm, const LcgTab &lcg, int start, int end, int C, int N_ch, int shortBlocks, int LM,
                            u32 &seed_io) {
    const int M = 1 << LM, B = shortBlocks ? M : 1;
    OG_STAT(0, 1);                 // frames
    OG_STAT(19, shortBlocks != 0); // transient frames
    const int norm_offset = M * rom_eband[start];
    const int norm = V_NORM, norm2 = V_NORM + M * rom_eband[NBANDS - 1] - norm_offset;
    // The reference borrows the last band's spectrum slot as scratch; here that slot already holds the band's
    // decoded pulses, so the scratch row lives in the (otherwise unused) pulse row.
    int low_scratch = V_IY;
    RecCur cur;
    cur.words = words;
    cur.w = 0;
    cur.base = -64;
    cur.leaf = 0;
    u32 seed = seed_io;
    for (int i = start; i < end; i++) {
        OG_MARK(3);
        const int last = i == end - 1;
        u32 w0, w1, w2, w3;
        cur.w = (cur.w + 3) & ~3; // (a band's header starts on a multiple of four: RecWriter::band_begin)
        rec_word4(cur, w0, w1, w2, w3);
        const int eb0 = (int)(w1 >> 11) & 2047, N = (int)(w1 >> 22) & 255;
        const int x = V_X + eb0, y = C == 2 ? V_X + N_ch + eb0 : -1;
        const int dual_stereo = (w0 & BW_DUAL) != 0;
        if (i == start + 1) { // special_hybrid_folding celt.cpp:1743
            int n1 = M * (rom_eband[start + 1] - rom_eband[start]), n2 = M * (rom_eband[start + 2] - rom_eband[start + 1]);
            if (n2 > n1) {
                OG_LSYNC();
                OG_FOR_LANES(j, n2 - n1) {
                    S.v[norm + n1 + j] = S.v[norm + 2 * n1 - n2 + j];
                    if (w0 & BW_DUAL_PRE) S.v[norm2 + n1 + j] = S.v[norm2 + 2 * n1 - n2 + j];
                }
                OG_LSYNC();
            }
        }
        const int tf_change = (int)((w0 >> BW_TF_SHIFT) & 7) - 4;
        OG_STAT(13, 1);                                             // bands
        OG_STAT(14, N == 1);                                        // N == 1 bands
        OG_STAT(15, (w0 & BW_STEREO) && N > 2);                     // bands that end in a stereo merge
        OG_STAT(16, (w0 & BW_STEREO) && N == 2);                    // N == 2 stereo bands
        OG_STAT(17, dual_stereo);                                   // dual-stereo bands
        OG_STAT(18, (w0 & BW_HAS_LOW) != 0);                        // bands with a folding source available
        if (last) low_scratch = -1;
        u32 x_cm, y_cm;
        if (w0 & BW_HAS_LOW) {
            const int fold_end = (int)(w0 >> BW_FOLD1_SHIFT) & 31;
            int fold_i = (int)(w0 >> BW_FOLD0_SHIFT) & 31;
            x_cm = y_cm = 0;
            do {
                x_cm |= (u32)OG_UNI(S.cmask_row()[fold_i * C + 0]);
                y_cm |= (u32)OG_UNI(S.cmask_row()[fold_i * C + C - 1]);
            } while (++fold_i < fold_end);
        } else
            x_cm = y_cm = (1u << B) - 1;
        if (w0 & BW_DUAL_END) {
            OG_LSYNC();
            OG_FOR_LANES(j, eb0 - norm_offset) S.v[norm + j] = (i16)((S.v[norm + j] + S.v[norm2 + j]) >> 1);
            OG_LSYNC();
        }
        const int eff = (w0 & BW_HAS_LOW) ? (int)(w1 & 2047) : -1;
        const int low1 = eff >= 0 ? norm + eff : -1, low2 = eff >= 0 ? norm2 + eff : -1;
        // the folding history of a band nobody folds from is not computed at all
        const int want_out = !last && ((need_norm >> i) & 1u);
        const int out1 = want_out ? norm + eb0 - norm_offset : -1, out2 = want_out ? norm2 + eb0 - norm_offset : -1;

        if (N == 1) { // quant_band_n1 celt.cpp:1357
            OG_MARK(11);
            OG_LSYNC();
            S.v[x] = (i16)((w0 & BW_SIGN0) ? -16384 : 16384);
            if (y >= 0) S.v[y] = (i16)((w0 & BW_SIGN1) ? -16384 : 16384);
            OG_LSYNC();
            if (out1 >= 0) S.v[out1] = (i16)(S.v[x] >> 4);
            if (dual_stereo && out2 >= 0) S.v[out2] = (i16)(S.v[y] >> 4);
            OG_LSYNC();
            x_cm = y_cm = 1;
        } else {
            OG_MARK(4);
            const int stereo = (w0 & BW_STEREO) != 0, mid_first = (w0 & BW_MID_FIRST) != 0, swap_c = (w0 & BW_SWAP) != 0;
            const i32 imid = (i32)(i16)(w2 & 0xffff), iside = (i32)(w2 >> 16), scale = (i32)(i16)(w3 & 0xffff);
            i32 fill0 = (i32)(x_cm | y_cm);
            const i32 orig_fill = fill0;
            int n2case = 0, njobs = 1;
            if (stereo) {
                if (w0 & BW_THETA0) fill0 &= (1 << B) - 1;
                if (w0 & BW_THETA1) fill0 &= ((1 << B) - 1) << B;
                if (N == 2)
                    n2case = 1;
                else
                    njobs = 2;
            } else if (dual_stereo)
                njobs = 2;
            u32 cm0 = 0, cm1 = 0;
#pragma nounroll
            for (int jb = 0; jb < njobs; jb++) {
                int jx, jlow, jout, jscr;
                i32 jfill;
                if (dual_stereo) {
                    jx = jb ? y : x; jlow = jb ? low2 : low1; jout = jb ? out2 : out1; jscr = low_scratch;
                    jfill = (i32)(jb ? y_cm : x_cm);
                } else if (!stereo) {
                    jx = x; jlow = low1; jout = out1; jscr = low_scratch; jfill = fill0;
                } else if (n2case) {
                    jx = swap_c ? y : x; jlow = low1; jout = out1; jscr = low_scratch; jfill = orig_fill;
                } else if ((jb == 0) == (mid_first != 0)) {
                    jx = x; jlow = low1; jout = out1; jscr = low_scratch; jfill = fill0;
                } else {
                    jx = y; jlow = -1; jout = -1; jscr = -1; jfill = fill0 >> B;
                }
                OG_MARK(5);
                const u32 jw = rec_word(cur);
                const u32 cmj = recon_band_mono(cur, jw, lcg, tf_change, seed, jx, N, B, jlow, jout, scale, jscr, jfill, 2 * i + jb);
                if (jb == 0) cm0 = cmj; else cm1 = cmj;
            }
            OG_MARK(10);
            if (stereo) {
                if (n2case) { // N == 2: the side is the mid rotated by 90 degrees (celt.cpp:1659-1697)
                    const int x2 = swap_c ? y : x, sign = (w0 & BW_SIGN) ? -1 : 1;
                    OG_LSYNC();
                    const i32 a0 = S.v[x2], a1 = S.v[x2 + 1];
                    const i32 b0 = tr16(-sign * a1), b1 = tr16(sign * a0);
                    i32 X0 = swap_c ? b0 : a0, X1 = swap_c ? b1 : a1, Y0 = swap_c ? a0 : b0, Y1 = swap_c ? a1 : b1;
                    X0 = tr16(mul16_q15(imid, X0));
                    X1 = tr16(mul16_q15(imid, X1));
                    Y0 = tr16(mul16_q15(iside, Y0));
                    Y1 = tr16(mul16_q15(iside, Y1));
                    OG_LSYNC();
                    S.v[x] = (i16)sub16(X0, Y0);
                    S.v[y] = (i16)add16(X0, Y0);
                    S.v[x + 1] = (i16)sub16(X1, Y1);
                    S.v[y + 1] = (i16)add16(X1, Y1);
                    OG_LSYNC();
                } else
                    stereo_merge(x, y, imid, N);
                if (w0 & BW_INV) {
                    OG_LSYNC();
                    OG_FOR_LANES(j, N) S.v[y + j] = (i16)(-S.v[y + j]);
                    OG_LSYNC();
                }
                x_cm = y_cm = cm0 | cm1;
            } else if (dual_stereo) {
                x_cm = cm0;
                y_cm = cm1;
            } else
                x_cm = y_cm = cm0;
        }
        S.cmask_row()[i * C + 0] = (u8)x_cm;
        S.cmask_row()[i * C + C - 1] = (u8)y_cm;
    }
    seed_io = seed;
}

} // namespace og

#include "og_celt_recon_pm.hpp"

namespace og {

// One CELT-only frame, vector half + synthesis + stream bookkeeping (decode_frame_wave's CELT branch).
// Returns the frame's result code (wave-uniform).  The comb-filtered output goes to the stream's history ring; the
// last, strictly serial step -- de-emphasis to int16 PCM -- is celt_post_lane's, one (frame, channel) per lane.
// Which reconstruction kernel takes a frame: 20 ms frames whose record is complete -- CELT-only ones and the CELT half of
// hybrid ones (bands 17 - 20) -- go to the kernel with the 8 KB working set (og_recon.hip, phase-major band loop only),
// everything else -- the 2.5 ms transition frame, records that overflowed -- to the general one.
enum { RECON_ALL = 0, RECON_FAST_ONLY = 1, RECON_REST_ONLY = 2, RECON_NOT_MINE = -1000 };

// Everything the reconstruction reads of the record's header and of the stream's scalars.  The kernel of 20 ms frames
// (og_recon.hip) fills it from two batched loads at its start -- a dozen dependent round trips to HBM one after the other, each
// followed by its wait, were 17 % of a wave's lifetime in the section profile (profiles/r02/a_celt_recon_sections_5: "outside") --
// the general kernel and the host emulation by plain loads (recon_hdr_load).
struct ReconHdr {
    i32 ret;
    u32 rng_final, flags;
    i32 pf_pitch, pf_gain, pf_tapset, start, n_leaves, n_words, n_coef;
    u32 need_norm;
    i32 channels, prev_mode, frames_decoded;
    u32 rng;
    i32 ring_pos, st_pf_period, st_pf_period_old, st_pf_gain, st_pf_gain_old, st_pf_tapset, st_pf_tapset_old;
};
OG_DEV void recon_hdr_load(const StreamState *st, const ParseRec *rec, ReconHdr &h) {
    h.ret = OG_UNI(rec->ret); h.rng_final = (u32)OG_UNI(rec->rng_final); h.flags = (u32)OG_UNI(rec->flags);
    h.pf_pitch = OG_UNI(rec->pf_pitch); h.pf_gain = OG_UNI(rec->pf_gain); h.pf_tapset = OG_UNI(rec->pf_tapset);
    h.start = OG_UNI(rec->start); h.n_leaves = OG_UNI(rec->n_leaves); h.n_words = OG_UNI(rec->n_words);
    h.need_norm = (u32)OG_UNI(rec->need_norm); h.n_coef = OG_UNI(rec->n_coef);
    h.channels = OG_UNI(st->channels); h.prev_mode = OG_UNI(st->prev_mode); h.frames_decoded = OG_UNI(st->frames_decoded);
    const CeltState *cs = &st->celt;
    h.rng = (u32)OG_UNI(cs->rng); h.ring_pos = OG_UNI(cs->ring_pos);
    h.st_pf_period = OG_UNI(cs->pf_period); h.st_pf_period_old = OG_UNI(cs->pf_period_old);
    h.st_pf_gain = OG_UNI(cs->pf_gain); h.st_pf_gain_old = OG_UNI(cs->pf_gain_old);
    h.st_pf_tapset = OG_UNI(cs->pf_tapset); h.st_pf_tapset_old = OG_UNI(cs->pf_tapset_old);
}
#ifndef OG_HOST_EMUL
// The same in ONE vector load (per-lane addresses): lanes 0-15 the record's first 16 words, 16-19 the stream's first four,
// 20-31 the twelve words of CeltState from `deemph` on; then lane reads.  (Layout asserted below.)
static_assert(offsetof(ParseRec, ret) == 0 && offsetof(ParseRec, rng_final) == 4 && offsetof(ParseRec, flags) == 8 && offsetof(ParseRec, pf_pitch) == 16 &&
              offsetof(ParseRec, pf_gain) == 20 && offsetof(ParseRec, pf_tapset) == 24 && offsetof(ParseRec, start) == 28 &&
              offsetof(ParseRec, n_leaves) == 32 && offsetof(ParseRec, n_words) == 36 && offsetof(ParseRec, need_norm) == 40 &&
              offsetof(ParseRec, n_coef) == 44, "record header words");
static_assert(offsetof(StreamState, channels) == 0 && offsetof(StreamState, prev_mode) == 4, "stream header words");
static_assert(offsetof(CeltState, rng) == offsetof(CeltState, deemph) + 8 && offsetof(CeltState, ring_pos) == offsetof(CeltState, deemph) + 12 &&
              offsetof(CeltState, pf_period) == offsetof(CeltState, deemph) + 16 && offsetof(CeltState, pf_tapset_old) == offsetof(CeltState, deemph) + 36,
              "stream scalar words");
OG_DEV i32 recon_hdr_fetch(const StreamState *st, const ParseRec *rec) { // the lane's word of the batch
    const int l = OG_LANE;
    const i32 *p = l < 16 ? reinterpret_cast<const i32 *>(rec) + l
                 : l < 20 ? reinterpret_cast<const i32 *>(st) + (l - 16)
                          : reinterpret_cast<const i32 *>(&st->celt.deemph[0]) + ((l < 32 ? l : 31) - 20);
    return *p;
}
OG_DEV void recon_hdr_unpack(i32 w, ReconHdr &h) {
#define OG_HW(lane) __builtin_amdgcn_readlane(w, lane)
    h.ret = OG_HW(0); h.rng_final = (u32)OG_HW(1); h.flags = (u32)OG_HW(2); h.pf_pitch = OG_HW(4); h.pf_gain = OG_HW(5); h.pf_tapset = OG_HW(6);
    h.start = OG_HW(7); h.n_leaves = OG_HW(8); h.n_words = OG_HW(9); h.need_norm = (u32)OG_HW(10); h.n_coef = OG_HW(11);
    h.channels = OG_HW(16); h.prev_mode = OG_HW(17); h.frames_decoded = OG_HW(18);
    h.rng = (u32)OG_HW(22); h.ring_pos = OG_HW(23); h.st_pf_period = OG_HW(24); h.st_pf_period_old = OG_HW(25); h.st_pf_gain = OG_HW(26);
    h.st_pf_gain_old = OG_HW(27); h.st_pf_tapset = OG_HW(28); h.st_pf_tapset_old = OG_HW(29);
#undef OG_HW
}
#endif

// The reconstruction of a frame in three stages, so that the middle one -- the PVQ leaves -- can be done for several frames of a
// workgroup at once (og_recon.hip); celt_recon_wave below strings them together for one frame.
//   recon_begin    is the frame this kernel's?  stream reset on a mode change, the spectrum cleared
//   (leaf pass)    every PVQ leaf: index -> pulses -> scaled, de-rotated coefficients + collapse mask (pvq_leaf_lane)
//   recon_finish   band loop, anti-collapse, synthesis, stream bookkeeping; returns the frame's result code
struct ReconCtx {
    ReconHdr h;
    u32 flags, rng_final;
    int ret, mode, C;
    int mode_after = -1; // what the frame leaves as prev_mode when it is not `mode` (desc_mode_after)
    bool leaves; // the frame has a leaf pass and a synthesis (its record is not a BAD_CELT one)
    bool fast;
    bool was_reset = false; // the stream's CELT state was reset at this frame (mode change)
    bool booked = false;    // recon_bookkeeping has run already (og_recon.hip: right behind recon_begin)
    // what recon_finish stages late, fetched early by the caller (per lane: entry `lane` of the record's band energies and
    // pulses, of the stream's two energy histories as they were BEFORE a reset), or not (pre == false: read there)
    bool pre = false;
    i32 pre_bandE, pre_logE1, pre_logE2, pre_pulses;
    i32 pre_band_w; // (entry `lane` of the record's band_w: recon_begin puts it where the band loop's set-up reads it, S.band_w_row())
};
OG_DEV bool recon_fast_eligible(const ReconHdr &h) {
    if (h.flags & (RF_SKIP | RF_BAD_CELT)) return false;
    return ((h.flags >> RF_LM_SHIFT) & 3) == 3 && h.n_words < REC_MAX_WORDS && h.n_leaves <= FAST_MAX_LEAVES;
}
// (rx.h filled by the caller.)  Returns false when the frame is not for this kernel (rx.ret then holds what celt_recon_wave
// returns for it)
OG_DEV bool recon_begin(StreamState *st, const ParseRec *rec, int mode, int ch, int role, ReconCtx &rx) {
    rx.flags = rx.h.flags;
    rx.ret = rx.h.ret;
    rx.mode = mode;
    rx.C = ch;
    rx.leaves = false;
    if (rx.flags & RF_SKIP) {
        if (role == RECON_FAST_ONLY) rx.ret = (int)RECON_NOT_MINE;
        return false;
    }
    rx.fast = recon_fast_eligible(rx.h);
    if ((role == RECON_FAST_ONLY && !rx.fast) || (role == RECON_REST_ONLY && rx.fast)) {
        rx.ret = (int)RECON_NOT_MINE;
        return false;
    }
    const int prev_mode = rx.h.prev_mode;
    if (mode != prev_mode && prev_mode > 0) {
        celt_reset_state(&st->celt); // (and the copies of what it clears)
        rx.was_reset = true;
        rx.h.rng = 0;
        rx.h.st_pf_period = rx.h.st_pf_period_old = rx.h.st_pf_tapset = rx.h.st_pf_tapset_old = 0;
        rx.h.st_pf_gain = rx.h.st_pf_gain_old = 0;
        OG_LSYNC();
    }
    rx.rng_final = rx.h.rng_final;
    if (!(rx.flags & RF_BAD_CELT)) {
        rx.leaves = true;
        OG_MARK(1);
        OG_LSYNC();
#ifndef OG_RECON_TIGHT
        CeltState *cs = &st->celt;
        OG_FOR_LANES(i, 2 * NBANDS) {
            S.bandE_row()[i] = rec->bandE[i];
            S.logE1_row()[i] = cs->logE1[i];
            S.logE2_row()[i] = cs->logE2[i];
            S.cmask_row()[i] = 0;
        }
        OG_FOR_LANES(i, NBANDS) {
            S.pulses_row()[i] = rec->pulses[i];
            S.tf_res[i] = rec->tf_res[i];
        }
#endif
        OG_FOR_LANES(i, 2 * NBANDS) S.job_mask_row()[i] = 0;
#ifdef OG_RECON_TIGHT
        if (rx.pre && OG_LANE < NBANDS) S.band_w_row()[OG_LANE] = (u16)rx.pre_band_w;
#endif
#ifdef OG_HOST_EMUL
        OG_FOR_LANES(i, 2 * 960) S.v[V_X + i] = 0;
#else
        OG_FOR_LANES(i, 2 * 960 / 8) *reinterpret_cast<og_v4i *>(&S.v[V_X + 8 * i]) = og_v4i{0, 0, 0, 0}; // 16 bytes per lane and store
#endif
    }
    return true;
}

// the frame's own leaves, one per lane of its own wave (the general kernel, the host emulation, one frame per workgroup)
// `pre`: the caller fetched leaf `lane`'s three words already (g0, aux0, idx0)
OG_DEV void recon_leaves_own(const ParseRec *rec, const ReconCtx &rx, bool pre = false, u32 g0 = 0, u32 aux0 = 0, u32 idx0 = 0) {
    const int n_leaves = rx.h.n_leaves, spread = (int)(rx.flags >> RF_SPREAD_SHIFT) & 3;
#if defined(OG_HOST_EMUL) && defined(OG_STATS)
    { // the wave pays for its longest leaf: what does that leaf look like?
        int max_n = 0, k_at_max = 0, sum_n = 0;
        for (int t = 0; t < n_leaves; t++) {
            const u32 g = rec->leaf[t].geom;
            const int n = (int)(g >> 11) & 255, k = (int)(g >> 19) & 255;
            sum_n += n;
            if (n > max_n) { max_n = n; k_at_max = k; }
        }
        OG_STAT(40, max_n); OG_STAT(41, k_at_max); OG_STAT(42, sum_n); OG_STAT(44, n_leaves);
        OG_STAT(45, max_n >= 96); OG_STAT(46, max_n >= 144);
    }
#endif
    OG_MARK(2);
#ifdef OG_HOST_EMUL
    OG_FOR_LANES(t, n_leaves) {
        const bool first = pre && t < OG_NLANES;
        const u32 g = first ? g0 : rec->leaf[t].geom;
        const u32 aux = first ? aux0 : rec->leaf[t].aux;
        const u32 idx = first ? idx0 : rec->leaf[t].idx;
        job_mask_or((int)(aux >> 20) & 63, (pvq_leaf_lane(S.v, pvq_lds(), (int)(g >> 11) & 255, (int)(g >> 19) & 255, idx, V_X + (int)(g & 2047),
                                                          (int)(g >> 27) + 1, (i32)(aux & 0xffff), spread)
                                            << ((aux >> 16) & 15)) & 0xffffu);
    }
    OG_LSYNC();
#else
    // rounds of 64 leaves: index -> pulses -> scaled, one leaf per lane; then the round's rotations by the whole wave
    for (int t0 = 0; t0 < n_leaves; t0 += OG_NLANES) {
        const int t = t0 + OG_LANE;
        RotJob job;
        job.x = job.blen = job.logB = job.stride2 = 0;
        job.c = job.s = 0;
        job.on = false;
        if (t < n_leaves) {
            const bool first = pre && t0 == 0;
            const u32 g = first ? g0 : rec->leaf[t].geom;
            const u32 aux = first ? aux0 : rec->leaf[t].aux;
            const u32 idx = first ? idx0 : rec->leaf[t].idx;
            job_mask_or((int)(aux >> 20) & 63, (pvq_leaf_lane(S.v, pvq_lds(), (int)(g >> 11) & 255, (int)(g >> 19) & 255, idx, V_X + (int)(g & 2047),
                                                              (int)(g >> 27) + 1, (i32)(aux & 0xffff), spread, &job)
                                                << ((aux >> 16) & 15)) & 0xffffu);
        }
        OG_LSYNC();
        OG_MARK(28);
        pvq_rotate_wave(S.v, job, S.rot_marker());
    }
    OG_LSYNC();
#endif
}

// What the frame leaves in the stream's header words, and the frame's result code -- all known once recon_begin has run (nothing
// in between reads these words).  The 20 ms kernel calls this THERE: carried to the end of the frame the three values were two
// spilled registers at its 80.
OG_DEV int recon_result(const ReconCtx &rx) { return (rx.leaves && (rx.flags & RF_TELL_OVERFLOW)) ? INTERNAL_ERROR : rx.ret; }
OG_DEV void recon_bookkeeping(StreamState *st, const ReconCtx &rx) {
    if (OG_LANE == 0) {
        st->prev_mode = rx.mode_after >= 0 ? rx.mode_after : rx.mode;
        st->frames_decoded = rx.h.frames_decoded + 1;
        st->range_final = rx.rng_final;
    }
}
OG_DEV int recon_finish(StreamState *st, const ParseRec *rec, const ReconCtx &rx) {
    const u32 flags = rx.flags;
    const int mode = rx.mode, C = rx.C, CC = rx.h.channels;
    int result = rx.ret;
    if (rx.leaves) {
        const int LM = (int)(flags >> RF_LM_SHIFT) & 3, M = 1 << LM, N = M * 120;
        const int transient = (flags & RF_TRANSIENT) != 0, silence = (flags & RF_SILENCE) != 0;
        const int start = rx.h.start, end = NBANDS;
        CeltState *cs = &st->celt;
        LcgTab lcg;
#ifndef OG_RECON_TIGHT
        // the phase-major band loop takes every 20 ms frame whose record did not overflow (hybrid: from band 17)
        const bool pm = rx.fast;
        if (!pm) { // the band walk starts from an empty folding history (the PVQ table that was there is no longer needed)
            OG_FOR_LANES(i, 1248) S.v[V_NORM + i] = 0;
            OG_LSYNC();
        }
#endif
        u32 seed = rx.h.rng;
#ifdef OG_RECON_TIGHT
        recon_all_bands_pm(rec, lcg, C, transient ? M : 0, seed, start, rx.pre);
        // what anti-collapse and the synthesis read besides the spectrum, staged only now (og_state.hpp, V_LATE: the rows
        // were the band loop's scratch until here; the bands' collapse masks are there already)
        if (rx.pre) {
            if (OG_LANE < 2 * NBANDS) {
                S.bandE_row()[OG_LANE] = (i16)rx.pre_bandE;
                S.logE1_row()[OG_LANE] = (i16)(rx.was_reset ? -28 * 1024 : rx.pre_logE1);
                S.logE2_row()[OG_LANE] = (i16)(rx.was_reset ? -28 * 1024 : rx.pre_logE2);
            }
            if (OG_LANE < NBANDS) S.pulses_row()[OG_LANE] = rx.pre_pulses;
        } else {
            OG_FOR_LANES(i, 2 * NBANDS) {
                S.bandE_row()[i] = rec->bandE[i];
                S.logE1_row()[i] = cs->logE1[i];
                S.logE2_row()[i] = cs->logE2[i];
            }
            OG_FOR_LANES(i, NBANDS) S.pulses_row()[i] = rec->pulses[i];
        }
        OG_LSYNC();
#else
        if (pm)
            recon_all_bands_pm(rec, lcg, C, transient ? M : 0, seed, start);
        else
            recon_all_bands(rec->words, rx.h.need_norm, lcg, start, end, C, N, transient ? M : 0, LM, seed);
#endif
        OG_MARK(12);
        if (flags & RF_ANTI_COLLAPSE) anti_collapse_pm(lcg, LM, C, N, start, end, seed);
        if (silence) {
            OG_LSYNC();
            OG_FOR_LANES(i, C * NBANDS) S.bandE_row()[i] = (i16)(-28 * 1024);
        }
        OG_TAP(1);
        CeltSynth sp;
        sp.N = N; sp.LM = LM; sp.C = C; sp.CC = CC; sp.start = start; sp.end = end; sp.silence = silence; sp.transient = transient;
        sp.pf_pitch = rx.h.pf_pitch; sp.pf_tapset = rx.h.pf_tapset; sp.pf_gain = rx.h.pf_gain;
        sp.have_state = 1;
        sp.st_pf_period = rx.h.st_pf_period; sp.st_pf_period_old = rx.h.st_pf_period_old; sp.st_pf_gain = rx.h.st_pf_gain;
        sp.st_pf_gain_old = rx.h.st_pf_gain_old; sp.st_pf_tapset = rx.h.st_pf_tapset; sp.st_pf_tapset_old = rx.h.st_pf_tapset_old;
        sp.st_ring_pos = rx.h.ring_pos;
        sp.rng_final = rx.rng_final; sp.rc_error = (flags & RF_RC_ERROR) != 0; sp.inline_deemph = 0;
        sp.loss = nullptr; sp.lost = 0; sp.energies_kept_by_parse = 1;
        OG_MARK(13);
        celt_synthesis(cs, sp);
        OG_MARK(17);
        if (flags & RF_TELL_OVERFLOW) result = INTERNAL_ERROR;
    }
    if (!rx.booked) recon_bookkeeping(st, rx);
    return result; // de-emphasis and PCM: celt_post_lane (k_celt_post), from the history ring
}

OG_DEV int celt_recon_wave(StreamState *st, const ParseRec *rec, int mode, int ch, int role = RECON_ALL, int mode_after = -1) {
    ReconCtx rx;
    rx.mode_after = mode_after;
    recon_hdr_load(st, rec, rx.h);
    if (!recon_begin(st, rec, mode, ch, role, rx)) return rx.ret;
    if (rx.leaves) {
        pvq_tab_load();
        OG_LSYNC();
        recon_leaves_own(rec, rx);
    }
    return recon_finish(st, rec, rx);
}

// Third step of the split path for (frame, channel c): runs whenever the frame was synthesised; PCM only on success.
// `silk` (hybrid frames): the SILK half's PCM, added with saturation over the first 960 * ch interleaved entries
// (opus_decode_frame src/opus_decoder.cpp:271-273, Q3).
OG_DEV void celt_post(StreamState *st, const ParseRec *rec, int result, int c, i16 *pcm, const i16 *silk, int ch) {
    if (rec->flags & (RF_SKIP | RF_BAD_CELT)) return;
    celt_post_lane(&st->celt, c, st->channels, 960, (st->celt.ring_pos - 960) & RING_MASK, result >= 0 ? pcm : nullptr, silk, 960 * ch);
}

} // namespace og
