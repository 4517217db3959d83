// TEST-ONLY program (tests/test_comb_step.py): the comb filter's steps as the device runs them (og_comb_step.hpp: comb_call,
// comb_steps over a memory policy) on the host with 64 lanes, against comb_filter's OG_HOST_EMUL loop (og_celt.hpp), sample for
// sample.  The policy here keeps a step's stores back until the step's last lane has read (the device's lanes read before any of
// them stores), restates the lane shifts of a window that crosses two memories, and checks EVERY read -- a dead lane's included --
// against the bounds of the synthesis buffer (SYN_LEN words), the ring (RING words) and the window table (OVERLAP entries).
// Then the scalar-operand form of MULT16_32_Q15 against mul16x32_q15 over all 65,536 gains.
#define OG_HOST_EMUL 1

#include "og_celt.hpp"
#include <stdio.h>
#include <stdlib.h>
using namespace og;

static long long fails = 0, cases = 0, samples = 0, clamped = 0, dead_reads = 0, reads = 0, fade_cases = 0, plain_cases = 0;
static long long win_steps[3] = {0, 0, 0}, mixed_fade_steps = 0, short_steps = 0, one_sided[2] = {0, 0};
#define CHECK(c) do { if (!(c)) { if (fails < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static CeltState st; // (the filter reads ring[c] and, in the reference loop, ring_pos)
static u32 lcg = 0x1234567u;
static u32 rnd() { return lcg = lcg * 1664525u + 1013904223u; }

struct HostMem {
    i32 *buf;        // SYN_LEN words
    const i32 *ring; // RING words
    int ring_pos;
    int pend_p[64];
    i32 pend_y[64];
    int npend = 0;
    int lane_begin() const { return 0; }
    int lane_end() const { return 64; }
    void sync() {
        for (int k = 0; k < npend; k++) buf[pend_p[k]] = pend_y[k];
        npend = 0;
    }
    i32 rd_buf(int i) {
        reads++;
        CHECK(i >= 0 && i < SYN_LEN);
        return buf[OG_MIN(OG_MAX(i, 0), SYN_LEN - 1)];
    }
    i32 rd_ring(int j) {
        reads++;
        CHECK(j >= 0 && j < RING);
        return ring[j & RING_MASK];
    }
    i32 y0(int p0, int lane) { return rd_buf(p0 + lane); }
    void store(int p0, int lane, i32 y) {
        CHECK(npend < 64 && p0 + lane >= 0 && p0 + lane < 960);
        pend_p[npend] = p0 + lane;
        pend_y[npend++] = y;
    }
    CombTaps buf_taps(int i0, int lane) {
        win_steps[COMB_WIN_BUF] += lane == 0;
        CHECK(i0 >= 0);
        CombTaps t;
        for (int k = 0; k < 5; k++) t.e[k] = rd_buf(i0 + lane + k);
        return t;
    }
    CombTaps ring_taps(int h0, int lane) {
        win_steps[COMB_WIN_RING] += lane == 0;
        CHECK(h0 >= 0 && h0 + 67 <= RING_MASK);
        CombTaps t;
        for (int k = 0; k < 5; k++) t.e[k] = rd_ring(h0 + lane + k);
        return t;
    }
    i32 win(int i) {
        reads++;
        CHECK(i >= 0 && i < OVERLAP);
        return rom_win120[OG_MIN(OG_MAX(i, 0), OVERLAP - 1)];
    }
    i32 tap_at(int idx) { // the device's: an unconditional buffer read at the clamped index, the ring's where the sample is history
        const i32 v = rd_buf(OG_MAX(idx, 0));
        return idx < 0 ? rd_ring((ring_pos + idx) & RING_MASK) : v;
    }
    // the device's lane shifts restated: e[4] of lane l is fetched at the index clamped to the last live lane, e[4 - k] is e[4] of
    // lane l - k, and lanes 0 .. k - 1 take what lanes 0 .. 3 fetched for lane 0's window
    CombTaps mixed_taps(int first, int lane, int last_live) {
        win_steps[COMB_WIN_MIXED] += lane == 0;
        CombTaps t;
        for (int k = 0; k < 5; k++) t.e[4 - k] = lane >= k ? tap_at(first + OG_MIN(lane - k, last_live) + 4) : tap_at(first + 4 - k + lane);
        (void)tap_at(first + (lane & 3));
        return t;
    }
};

static i32 sig() { // a signal sample: anywhere in the clamp's range, one in eight at the rails
    const u32 r = rnd();
    if ((r & 7) == 0) return (r & 8) ? SIG_SAT : -SIG_SAT;
    return (i32)((i64)(i32)rnd() * SIG_SAT / 2147483648LL);
}

static i32 buf_ref[SYN_LEN], buf_new[SYN_LEN], buf_in[SYN_LEN];

static void one_case(int c, int off, int N, int T0, int T1, i32 g0, i32 g1, int tap0, int tap1, int head) {
    for (int i = 0; i < SYN_LEN; i++) buf_in[i] = sig();
    st.ring_pos = head;
    i32 *const SY = syn_buf();
    memcpy(SY, buf_in, sizeof(buf_in));
    comb_filter(&st, c, off, T0, T1, N, g0, g1, tap0, tap1, head); // the reference: og_celt.hpp's host loop
    memcpy(buf_ref, SY, sizeof(buf_ref));
    memcpy(buf_new, buf_in, sizeof(buf_in));
    if (g0 != 0 || g1 != 0) {
        const CombCall q = comb_call(T0, T1, N, g0, g1, tap0, tap1);
        HostMem m;
        m.buf = buf_new;
        m.ring = st.ring[c];
        m.ring_pos = head;
        // (the classes of steps this case runs, by the step rule alone)
        for (int base = 0, lim; base < q.end; base += lim) {
            lim = comb_step_len(base, q.overlap, q.chunk_fade, q.chunk_rest, q.end);
            CHECK(lim >= 1 && lim <= 64);
            short_steps += lim < 64 && lim < q.end - base;
            mixed_fade_steps += base < q.overlap && base + lim > q.overlap;
            dead_reads += 64 - lim;
        }
        if (q.overlap) {
            fade_cases++;
            if (!q.use0) one_sided[0]++;
            if (!q.use1) one_sided[1]++;
        } else
            plain_cases++;
        comb_steps(m, off, q, head, RING_MASK);
        m.sync();
    }
    cases++;
    for (int i = 0; i < SYN_LEN; i++) {
        if (buf_ref[i] != buf_new[i]) {
            if (fails < 10)
                fprintf(stderr, "sample %d: %d != %d (off %d N %d T0 %d T1 %d g0 %d g1 %d taps %d %d head %d)\n", i, buf_new[i], buf_ref[i], off, N, T0, T1, g0, g1,
                        tap0, tap1, head);
            fails++;
            break;
        }
        if (i >= off && i < off + N) {
            samples++;
            clamped += (buf_ref[i] == SIG_SAT || buf_ref[i] == -SIG_SAT) && buf_ref[i] != buf_in[i];
        }
    }
}

int main() {
    for (int c = 0; c < 2; c++)
        for (int j = 0; j < RING; j++) st.ring[c][j] = sig();
    static const int T1_SET[] = {15, 16, 17, 33, 65, 66, 67, 118, 120, 122, 300, 512, 700, 959, 1021, 1022};
    const int NT1 = (int)(sizeof(T1_SET) / sizeof(T1_SET[0]));
    static const i32 GAINS[][2] = {{0, 9216}, {9216, 0}, {9216, 9216}, {3072, 24576}, {24576, 6144}, {0, 24576}, {15360, 0}}; // 3072 (qg + 1)
    const int NG = (int)(sizeof(GAINS) / sizeof(GAINS[0]));
    static long long head_used[RING / 8], gain_used[7], taps_used[9];
    long long k = 0;
    // every lag for T0 against a spread for T1 (the lag itself among them: no cross-fade where gains and tapsets agree), both
    // calls of celt_synthesis; gains, tapsets and ring heads in rotation, so that every one of each meets every lag class
    for (int T0 = 15; T0 <= 1022; T0++)
        for (int r = 0; r < 3; r++) { // three of the spread per lag, in rotation
            const int s = (3 * T0 + r) % (NT1 + 1);
            const int T1 = s == NT1 ? T0 : T1_SET[s];
            for (int call = 0; call < 2; call++, k++) {
                const int gi = (int)(k % NG), ti = (int)((k / NG) % 9), hi = (int)((k * 37 + T0) % (RING / 8));
                const i32 g0 = GAINS[gi][0], g1 = GAINS[gi][1];
                const int tap0 = ti / 3, tap1 = (s == NT1 && gi == 2) ? tap0 : ti % 3; // (gi 2: equal gains -- with T1 == T0, no cross-fade)
                head_used[hi]++; gain_used[gi]++; taps_used[tap0 * 3 + tap1]++;
                one_case((int)(k & 1), call ? 120 : 0, call ? 840 : 120, T0, T1, g0, g1, tap0, tap1, hi * 8);
                // ... and the roles swapped: every lag as the new filter's
                one_case((int)(k & 1), call ? 120 : 0, call ? 840 : 120, T1, T0, g0, g1, tap1, tap0, hi * 8);
            }
        }
    for (int h = 0; h < RING / 8; h++) CHECK(head_used[h] > 0);
    for (int g = 0; g < NG; g++) CHECK(gain_used[g] > 0);
    for (int t = 0; t < 9; t++) CHECK(taps_used[t] > 0);

    // MULT16_32_Q15 with the 16-bit operand sign-extended beforehand (mul16x32_q15_u) against mul16x32_q15: every gain against the
    // extremes of 32 bits, of the clamp's range and of the tap sums (twice the clamp), and against sampled words
    long long products = 0;
    {
        static i32 B[96];
        int nb = 0;
        const i32 ext[] = {0, 1, -1, 2147483647, -2147483647 - 1, SIG_SAT, -SIG_SAT, 2 * SIG_SAT, -2 * SIG_SAT, 32767, -32768, 65536, -65536, 0x40000000, -0x40000000};
        for (i32 e : ext) B[nb++] = e;
        while (nb < 96) B[nb++] = (i32)rnd();
        for (int g = -32768; g <= 32767; g++)
            for (int j = 0; j < nb; j++) {
                products++;
                if (mul16x32_q15_u(g, B[j]) != mul16x32_q15(g, B[j]) || mul16x32_q15_u(g, B[j]) != mul16x32_q15(g & 0xffff, B[j])) fails++;
            }
    }
    printf("cases %lld fade_cases %lld plain_cases %lld off_to_on %lld on_to_off %lld samples %lld clamped %lld reads %lld dead_lane_slots %lld "
           "buf_windows %lld ring_windows %lld mixed_windows %lld mixed_fade_steps %lld short_steps %lld products %lld fails %lld\n",
           cases, fade_cases, plain_cases, one_sided[0], one_sided[1], samples, clamped, reads, dead_reads, win_steps[0], win_steps[1], win_steps[2],
           mixed_fade_steps, short_steps, products, fails);
    return fails ? 1 : 0;
}
