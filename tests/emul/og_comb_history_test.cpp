// TEST-ONLY program (tests/test_comb_history_plan.py): the comb filter's history touch (og_celt.hpp: comb_touch_plan, comb_touch_span,
// comb_touch_code / comb_touch_at) against syn_at's rule, with "value = address" data: ring word j holds j (the touch reads no
// buffer word).  For both calls of celt_synthesis (off 0 / N 120, off 120 / N 840), every lag and the ring heads: every tap of every sample
// that the filter reads before the frame's first sample lies in the run the plan names for its lag, the runs lie in the span, the
// span lies inside [-1024, -1], and the 64 lanes of the touch read ring words of the span only, its first and last among them
// and no two neighbours more than a 128-byte line apart -- so every line that holds a sample of the span holds one that is read.
#define OG_HOST_EMUL 1

#include "og_celt.hpp"
#include <stdio.h>
using namespace og;

static long long taps = 0, ring_taps = 0, single_cases = 0, fade_cases = 0, lane_cases = 0, fails = 0;
static i32 ring[RING];
#define CHECK(c) do { if (!(c)) { if (fails < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #c); fails++; } } while (0)

// the taps of one call (comb_filter's arithmetic left out: which samples it reads), against run `r1` of lag T1 and `r0` of lag T0
static void call_taps(int off, int N, int T0, int T1, bool use0, bool use1, int overlap, CombRun r0, CombRun r1, int head) {
    const int end = use1 ? N : overlap;
    for (int i = 0; i < end; i++) {
        const int p = off + i;
        for (int k = -2; k <= 2; k++) {
            if (use1) {
                const int idx = p - T1 + k;
                taps++;
                if (idx < 0) {
                    ring_taps++;
                    CHECK(r1.lo <= idx && idx <= r1.hi);
                }
            }
            if (use0 && i < overlap) {
                const int idx = p - T0 + k;
                taps++;
                if (idx < 0) {
                    ring_taps++;
                    CHECK(r0.lo <= idx && idx <= r0.hi);
                }
            }
        }
    }
}

static unsigned char span_seen[1025][1025]; // [-lo][-hi]: spans whose lanes were checked at every head
static long long spans = 0;
static void lanes(const CombTouchPlan &q, int head) {
    const CombRun span = comb_touch_span(q);
    const CombRun runs[3] = {q.cur, q.old, q.next};
    for (int k = 0; k < 3; k++)
        if (runs[k].lo <= runs[k].hi) CHECK(span.lo <= runs[k].lo && runs[k].hi <= span.hi);
    if (span.lo > span.hi) return;
    CHECK(span.lo >= -1024 && span.hi <= -1);
    const int code = comb_touch_code(span, head);
    int prev = span.lo;
    bool first = false, last = false;
    for (int lane = 0; lane < 64; lane++) {
        const int idx = comb_touch_index(span, lane), at = comb_touch_at(code, lane);
        lane_cases++;
        CHECK(idx >= span.lo && idx <= span.hi);
        CHECK(at >= 0 && at < RING && ring[at] == ((head + idx) & RING_MASK)); // (the word syn_at reads for idx)
        CHECK(idx - prev <= COMB_TOUCH_STEP && idx >= prev);
        first |= idx == span.lo;
        last |= idx == span.hi;
        prev = idx;
    }
    CHECK(first && last);
}

int main() {
    for (int j = 0; j < RING; j++) ring[j] = j;
    static const int T_SET[] = {15, 16, 65, 66, 67, 120, 510, 511, 512, 513, 514, 515, 516, 958, 959, 960, 961, 962, 963, 964, 965, 966, 1022};
    const int NSET = (int)(sizeof(T_SET) / sizeof(T_SET[0]));
    // Which run a tap lies in does not depend on the ring head; where the touch's lanes read does.  So the taps of every case are
    // walked once, each case at the next of the 256 heads that are multiples of 8, and the lanes of every single-lag case and of
    // every distinct span of the cross-fade cases at all 256 heads.
    int head = 0;
    // single-lag steps: the same filter before and in the frame (no cross-fade in either call)
    for (int T = 15; T <= 1022; T++) {
        const CombTouchPlan q = comb_touch_plan(T, T, T, 8192, 8192, 8192, 0, 0, 0, 960);
        call_taps(0, 120, T, T, true, true, 0, q.old, q.cur, head);
        call_taps(120, 840, T, T, true, true, 0, q.cur, q.next, head);
        for (int h = 0; h < RING; h += 8) lanes(q, h);
        single_cases += 2;
        head = (head + 8) & RING_MASK;
    }
    // cross-fades in both calls: three different lags, one of them through every lag, the others through the set
    for (int T = 15; T <= 1022; T++)
        for (int s = 0; s < NSET; s++)
            for (int swap = 0; swap < 2; swap++) {
                const int Ta = swap ? T_SET[s] : T, Tb = swap ? T : T_SET[s], Tc = T_SET[(s + 7) % NSET];
                // call 1 fades from Ta to Tb, call 2 from Tb to Tc
                const CombTouchPlan q = comb_touch_plan(Ta, Tb, Tc, 4096, 8192, 12288, 0, 1, 2, 960);
                call_taps(0, 120, Ta, Tb, true, true, OVERLAP, q.old, q.cur, head);
                call_taps(120, 840, Tb, Tc, true, true, OVERLAP, q.cur, q.next, head);
                { // the lanes depend on the plan through its span alone: every span at all 256 heads, once
                    const CombRun sp = comb_touch_span(q);
                    if (sp.lo <= sp.hi && sp.lo >= -1024 && !span_seen[-sp.lo][-sp.hi]) {
                        span_seen[-sp.lo][-sp.hi] = 1;
                        spans++;
                        for (int h = 0; h < RING; h += 8) lanes(q, h);
                    } else
                        lanes(q, head);
                }
                fade_cases += 2;
                head = (head + 8) & RING_MASK;
            }
    // gains of zero: a filter that is off fetches no taps and gets no run
    {
        const CombTouchPlan off_on = comb_touch_plan(15, 15, 700, 0, 0, 8192, 0, 0, 0, 960); // off -> on in the second call
        CHECK(off_on.old.lo > off_on.old.hi && off_on.cur.lo > off_on.cur.hi && off_on.next.lo == 120 - 700 - 2 && off_on.next.hi == -1);
        call_taps(120, 840, 15, 700, false, true, OVERLAP, off_on.cur, off_on.next, 0);
        const CombTouchPlan on_off = comb_touch_plan(300, 300, 0, 8192, 8192, 0, 0, 0, 0, 960); // on -> off: the cross-fade only
        CHECK(on_off.next.lo > on_off.next.hi);
        call_taps(0, 120, 300, 300, true, true, 0, on_off.old, on_off.cur, 0);
        call_taps(120, 840, 300, 15, true, false, OVERLAP, on_off.cur, on_off.next, 0);
        const CombTouchPlan none = comb_touch_plan(100, 200, 300, 0, 0, 0, 0, 0, 0, 960);
        const CombRun span = comb_touch_span(none);
        CHECK(span.lo > span.hi);
    }
    printf("spans %lld single_cases %lld fade_cases %lld lane_cases %lld taps %lld ring_taps %lld fails %lld\n", spans, single_cases, fade_cases, lane_cases, taps,
           ring_taps, fails);
    return fails ? 1 : 0;
}
