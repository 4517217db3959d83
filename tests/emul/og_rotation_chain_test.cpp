// TEST-ONLY program for tests/test_rotation_chain.py (built there with g++ under ASan + UBSan; no GPU): the spreading rotation as it
// ships -- rotate1_lane / rotate_chain, og_celt_recon.hpp: one chain at a time, four steps at a time on packed pairs, the backward
// sweep started where the forward one counted to -- in the one-lane host emulation, against exp_rotation1 (celt.cpp:684) written as
// its two plain sweeps.  Every block length 1 .. 176 with every stride 1 .. len; c, s and the coefficients are random i16 values
// and the corners -32768, -1, 0, 32767.  Every vector is allocated with exactly `len` elements, so an access of the unrolled loops
// past the block's end is a sanitizer report.  Exit status 0 and one line of counts when everything is equal bit for bit.
#define OG_HOST_EMUL 1
#include <stdio.h>
#include <stdlib.h>
#include "og_celt_recon.hpp"

extern "C" void og_emul_tap(int) {}

using namespace og;

// the reference: forward over i = 0 .. len-stride-1, then backward from len-2*stride-1, pairs (i, i + stride)
static void two_sweeps(i16 *X, int len, int stride, i32 c, i32 s) {
    const i32 ms = tr16(-s);
    auto pair = [&](int i) {
        const i32 x1 = X[i], x2 = X[i + stride];
        X[i + stride] = (i16)pshr32(mul16(c, x2) + mul16(s, x1), 15);
        X[i] = (i16)pshr32(mul16(c, x1) + mul16(ms, x2), 15);
    };
    for (int i = 0; i < len - stride; i++) pair(i);
    for (int i = len - 2 * stride - 1; i >= 0; i--) pair(i);
}

static u32 g_seed = 2024u;
static u32 rnd() { return (g_seed = g_seed * 1664525u + 1013904223u) >> 8; }
static const i32 CORNER[4] = {-32768, -1, 0, 32767};
static i32 rnd16() { return (i32)(i16)(rnd() & 0xffffu); }
static i32 value() { return (rnd() & 3u) == 0 ? CORNER[rnd() & 3u] : rnd16(); } // a corner one time in four

int main() {
    const int DRAWS = 8;
    long cases = 0, no_pair = 0, one_pair = 0, fours = 0;
    unsigned combo = 0;
    for (int len = 1; len <= 176; len++)
        for (int stride = 1; stride <= len; stride++) {
            for (int r = 0; r < stride; r++) { // what the chains of this shape look like: forward steps of chain r
                const int steps = (len - r + stride - 1) / stride - 1;
                no_pair += steps == 0;
                one_pair += steps == 1;
                fours += steps > 0 && steps % 4 == 0;
            }
            for (int t = 0; t < DRAWS; t++, cases++) {
                // c and s: both random, one of them a corner, both corners (all sixteen pairs in turn)
                i32 c = rnd16(), s = rnd16();
                if ((t & 3) == 1) c = CORNER[rnd() & 3u];
                if ((t & 3) == 2) s = CORNER[rnd() & 3u];
                if ((t & 3) == 3) {
                    c = CORNER[combo & 3u];
                    s = CORNER[(combo >> 2) & 3u];
                    combo++;
                }
                i16 *ref = (i16 *)malloc(sizeof(i16) * (size_t)len), *got = (i16 *)malloc(sizeof(i16) * (size_t)len);
                if (!ref || !got) return 2;
                for (int i = 0; i < len; i++) ref[i] = got[i] = (i16)(t < 4 ? value() : rnd16());
                two_sweeps(ref, len, stride, c, s);
                rotate1_lane(got, 0, len, stride, c, s);
                for (int i = 0; i < len; i++)
                    if (ref[i] != got[i]) {
                        printf("len %d stride %d c %d s %d: element %d is %d, the two sweeps give %d\n", len, stride, c, s, i, got[i], ref[i]);
                        return 1;
                    }
                free(ref);
                free(got);
            }
        }
    printf("cases %ld no_pair %ld one_pair %ld fours %ld\n", cases, no_pair, one_pair, fours);
    return 0;
}
