// TEST-ONLY program for tests/test_synth_twiddles.py (built there with g++ under ASan + UBSan; no GPU): the long block's radix-3 and
// radix-5 stages as they ship -- LongStage's element and twiddle indices by (pass, lane), long_bfly3 / long_bfly5 with packed
// twiddles (og_celt.hpp) -- against the generic fft_stage of the same 480-point schedule in the one-lane host emulation.
//   1  every (stage, pass, lane, twiddle): the index LongStage names equals the one fft_stage derives from the butterfly's id
//      = lane + 64 pass (i = id / m, j = id mod m, element i mm + j, twiddle k j fstride); the live (pass, lane) of a stage are its
//      butterflies, each once; every index a lane names, live or not, lies inside the 480-entry table;
//   2  the same j -- so the same two twiddles -- in every radix-3 pass of a lane;
//   3  every packed word of rom_fft_tw32 equals the pair (rom_fft_tw[2 t], rom_fft_tw[2 t + 1]);
//   4  the stages themselves: 480 random points (corners included) through fft_stage and through the lane-by-lane butterflies,
//      every word equal.
// Exit status 0 and one line of counts when everything holds.
#define OG_HOST_EMUL 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "og_celt_recon.hpp"

extern "C" void og_emul_tap(int) {}

using namespace og;

static u32 g_seed = 480u;
static u32 rnd() { return (g_seed = g_seed * 1664525u + 1013904223u) >> 4; }
static i32 value() {
    static const i32 CORNER[6] = {0, 1, -1, SIG_SAT, -SIG_SAT, 1 << 28};
    const u32 r = rnd();
    return (r & 7u) == 0 ? CORNER[(r >> 3) % 6] : (i32)(rnd() << 4) >> 3; // up to +-2^28: what a saturated spectrum can reach
}

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main() {
    const int LANES = 64;
    long idx_cases = 0, word_cases = 0, same_j = 0, stage_words = 0;
    // ---- 1, 2: indices
    struct Gen { int p, m, Nrep, mm, fstride, passes; } gen[2] = {{3, 32, 5, 96, 5, LongStage::R3_PASSES}, {5, 96, 1, 1, 1, LongStage::R5_PASSES}};
    for (const Gen &g : gen) {
        const int per_blk = g.Nrep * g.m;
        std::vector<int> seen(per_blk, 0);
        int j_first[64];
        CHECK(g.passes == (per_blk + LANES - 1) / LANES, "radix %d: %d passes", g.p, g.passes);
        for (int pass = 0; pass < g.passes; pass++)
            for (int lane = 0; lane < LANES; lane++) {
                const int id = lane + LANES * pass; // OG_FOR_LANES(id, per_blk) with 64 lanes
                const bool live = g.p == 3 ? LongStage::r3_live(lane, pass) : LongStage::r5_live(lane, pass);
                CHECK(live == (id < per_blk), "radix %d pass %d lane %d", g.p, pass, lane);
                const int elem = g.p == 3 ? LongStage::r3_elem(lane, pass) : LongStage::r5_elem(lane, pass);
                for (int k = 1; k < g.p; k++, idx_cases++) {
                    const int tw = g.p == 3 ? LongStage::r3_tw(lane, k) : LongStage::r5_tw(lane, pass, k);
                    CHECK(tw >= 0 && tw < 480, "radix %d pass %d lane %d k %d: twiddle %d outside the table", g.p, pass, lane, k, tw);
                    if (!live) continue;
                    const int i = id / g.m, j = id - i * g.m;
                    CHECK(elem == i * g.mm + j, "radix %d pass %d lane %d: element %d, generic %d", g.p, pass, lane, elem, i * g.mm + j);
                    CHECK(tw == k * j * g.fstride, "radix %d pass %d lane %d k %d: twiddle %d, generic %d", g.p, pass, lane, k, tw, k * j * g.fstride);
                    CHECK(elem + (g.p - 1) * g.m < 480, "radix %d pass %d lane %d: element past the transform", g.p, pass, lane);
                    if (g.p == 3) {
                        if (pass == 0) j_first[lane] = j; // (the generic stage's j of this lane's first butterfly)
                        CHECK(j == j_first[lane], "radix 3 pass %d lane %d: j %d, in pass 0 %d", pass, lane, j, j_first[lane]);
                        same_j++;
                    }
                }
                if (live) seen[id]++;
            }
        for (int id = 0; id < per_blk; id++) CHECK(seen[id] == 1, "radix %d: butterfly %d run %d times", g.p, id, seen[id]);
    }
    // ---- 3: packed words
    for (int t = 0; t < 480; t++, word_cases++) {
        const u32 w = rom_fft_tw32[t];
        CHECK((i32)(i16)(w & 0xffff) == rom_fft_tw[2 * t] && ((i32)w >> 16) == rom_fft_tw[2 * t + 1], "packed twiddle %d", t);
    }
    // ---- 4: the stages on data
    for (int round = 0; round < 8; round++) {
        std::vector<i32> a(960), b(960);
        for (int k = 0; k < 960; k++) a[k] = b[k] = value();
        fft_stage(a.data(), 1, 960, 3, 32, 5, 96, 5);
        for (int pass = 0; pass < LongStage::R3_PASSES; pass++)
            for (int lane = 0; lane < LANES; lane++)
                if (LongStage::r3_live(lane, pass))
                    long_bfly3(b.data(), LongStage::r3_elem(lane, pass), rom_fft_tw32[LongStage::r3_tw(lane, 1)], rom_fft_tw32[LongStage::r3_tw(lane, 2)]);
        for (int k = 0; k < 960; k++, stage_words++) CHECK(a[k] == b[k], "radix-3 stage, round %d word %d: %d vs %d", round, k, a[k], b[k]);
        fft_stage(a.data(), 1, 960, 5, 96, 1, 1, 1);
        for (int pass = 0; pass < LongStage::R5_PASSES; pass++)
            for (int lane = 0; lane < LANES; lane++)
                if (LongStage::r5_live(lane, pass))
                    long_bfly5(b.data(), LongStage::r5_elem(lane, pass), rom_fft_tw32[LongStage::r5_tw(lane, pass, 1)],
                               rom_fft_tw32[LongStage::r5_tw(lane, pass, 2)], rom_fft_tw32[LongStage::r5_tw(lane, pass, 3)],
                               rom_fft_tw32[LongStage::r5_tw(lane, pass, 4)]);
        for (int k = 0; k < 960; k++, stage_words++) CHECK(a[k] == b[k], "radix-5 stage, round %d word %d: %d vs %d", round, k, a[k], b[k]);
    }
    printf("idx_cases %ld word_cases %ld same_j %ld stage_words %ld fails %ld\n", idx_cases, word_cases, same_j, stage_words, fails);
    return fails ? 1 : 0;
}
