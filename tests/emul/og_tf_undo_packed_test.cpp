// TEST-ONLY program for tests/test_tf_undo_packed.py (built there with g++ under ASan + UBSan; no GPU): the packed-word forms of the
// 20 ms reconstruction kernel (og_celt_packed.hpp: what the device runs in the tight layout) against the general forms (what the
// host emulation runs), both instantiations of the same functions of og_celt_recon_pm.hpp, in the one-lane host emulation.
//
// usage: og_tf_undo_packed_test CLASS...   with CLASS = ls,had,s0,s1,s2:N/N/...  -- a job's time-frequency class as pm_setup_jobs
// writes it into jdesc (log2 of the interleave stride, Hadamard ordering, the three Haar step codes) and the band widths it can have.
// The list comes from the test, which derives it from the ROM tf table; nothing here names a class.
//   1  per class: every band of a 20 ms frame whose width is listed gets the class in both channels (the other bands: a job without
//      a change), on random and on extreme spectra; pm_tf_undo<false> and pm_tf_undo<true> from the same state, every word of both
//      channels' spectra compared.  Then mixed frames: a random listed class, a fill job or no job per (band, channel);
//   2  pm_stereo_merge<false> against pm_stereo_merge<true>: random stereo / inverted / plain bands, mid gains and spectra that
//      reach the copy mode too; spectra and the bands' merge words compared;
//   3  the gather's alignment claim from the band table: every read of every (band, channel, stride 2 / 4 / 8, group, row) is
//      naturally aligned and inside its band;
//   4  the ring pieces: every ring head that is a multiple of 8, every frame size: no piece of 4 samples straddles the wrap, every
//      piece is 16-byte aligned, and ring and tail equal the sample-by-sample writes.
// Exit status 0 and one line of counts when everything holds.
#define OG_HOST_EMUL 1
#define OG_RECON_TIGHT 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "og_celt_recon.hpp"

extern "C" void og_emul_tap(int) {}

using namespace og;

static u32 g_seed = 20u;
static u32 rnd() { return (g_seed = g_seed * 1664525u + 1013904223u) >> 8; }
static i16 value(bool extremes_only) {
    static const i16 CORNER[6] = {32767, -32767, -32768, 0, 1, -1};
    const u32 r = rnd();
    return (extremes_only || (r & 7u) == 0) ? CORNER[(r >> 3) % 6] : (i16)(rnd() & 0xffffu);
}

static long fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 10) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Class { int ls, had, s[3]; std::vector<int> widths; u32 jd() const; bool has(int N) const; };
u32 Class::jd() const {
    return JD_VALID | (u32)ls << JD_PERM_SHIFT | (had ? (u32)JD_HAD : 0u) | (u32)s[0] << JD_STEP_SHIFT | (u32)s[1] << (JD_STEP_SHIFT + 4) |
           (u32)s[2] << (JD_STEP_SHIFT + 8);
}
bool Class::has(int N) const {
    for (int w : widths)
        if (w == N) return true;
    return false;
}
static u32 tfm_of(u32 jd) { // pm_setup_jobs' summary of a job without fill leaves
    u32 m = 0;
    if (!(jd & JD_VALID) || (jd & JD_FILL)) return 0;
    if ((jd >> JD_PERM_SHIFT) & 7) m |= 1u;
    for (int k = 0; k < 3; k++) {
        const int c = (int)(jd >> (JD_STEP_SHIFT + 4 * k)) & 15;
        if (c) m |= 1u << (1 + 4 * k + (c - 1));
    }
    return m;
}
static int width(int band) { return 8 * (rom_eband[band + 1] - rom_eband[band]); }

static void tables() {
    PmLds &P = PM();
    memset(&P, 0, sizeof(P));
    for (int bin = 0; bin < PM_GROUPS; bin++) {
        P.binband[bin] = rom_bin2band[bin];
        P.binoff[bin] = rom_binoff[bin];
    }
    for (int b = 0; b < NBANDS; b++) P.bw1[b] = (u32)width(b) << 22 | (u32)(8 * rom_eband[b]) << 11;
}
static void spectrum(i16 *keep, bool extremes_only) {
    for (int k = 0; k < 1920; k++) keep[k] = (k % 960) < 800 ? value(extremes_only) : 0;
}
// both forms from the same spectrum; returns the words compared
static long both_tf(const i16 *in, u32 tfm, const char *what, int id) {
    static i16 a[1920];
    memcpy(&S.v[V_X], in, sizeof(a));
    pm_tf_undo<false>(tfm);
    memcpy(a, &S.v[V_X], sizeof(a));
    memcpy(&S.v[V_X], in, sizeof(a));
    pm_tf_undo<true>(tfm);
    for (int k = 0; k < 1920; k++) CHECK(a[k] == S.v[V_X + k], "%s %d: coefficient %d (channel %d): general %d, packed %d", what, id, k % 960, k / 960, a[k], S.v[V_X + k]);
    return 960;
}

int main(int argc, char **argv) {
    std::vector<Class> classes;
    for (int i = 1; i < argc; i++) {
        Class c;
        int used = 0;
        if (sscanf(argv[i], "%d,%d,%d,%d,%d:%n", &c.ls, &c.had, &c.s[0], &c.s[1], &c.s[2], &used) != 5 || !used) return 2;
        for (const char *p = argv[i] + used; *p;) {
            c.widths.push_back((int)strtol(p, (char **)&p, 10));
            if (*p == '/') p++;
        }
        classes.push_back(c);
    }
    if (classes.empty()) return 2;
    static i16 in[1920];
    long tf_words = 0, class_widths = 0, mixed_words = 0, merge_words = 0, copy_groups = 0, inv_groups = 0, plain_groups = 0, reads = 0, pieces = 0;

    // ---- 1: the time-frequency undo
    tables();
    for (size_t ci = 0; ci < classes.size(); ci++) {
        const Class &c = classes[ci];
        PmLds &P = PM();
        u32 tfm = 0;
        bool seen[256] = {false};
        for (int b = 0; b < NBANDS; b++)
            for (int ch = 0; ch < 2; ch++) {
                const u32 jd = c.has(width(b)) ? c.jd() : (u32)JD_VALID;
                P.jdesc[2 * b + ch] = jd;
                tfm |= tfm_of(jd);
                if (c.has(width(b)) && !seen[width(b)]) {
                    seen[width(b)] = true;
                    class_widths++;
                }
            }
        for (int w : c.widths) CHECK(seen[w], "class %d: no band of a 20 ms frame is %d wide", (int)ci, w);
        for (int round = 0; round < 6; round++) {
            spectrum(in, round < 2);
            tf_words += both_tf(in, tfm, "class", (int)ci);
        }
    }
    for (int round = 0; round < 48; round++) { // mixed frames
        PmLds &P = PM();
        u32 tfm = 0;
        for (int b = 0; b < NBANDS; b++)
            for (int ch = 0; ch < 2; ch++) {
                u32 jd = 0;
                const u32 r = rnd() % 8;
                if (r == 0) jd = 0; // no job
                else {
                    for (int tries = 0; tries < 64 && !jd; tries++) {
                        const Class &c = classes[rnd() % classes.size()];
                        if (c.has(width(b))) jd = c.jd();
                    }
                    if (!jd) jd = JD_VALID;
                    if (r == 1) jd |= JD_FILL; // phase D's: the parallel pass leaves it alone
                }
                P.jdesc[2 * b + ch] = jd;
                tfm |= tfm_of(jd);
            }
        spectrum(in, round % 8 == 0);
        mixed_words += both_tf(in, tfm, "mixed frame", round);
    }

    // ---- 2: the stereo merge
    for (int round = 0; round < 64; round++) {
        PmLds &P = PM();
        static i16 a[1920];
        u32 mpar_a[NBANDS][2];
        spectrum(in, round % 8 == 0);
        for (int b = 0; b < NBANDS; b++) {
            const u32 r = rnd() % 8;
            P.bw0[b] = r == 0 ? 0u : (u32)BW_STEREO | (r & 1 ? (u32)BW_INV : 0u);
            P.bw2[b] = rnd() & 0x7fffu; // the mid gain
            if (r >= 6) { // a band near silence: the copy mode
                P.bw2[b] = rnd() % 200;
                for (int ch = 0; ch < 2; ch++)
                    for (int k = 0; k < width(b); k++) in[960 * ch + 8 * rom_eband[b] + k] = (i16)((int)(rnd() % 7) - 3);
            }
        }
        memcpy(&S.v[V_X], in, sizeof(a));
        pm_stereo_merge<false>(2);
        memcpy(a, &S.v[V_X], sizeof(a));
        memcpy(mpar_a, P.mpar, sizeof(mpar_a));
        memcpy(&S.v[V_X], in, sizeof(a));
        pm_stereo_merge<true>(2);
        for (int k = 0; k < 1920; k++) CHECK(a[k] == S.v[V_X + k], "merge %d: coefficient %d (channel %d): general %d, packed %d", round, k % 960, k / 960, a[k], S.v[V_X + k]);
        CHECK(!memcmp(mpar_a, P.mpar, sizeof(mpar_a)), "merge %d: the bands' gains differ", round);
        merge_words += 960;
        for (int b = 0; b < NBANDS; b++) {
            const int groups = width(b) / 8;
            if (!(P.mpar[b][0] & 3)) plain_groups += groups;
            else if (P.mpar[b][0] & 2) copy_groups += groups;
            if ((P.mpar[b][0] & 3) && (P.mpar[b][0] & 4)) inv_groups += groups;
        }
    }

    // ---- 3: the gather's reads
    CHECK(((uintptr_t)&S.v[0] & 15) == 0 && rom_eband[NBANDS] == PM_GROUPS, "the working set");
    for (int b = 0; b < NBANDS; b++)
        for (int ch = 0; ch < 2; ch++) {
            const int x = V_X + 960 * ch + 8 * rom_eband[b], N = width(b);
            CHECK(N % 8 == 0 && N >= 8 && N <= 255 && x % 8 == 0, "band %d", b);
            for (int ls = 1; ls <= 3; ls++) {
                const int n0 = N >> ls, unit = 8 >> ls;
                for (int gj = 0; gj < N / 8; gj++)
                    for (int row = 0; row < (1 << ls); row++, reads++) {
                        const int at = x + row * n0 + unit * gj;
                        CHECK(at % unit == 0 && at >= x && at + unit <= x + N, "band %d stride %d group %d row %d: read at %d", b, 1 << ls, gj, row, at);
                    }
            }
        }

    // ---- 4: the ring pieces
    {
        static CeltState sa, sb;
        static i32 sy[960 + OVERLAP];
        CHECK(((uintptr_t)sb.ring[0] & 15) == 0 && ((uintptr_t)sb.ring[1] & 15) == 0 && ((uintptr_t)sb.tail[0] & 15) == 0 && ((uintptr_t)sb.tail[1] & 15) == 0, "the state's rows");
        for (int head = 0; head < RING; head += 8)
            for (int LM = 0; LM <= 3; LM++) {
                const int N = 120 << LM, c = (head >> 3) & 1;
                for (int k = 0; k < N + OVERLAP; k++) sy[k] = (i32)(rnd() << 8) ^ (i32)rnd();
                memset(&sa, 0x5a, sizeof(sa));
                memset(&sb, 0x5a, sizeof(sb));
                for (int i = 0; i < N; i++) sa.ring[c][(head + i) & RING_MASK] = sy[i]; // celt_synthesis' general form
                for (int i = 0; i < OVERLAP / 2; i++) sa.tail[c][i] = sy[N + i];
                pk_ring_tail_store(sb.ring[c], sb.tail[c], sy, head, N);
                CHECK(!memcmp(&sa, &sb, sizeof(sa)), "ring head %d, frame of %d", head, N);
                for (int p = 0; p < N / 4; p++, pieces++) {
                    const int at = (head + 4 * p) & RING_MASK;
                    CHECK(at % 4 == 0 && at + 4 <= RING, "ring head %d, frame of %d: piece %d at %d", head, N, p, at);
                }
            }
    }
    printf("classes %d class_widths %ld tf_words %ld mixed_words %ld merge_words %ld plain_groups %ld copy_groups %ld inv_groups %ld reads %ld pieces %ld fails %ld\n",
           (int)classes.size(), class_widths, tf_words, mixed_words, merge_words, plain_groups, copy_groups, inv_groups, reads, pieces, fails);
    return fails ? 1 : 0;
}
