// TEST-ONLY: the plan of the multistream host path (csrc/og_ms_framing.hpp) behind a C interface for tests/test_ms_host_plan.py.
// Host code only.  An Mt is what an opusgpu_ms is to the header: a layout, a decoder count and the two halves' stream memories.
// With -DMT_MAIN (make ms_framing_asan) a program of its own: random multistream packets, damaged ones included, through the plan,
// the arena and every step table with a device that fails some frames, for the address / undefined-behaviour sanitizers to watch.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "og_ms_framing.hpp"

struct Mt {
    opusgpu_ms_layout lay;
    int n_dec;
    std::vector<int32_t> last_count[2], last_flags[2];
    ogh::MsCallPlan plan;
    ogh::MsStepTable tab[2];
    Mt(const opusgpu_ms_layout &l, int n) : lay(l), n_dec(n) {
        for (int h = 0; h < 2; h++) {
            last_count[h].assign((size_t)n * ogh::ms_half(l, h).streams, 0);
            last_flags[h].assign((size_t)n * ogh::ms_half(l, h).streams, 0);
        }
    }
    int run_plan(int mode, int cap, int n, const int32_t *ids, const uint8_t *const *packets, const int32_t *lens) {
        const ogh::MsMemory mem[2] = {{last_count[0].data(), last_flags[0].data(), (int)last_count[0].size()},
                                      {last_count[1].data(), last_flags[1].data(), (int)last_count[1].size()}};
        return ogh::ms_plan_call(lay, n_dec, mode, cap, n, ids, packets, lens, mem, plan);
    }
};

extern "C" {
void *mt_new(const opusgpu_ms_layout *lay, int n_dec) { return ogh::ms_layout_ok(lay) && n_dec > 0 ? new Mt(*lay, n_dec) : nullptr; }
void mt_free(void *h) { delete (Mt *)h; }
// out[3]: first, streams, channels of half `half`; returns index(d, s)
int mt_half(const opusgpu_ms_layout *lay, int half, int d, int s, int32_t out[3]) {
    const ogh::MsHalfLayout x = ogh::ms_half(*lay, half);
    out[0] = x.first, out[1] = x.streams, out[2] = x.channels;
    return x.index(d, s);
}
int mt_memory(void *h, int half, int32_t *last_count, int32_t *last_flags) {
    Mt *m = (Mt *)h;
    memcpy(last_count, m->last_count[half].data(), 4 * m->last_count[half].size());
    memcpy(last_flags, m->last_flags[half].data(), 4 * m->last_flags[half].size());
    return (int)m->last_count[half].size();
}
// first / cnt / eres / placed: n * streams entries each, base: n + 1; returns ms_plan_call's code
int mt_plan(void *h, int mode, int cap, int n, const int32_t *ids, const uint8_t *const *packets, const int32_t *lens) {
    return ((Mt *)h)->run_plan(mode, cap, n, ids, packets, lens);
}
int mt_plan_get(void *h, int32_t *first, int32_t *cnt, int32_t *eres, int32_t *placed, int64_t *base) {
    const ogh::MsCallPlan &p = ((Mt *)h)->plan;
    const size_t e = 4 * (size_t)p.n * p.S;
    if (p.first.size() * 4 != e || p.cnt.size() * 4 != e || p.eres.size() * 4 != e || p.placed.size() * 4 != e || p.base.size() != (size_t)p.n + 1) return -1;
    memcpy(first, p.first.data(), e), memcpy(cnt, p.cnt.data(), e), memcpy(eres, p.eres.data(), e), memcpy(placed, p.placed.data(), e);
    for (int i = 0; i <= p.n; i++) base[i] = (int64_t)p.base[i];
    return (int)p.frames.size();
}
void mt_frames(void *h, opusgpu_frame_desc *out) {
    const ogh::MsCallPlan &p = ((Mt *)h)->plan;
    memcpy(out, p.frames.data(), sizeof(*out) * p.frames.size());
}
// the arena's size; its bytes into `out` when `room` holds them
int64_t mt_arena(void *h, const uint8_t *const *packets, uint8_t *out, int64_t room) {
    const std::vector<uint8_t> a = ogh::ms_fill_arena(((Mt *)h)->plan, packets);
    if ((int64_t)a.size() <= room) memcpy(out, a.data(), a.size());
    return (int64_t)a.size();
}
// step k's tables: m[h] = frames of half h; returns ms_step_tables' answer
int mt_step(void *h, int k, int32_t m[2]) {
    Mt *t = (Mt *)h;
    const bool more = ogh::ms_step_tables(t->lay, t->plan, k, t->tab);
    for (int x = 0; x < 2; x++) {
        m[x] = (int32_t)t->tab[x].tab.size();
        if (t->tab[x].place.size() != 2 * t->tab[x].tab.size() || t->tab[x].owner.size() != t->tab[x].tab.size()) return -1;
    }
    return more ? 1 : 0;
}
void mt_table(void *h, int half, opusgpu_frame_desc *tab, int32_t *place, int32_t *owner) {
    const ogh::MsStepTable &t = ((Mt *)h)->tab[half];
    memcpy(tab, t.tab.data(), sizeof(*tab) * t.tab.size());
    memcpy(place, t.place.data(), 4 * t.place.size());
    memcpy(owner, t.owner.data(), 4 * t.owner.size());
}
void mt_fold(void *h, int half, const int32_t *got) { ogh::ms_fold_step(((Mt *)h)->plan, ((Mt *)h)->tab[half], got); }
int mt_results(void *h, int half, int32_t *out) {
    const std::vector<int32_t> r = ogh::ms_half_results(((Mt *)h)->lay, ((Mt *)h)->plan, half);
    memcpy(out, r.data(), 4 * r.size());
    return (int)r.size();
}
}

#ifdef MT_MAIN
#include <stdio.h>
int main() {
    uint32_t x = 4321;
    auto rnd = [&](uint32_t m) { return ((x = x * 1664525u + 1013904223u) >> 8) % m; };
    long frames = 0, refused = 0, failed = 0;
    for (int it = 0; it < 3000; it++) {
        opusgpu_ms_layout lay{};
        lay.streams = 1 + (int)rnd(5), lay.coupled = (int)rnd(lay.streams + 1), lay.channels = 1;
        const int S = lay.streams, n_dec = 1 + (int)rnd(4), n = 1 + (int)rnd(6), cap = 1 + (int)rnd(6);
        const int mode = it & 1 ? OPUSGPU_MODE_RFC : OPUSGPU_MODE_REFERENCE;
        Mt mt(lay, n_dec);
        for (int call = 0; call < 3; call++) {
            std::vector<std::vector<uint8_t>> pk(n); // (exactly len bytes each: a read past a packet is the sanitizer's)
            std::vector<const uint8_t *> ptr(n);
            std::vector<int32_t> len(n), ids(n);
            for (int i = 0; i < n; i++) {
                ids[i] = (int)rnd(n_dec + 1) - (rnd(8) == 0); // (now and then out of range)
                const uint8_t toc = (uint8_t)(rnd(32) << 3);
                const int count = 1 + (int)rnd(3);
                for (int s = 0; s < S && rnd(9); s++) { // code 3, CBR, `count` frames of `sz` bytes; self-delimited but for the last stream
                    const int sz = (int)rnd(40);
                    pk[i].push_back((uint8_t)(toc | rnd(2) << 2 | 3));
                    pk[i].push_back((uint8_t)(rnd(7) ? count : rnd(64)));
                    if (s != S - 1) pk[i].push_back((uint8_t)sz);
                    for (int b = 0; b < sz * count; b++) pk[i].push_back((uint8_t)rnd(256));
                }
                if (rnd(4) == 0 && pk[i].size() > 1) { // damage: cut, or change a byte
                    if (rnd(2))
                        pk[i].resize(1 + rnd((uint32_t)pk[i].size() - 1));
                    else
                        pk[i][rnd((uint32_t)pk[i].size())] = (uint8_t)rnd(256);
                }
                if (rnd(6) == 0) pk[i].clear();
                len[i] = rnd(40) ? (int32_t)pk[i].size() : -1;
                ptr[i] = pk[i].empty() ? nullptr : pk[i].data();
            }
            if (mt.run_plan(mode, cap, n, ids.data(), ptr.data(), len.data())) return 1;
            const ogh::MsCallPlan &p = mt.plan;
            const std::vector<uint8_t> arena = ogh::ms_fill_arena(p, ptr.data());
            for (size_t e = 0; e < p.eres.size(); e++) refused += p.eres[e] < 0;
            for (int k = 0; ogh::ms_step_tables(lay, p, k, mt.tab); k++) {
                if (k >= 48) return 2;
                for (int h = 0; h < 2; h++) {
                    const ogh::MsStepTable &t = mt.tab[h];
                    std::vector<int32_t> got(t.tab.size()); // (exactly one code per frame)
                    for (size_t j = 0; j < got.size(); j++) {
                        const opusgpu_frame_desc &d = t.tab[j];
                        if (d.offset < 0 || d.len < 0 || (size_t)d.offset + d.len + 16 > arena.size() || d.stream < 0 ||
                            d.stream >= (int)mt.last_count[h].size() || t.place[2 * j] < 0 || t.place[2 * j] >= n * ogh::ms_half(lay, h).streams) {
                            fprintf(stderr, "a descriptor or placement out of bounds at %d\n", it);
                            return 3;
                        }
                        got[j] = rnd(10) ? (mode == OPUSGPU_MODE_RFC ? ogh::flags_frame_size(d.flags) : OPUSGPU_FRAME_SAMPLES) : -18;
                        failed += got[j] < 0;
                    }
                    frames += (long)got.size();
                    ogh::ms_fold_step(mt.plan, t, got.data());
                }
            }
            for (int h = 0; h < 2; h++)
                if (ogh::ms_half_results(lay, p, h).size() != (size_t)n * ogh::ms_half(lay, h).streams) return 4;
        }
    }
    printf("multistream plan under the sanitizers: %ld frames in step tables (%ld failed), %ld refused streams\n", frames, failed, refused);
    return frames > 10000 && failed > 1000 && refused > 1000 ? 0 : 5;
}
#endif
