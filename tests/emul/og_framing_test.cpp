// TEST-ONLY: the host framing of the host-buffer path (csrc/og_host_framing.hpp) behind a C interface for tests/test_host_framing.py.
// Host code only.  With -DFT_MAIN (make framing_asan) a program of its own: random packets through plan_packet + plan_descs into
// buffers of exactly plan.frames descriptors, for the address / undefined-behaviour sanitizers to watch.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "og_host_framing.hpp"

// One packet through both framing passes.  plan[8]: code, frames, flags, kind, in_arena, pieces, and the stream memory after
// remember_packet.  descs: room for `room` descriptors -- written only when the plan's frames fit; returns what plan_descs
// returned, -1000 when the room is too small, -2000 when plan_descs left a descriptor unwritten or wrote past plan.frames.
extern "C" int ft_plan(const uint8_t *packet, int32_t len, int32_t stream, int n_streams, int mode, int fec, int channels, int frame_capacity,
                       int32_t last_count, int32_t last_flags, int32_t arena_base, int32_t plan[8], opusgpu_frame_desc *descs, int room) {
    int32_t conceal[48];
    const ogh::PacketPlan p = ogh::plan_packet(packet, len, stream, n_streams, mode, fec != 0, channels, frame_capacity, last_count, last_flags, conceal);
    ogh::remember_packet(p, &last_count, &last_flags);
    const int32_t out[8] = {p.code, p.frames, p.flags, p.kind, p.in_arena, p.pieces, last_count, last_flags};
    memcpy(plan, out, sizeof(out));
    if (p.frames > room) return -1000;
    const opusgpu_frame_desc mark{-77, -77, -77, -77};
    std::vector<opusgpu_frame_desc> d((size_t)p.frames + 4, mark);
    const int wrote = ogh::plan_descs(p, packet, len, stream, mode, arena_base, conceal, d.data());
    for (int k = 0; k < p.frames + 4; k++)
        if ((memcmp(&d[k], &mark, sizeof(mark)) == 0) != (k >= p.frames)) return -2000;
    memcpy(descs, d.data(), sizeof(mark) * (size_t)p.frames);
    return wrote;
}
extern "C" int ft_conceal_pieces(int total, int last_fs, int32_t base_flags, int32_t out_flags[48]) {
    return ogh::conceal_pieces(total, last_fs, base_flags, out_flags);
}
extern "C" int ft_is_regular(const uint8_t *packet, int32_t len, int32_t stream, int n_streams, int frame_capacity) {
    return ogh::is_regular_packet(packet, len, stream, n_streams, frame_capacity) ? 1 : 0;
}
extern "C" int32_t ft_lost_flags_no_packet_yet(int channels) { return ogh::lost_flags_no_packet_yet(channels); }

#ifdef FT_MAIN
#include <stdio.h>
int main() {
    uint32_t x = 12345;
    auto rnd = [&](uint32_t m) { return ((x = x * 1664525u + 1013904223u) >> 8) % m; };
    long checked = 0;
    for (int it = 0; it < 200000; it++) {
        const int len = it % 7 == 0 ? 0 : 1 + (int)rnd(it % 5 ? 64 : 1400);
        std::vector<uint8_t> pkt((size_t)len); // (exactly len bytes: a read past the packet is the sanitizer's)
        for (auto &b : pkt) b = (uint8_t)rnd(256);
        if (len > 2 && it % 3 == 0) pkt[1] = (uint8_t)((pkt[1] & 0xC0) | rnd(50));
        const int mode = it & 1 ? OPUSGPU_MODE_RFC : OPUSGPU_MODE_REFERENCE, fec = mode == OPUSGPU_MODE_RFC && it % 4 == 1;
        const int cap = 1 + (int)rnd(7), lc = (int)rnd(4) ? 1 + (int)rnd(48) : 0;
        const uint8_t last_toc = (uint8_t)rnd(256);
        const int32_t lf = lc ? (mode == OPUSGPU_MODE_RFC ? ogh::toc_flags_rfc(last_toc) : ogh::toc_flags(last_toc)) : 0;
        int32_t conceal[48];
        const ogh::PacketPlan p = ogh::plan_packet(len ? pkt.data() : nullptr, len, (int)rnd(5) - 1, 3, mode, fec, 1 + (int)rnd(2), cap, lc, lf, conceal);
        std::vector<opusgpu_frame_desc> d((size_t)p.frames);
        if (ogh::plan_descs(p, pkt.data(), len, 0, mode, 1000, conceal, d.data()) != p.frames || (p.code != 0 && p.frames != 0)) {
            fprintf(stderr, "plan and descriptors disagree at %d\n", it);
            return 1;
        }
        checked += p.frames;
    }
    printf("framing under the sanitizers: %ld descriptors\n", checked);
    return 0;
}
#endif
