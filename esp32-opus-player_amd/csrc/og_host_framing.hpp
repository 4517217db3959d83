// og_host_framing.hpp -- what one packet of a host-buffer call becomes, decided ONCE (host code only: nothing of HIP is needed,
// tests/emul/og_framing_test.cpp compiles it with a plain C++ compiler and tests/test_host_framing.py checks it on the CPU).
//
// opusgpu_decode_packets / _fec (og_host_path.hpp) and opusgpu_ms_decode_packets (through og_ms_framing.hpp's ms_plan_call: plan_packet
// and plan_descs for its empty packets, remember_packet for its decoded ones) frame in two passes with the prefix sums that
// place every packet between them: plan_packet is the first pass -- every result code, every count, the kind of the
// packet --, plan_descs the second: it writes what the plan says and decides nothing.  The flags of a stream that has had no
// packet yet and the stream memory an empty / lost packet is decoded from (last_count, last_flags) are spelled here and nowhere else.
#pragma once
#include "og_packet.hpp"

namespace ogh {

// descriptors of one packet (opusgpu_packet_to_frames_mode, include/opusgpu.h; packet != null, len > 0)
inline int packet_to_frames_mode(const uint8_t *packet, int32_t len, int32_t stream, int mode, opusgpu_frame_desc descs[48]) {
    int16_t size[48];
    uint8_t toc;
    int offset = 0;
    const int count = parse_packet(packet, len, 0, &toc, size, &offset, nullptr);
    if (count < 0) return count;
    const int32_t flags = mode == OPUSGPU_MODE_RFC ? toc_flags_rfc(toc) : toc_flags(toc);
    for (int i = 0; i < count; i++) {
        descs[i] = opusgpu_frame_desc{stream, offset, size[i], flags};
        offset += size[i];
    }
    return count;
}

// RFC mode, a LOST packet of a stream that has had no packet yet: one 20 ms CELT-only fullband frame of the decoder's channels
inline int32_t lost_flags_no_packet_yet(int decoder_channels) {
    return (MODE_CELT - MODE_SILK) | 4 << 2 | (decoder_channels == 2 ? 32 : 0) | 1 << 9;
}
// Reference mode, the flags of an empty packet's frames: the stream's last packet's mode / bandwidth / channels (toc_flags: bits
// 0 - 5, all that one mode ever stores), negative `last_flags` = none yet
inline int32_t empty_flags(int32_t last_flags, int decoder_channels) {
    return last_flags >= 0 ? (last_flags & 63) : empty_flags_no_packet_yet(decoder_channels);
}

// How a concealment of `total` samples is cut into device frames (valid duration codes): a frame of the last packet's size at a
// time like opus_decode(NULL) (src/opus_decoder.cpp:294-308 has the loop), what is left over (30 / 50 ms) as 20 / 40 ms + 10 ms.
inline int conceal_pieces(int total, int last_fs, int32_t base_flags, int32_t out_flags[48]) {
    static const int kDur[6] = {2880, 1920, 960, 480, 240, 120}, kCode[6] = {5, 4, 0, 3, 2, 1};
    int n = 0;
    while (total > 0) {
        int w = total < last_fs ? total : last_fs;
        total -= w;
        while (w > 0) {
            int j = 0;
            while (kDur[j] > w) j++;
            if (n == 48) return -1;
            out_flags[n++] = (base_flags & ~(7 << 6) & ~(1 << 10)) | kCode[j] << 6 | 1 << 9;
            w -= kDur[j];
        }
    }
    return n;
}

enum PlanKind : uint8_t {
    PLAN_DECODED,      // the packet's own frames
    PLAN_EMPTY,        // empty (reference mode) or lost (RFC mode): frames of no bytes from the stream memory
    PLAN_FEC,          // decode_fec: concealment pieces, then the packet's first frame with the FEC bit (bit 10)
    PLAN_CONCEAL_ONLY, // decode_fec without usable FEC data: concealment pieces only
};
struct PacketPlan {
    int32_t code = 0;   // the packet's result code, or 0
    int32_t frames = 0; // descriptors plan_descs writes (0: nothing is decoded -- `code` says why)
    int32_t flags = 0;  // PLAN_DECODED: the first frame's flags (what the stream memory takes); PLAN_EMPTY: every frame's flags
    PlanKind kind = PLAN_DECODED;
    uint8_t in_arena = 0; // the packet's bytes go into the arena
    uint8_t pieces = 0;   // the FEC kinds: concealment pieces (their flags: plan_packet's conceal_flags)
};
inline PacketPlan refused(int code) { return PacketPlan{code, 0, 0, PLAN_DECODED, 0, 0}; }
inline PacketPlan decoded_plan(int count, int32_t first_flags) { return PacketPlan{0, count, first_flags, PLAN_DECODED, 1, 0}; }

// ONE look at the TOC settles the common packet: one frame (frame-count code 0) of a stream that exists, of a size and duration
// the call has room for -- reference mode, no FEC: exactly the packets plan_packet answers with decoded_plan(1, toc_flags(toc))
inline bool is_regular_packet(const uint8_t *p, int32_t len, int32_t stream, int n_streams, int frame_capacity) {
    return stream >= 0 && stream < n_streams && p && len >= 1 && len <= 1276 && (p[0] & 3) == 0 &&
           toc_samples_per_frame(p[0], 48000) <= frame_capacity * OPUSGPU_FRAME_SAMPLES;
}

// decode_fec: the packet BEFORE this one was lost (opus_decode with decode_fec = 1): its duration is concealed, the last frame's
// worth of it from this packet's first frame where SILK data is there to carry LBRR frames
inline PacketPlan plan_fec(uint8_t toc, int32_t first_flags, int frame_capacity, int32_t lc, int32_t last_flags, int32_t conceal_flags[48]) {
    const int last_fs = lc ? flags_frame_size(last_flags) : 120;
    const int lost_dur = lc ? lc * last_fs : OPUSGPU_FRAME_SAMPLES;
    const int pfs = toc_samples_per_frame(toc, 48000);
    const bool celt = (first_flags & 3) == 2 || (lc && (last_flags & 3) == 2);
    if (lost_dur > frame_capacity * OPUSGPU_FRAME_SAMPLES) return refused(OPUSGPU_BUFFER_TOO_SMALL);
    const bool use = !(lost_dur < pfs || celt);
    const int np = conceal_pieces(use ? lost_dur - pfs : lost_dur, last_fs, lc ? last_flags : first_flags, conceal_flags);
    if (np < 0 || np + (use ? 1 : 0) > 48) return refused(OPUSGPU_BAD_ARG);
    return PacketPlan{0, np + (use ? 1 : 0), 0, use ? PLAN_FEC : PLAN_CONCEAL_ONLY, (uint8_t)use, (uint8_t)np};
}

// Framing pass 1 (opus_decode_native, src/opus_decoder.cpp:280-348).  `last_count` / `last_flags`: the stream memory (read only
// for a stream that exists); `conceal_flags`: where the pieces' flags of the FEC kinds go (needed when `fec`).
inline PacketPlan plan_packet(const uint8_t *packet, int32_t len, int32_t stream, int n_streams, int mode, bool fec, int channels,
                              int frame_capacity, int32_t last_count, int32_t last_flags, int32_t conceal_flags[48]) {
    const bool rfc = mode == OPUSGPU_MODE_RFC;
    if (stream < 0 || stream >= n_streams || len < 0) return refused(OPUSGPU_BAD_ARG);
    if (!packet || len == 0) {
        if (!rfc)
            // The reference has no concealment, but opus_decode_native's empty-packet branch is live (src/opus_decoder.cpp:
            // 290-308): opus_decode_frame(st, NULL, 0) -- a frame of no bytes in the stream's LAST mode / bandwidth / channel
            // count, 960 samples per pass -- until frame_size (here frame_capacity x 960, a multiple of 120) is filled or a
            // pass fails: SILK-only decodes (the coder reads zeros), hybrid runs its SILK half and ends in CELT's -18
            // (src/celt.cpp:2225), CELT-only in -18; a stream without a packet since its reset is in mode 0 (descriptor bit 11)
            return PacketPlan{0, frame_capacity, empty_flags(last_count ? last_flags : -1, channels), PLAN_EMPTY, 0, 0};
        // RFC mode: a lost packet is concealed as long as the stream's last packet was (one 20 ms frame if there was none)
        const int count = last_count ? last_count : 1;
        if ((int64_t)count * flags_frame_size(last_flags) > (int64_t)frame_capacity * OPUSGPU_FRAME_SAMPLES) return refused(OPUSGPU_BUFFER_TOO_SMALL);
        return PacketPlan{0, count, last_count ? last_flags : lost_flags_no_packet_yet(channels), PLAN_EMPTY, 0, 0};
    }
    int16_t size[48];
    uint8_t toc;
    const int count = parse_packet(packet, len, 0, &toc, size, nullptr, nullptr);
    if (count < 0) return refused(count);
    const int32_t first_flags = rfc ? toc_flags_rfc(toc) : toc_flags(toc);
    if (fec) return plan_fec(toc, first_flags, frame_capacity, last_count, last_flags, conceal_flags);
    // count * packet_frame_size > frame_size -> OPUS_BUFFER_TOO_SMALL (src/opus_decoder.cpp:323)
    // (RFC mode decodes the durations the check is about: no second condition)
    if ((int64_t)count * toc_samples_per_frame(toc, 48000) > (int64_t)frame_capacity * OPUSGPU_FRAME_SAMPLES || (!rfc && count > frame_capacity))
        return refused(OPUSGPU_BUFFER_TOO_SMALL);
    return decoded_plan(count, first_flags);
}

// What a later empty packet of the stream decodes / conceals as: st->mode, bandwidth, stream_channels (src/opus_decoder.cpp:
// 327-331: set once the packet has passed every check of plan_packet, whatever its frames return).  Empty, lost and refused
// packets leave the memory alone -- and so do the FEC kinds (the packet itself is decoded by a call of its own afterwards).
inline void remember_packet(const PacketPlan &p, int32_t *last_count, int32_t *last_flags) {
    if (p.kind != PLAN_DECODED || !p.frames) return;
    *last_count = p.frames;
    *last_flags = p.flags;
}

// Framing pass 2: the plan's p.frames descriptors (the packet's bytes at `arena_base` of the arena when p.in_arena); returns p.frames
inline int plan_descs(const PacketPlan &p, const uint8_t *packet, int32_t len, int32_t stream, int mode, int32_t arena_base,
                      const int32_t *conceal_flags, opusgpu_frame_desc *out) {
    if (p.kind == PLAN_EMPTY) { // nothing to read: len 0, the flags of the stream's last packet (RFC mode: RFC bit and duration included)
        for (int k = 0; k < p.frames; k++) out[k] = opusgpu_frame_desc{stream, 0, 0, p.flags};
        return p.frames;
    }
    if (p.kind == PLAN_CONCEAL_ONLY || p.kind == PLAN_FEC)
        for (int k = 0; k < p.pieces; k++) out[k] = opusgpu_frame_desc{stream, 0, 0, conceal_flags[k]};
    if (p.kind == PLAN_CONCEAL_ONLY || !p.frames) return p.frames;
    opusgpu_frame_desc d[48];
    (void)packet_to_frames_mode(packet, len, stream, mode, d);
    const int own = p.kind == PLAN_FEC ? 1 : p.frames; // (PLAN_FEC: the first frame only, behind the pieces)
    for (int k = 0; k < own; k++) {
        d[k].offset += arena_base;
        if (p.kind == PLAN_FEC) d[k].flags |= 1 << 10;
        out[p.pieces + k] = d[k];
    }
    return p.frames;
}

} // namespace ogh
