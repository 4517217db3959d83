// og_ms_framing.hpp -- what the multistream host path decides (host code only: nothing of HIP is needed, tests/emul/
// og_ms_framing_test.cpp compiles it with a plain C++ compiler and tests/test_ms_host_plan.py checks it on the CPU): the layout
// checks, the framing of one multistream packet, what a HALF of a layout is, the plan of a call -- every refusal, every count, the
// arena's prefix sums --, its step tables and what the returned codes do to them.  opusgpu_ms_decode_packets (og_ms.hpp) grows
// buffers, copies and launches around these functions and decides nothing.
#pragma once
#include <string.h>
#include <vector>
#include "og_host_framing.hpp"

namespace ogh {

// opus_multistream_decoder_init's argument checks and validate_layout (src/opus_decoder.cpp:742-770, :688-697)
inline bool ms_layout_ok(const opusgpu_ms_layout *l) {
    if (!l || l->channels > 255 || l->channels < 1 || l->coupled > l->streams || l->streams < 1 || l->coupled < 0 ||
        l->streams > 255 - l->coupled)
        return false;
    for (int c = 0; c < l->channels; c++)
        if (l->mapping[c] >= l->streams + l->coupled && l->mapping[c] != 255) return false;
    return true;
}

// samples of one (elementary) packet as opus_packet_get_nb_samples counts them (src/opus_decoder.cpp:477-504)
inline int ms_nb_samples(const uint8_t *p, int32_t len) {
    if (len < 1) return OPUSGPU_BAD_ARG;
    const int code = p[0] & 3;
    int count = code == 0 ? 1 : code != 3 ? 2 : -1;
    if (code == 3) {
        if (len < 2) return OPUSGPU_INVALID_PACKET;
        count = p[1] & 0x3F;
    }
    const int samples = count * toc_samples_per_frame(p[0], 48000);
    return samples * 25 > 48000 * 3 ? OPUSGPU_INVALID_PACKET : samples;
}

// opusgpu_ms_packet_to_frames (include/opusgpu.h) behind its argument checks: descs[s * 48 + k] = frame k of elementary stream s
// (offsets from `packet`, stream = `decoder`), counts[s] = its frames; returns the packet's samples or a negative code
inline int ms_packet_to_frames(const opusgpu_ms_layout &layout, const uint8_t *packet, int32_t len, int32_t decoder, int mode,
                               opusgpu_frame_desc *descs, int32_t *counts) {
    const int S = layout.streams;
    // opus_multistream_decode_native (:855-865) and opus_multistream_packet_validate (:803-823)
    if (len == 0 || len < 2 * S - 1) return OPUSGPU_INVALID_PACKET;
    const uint8_t *data = packet;
    int samples = 0;
    for (int s = 0; s < S; s++) {
        if (len <= 0) return OPUSGPU_INVALID_PACKET;
        int16_t size[48];
        uint8_t toc;
        int off = 0;
        int32_t packet_offset = 0;
        const int count = parse_packet(data, len, s != S - 1, &toc, size, &off, &packet_offset);
        if (count < 0) return count;
        const int tmp = ms_nb_samples(data, packet_offset);
        if (tmp < 0) return tmp;
        if (s != 0 && samples != tmp) return OPUSGPU_INVALID_PACKET;
        samples = tmp;
        const int32_t flags = mode == OPUSGPU_MODE_RFC ? toc_flags_rfc(toc) : toc_flags(toc);
        int32_t at = (int32_t)(data - packet) + off;
        for (int k = 0; k < count; k++) {
            descs[s * 48 + k] = opusgpu_frame_desc{decoder, at, size[k], flags};
            at += size[k];
        }
        counts[s] = count;
        data += packet_offset;
        len -= packet_offset;
    }
    // Reference mode decodes every frame as 960 samples (Q6): streams of equal durations but different frame counts would give
    // different sample counts, and the reference's loop would overrun its buffer.  Refused here.
    if (mode == OPUSGPU_MODE_REFERENCE)
        for (int s = 1; s < S; s++)
            if (counts[s] != counts[0]) return OPUSGPU_INVALID_PACKET;
    return samples;
}

// A HALF of a layout: the elementary streams that one of an opusgpu_ms's two contexts decodes.  Half 0: the coupled streams
// [0, coupled) on the 2-channel context, half 1: the mono streams [coupled, streams) on the 1-channel one; either may be empty.
// index(d, s): the context's stream that decodes stream s of decoder d -- and, with a packet's or row's number for d, its row in
// the half's [rows * streams] tables and PCM.  Host code spells this rule here and nowhere else (k_ms_split: the device's copy).
struct MsHalfLayout {
    int first, streams, channels;
    bool has(int s) const { return s >= first && s < first + streams; }
    int index(int d, int s) const { return d * streams + (s - first); }
};
inline MsHalfLayout ms_half(const opusgpu_ms_layout &l, int h) {
    return h ? MsHalfLayout{l.coupled, l.streams - l.coupled, 1} : MsHalfLayout{0, l.coupled, 2};
}

// a half's stream memory (og_host_framing.hpp): its context's arrays, n_streams entries
struct MsMemory {
    int32_t *last_count, *last_flags;
    int n_streams;
};

// The plan of one call.  Per (packet i, elementary stream s), e = i * S + s: its frames are frames[first[e] .. + cnt[e]) -- stream =
// the half's stream index, offsets into the arena --, eres[e] = samples decoded so far or the first negative code (a refused packet:
// the refusal in every stream, and no frames), placed[e] = samples gathered so far.  base[i]: packet i's bytes in the arena.
struct MsCallPlan {
    int n = 0, S = 0;
    std::vector<int32_t> first, cnt, eres, placed;
    std::vector<opusgpu_frame_desc> frames;
    std::vector<size_t> base;
};

// Framing pass 1 of a call.  OPUSGPU_BAD_ARG: the arena outgrows the descriptors' 32-bit offsets (split the call).  A packet that
// passes every check is remembered by its streams (remember_packet); empty, lost and refused packets leave the memory alone.
inline int ms_plan_call(const opusgpu_ms_layout &L, int n_decoders, int mode, int frame_capacity, int n, const int32_t *decoder_ids,
                        const uint8_t *const *packets, const int32_t *lens, const MsMemory mem[2], MsCallPlan &p) {
    const int S = L.streams;
    const bool rfc = mode == OPUSGPU_MODE_RFC;
    const MsHalfLayout half[2] = {ms_half(L, 0), ms_half(L, 1)};
    // frame_size as opus_multistream_decode_native limits it (:840: at most 120 ms)
    const int frame_size = frame_capacity * OPUSGPU_FRAME_SAMPLES < 5760 ? frame_capacity * OPUSGPU_FRAME_SAMPLES : 5760;
    p.n = n, p.S = S;
    p.first.assign((size_t)n * S, 0), p.cnt.assign((size_t)n * S, 0), p.eres.assign((size_t)n * S, 0), p.placed.assign((size_t)n * S, 0);
    p.base.assign((size_t)n + 1, 0);
    p.frames.clear();
    p.frames.reserve((size_t)n * S);
    std::vector<opusgpu_frame_desc> tmp((size_t)S * 48);
    std::vector<int32_t> tcnt(S);
    for (int i = 0; i < n; i++) {
        const int d = decoder_ids[i];
        const bool empty = !packets[i] || lens[i] == 0;
        p.base[i + 1] = p.base[i] + (empty || lens[i] < 0 ? 0 : (size_t)lens[i]);
        int code = 0;
        if (d < 0 || d >= n_decoders || lens[i] < 0)
            code = OPUSGPU_BAD_ARG;
        else if (empty) {
            for (int s = 0; s < S; s++) { // every elementary stream, as do_plc does (:851-874): the empty-packet branch, frame_size /
                                          // 960 passes (include/opusgpu.h EMPTY PACKETS); RFC mode: a lost packet, concealed
                const int h = half[1].has(s);
                const int e = half[h].index(d, s);
                const PacketPlan pp = plan_packet(nullptr, 0, e, mem[h].n_streams, mode, false, half[h].channels,
                                                  rfc ? frame_capacity : frame_size / OPUSGPU_FRAME_SAMPLES, mem[h].last_count[e], mem[h].last_flags[e], nullptr);
                if (pp.code) code = pp.code;
                tcnt[s] = plan_descs(pp, nullptr, 0, e, mode, 0, nullptr, &tmp[s * 48]);
            }
        } else {
            const int samples = ms_packet_to_frames(L, packets[i], lens[i], d, mode, tmp.data(), tcnt.data());
            if (samples < 0)
                code = samples;
            else if (samples > frame_size)
                code = OPUSGPU_BUFFER_TOO_SMALL; // (:845-847)
            else if (!rfc && (tcnt[0] > frame_capacity || (S > 1 && toc_samples_per_frame(packets[i][0], 48000) > OPUSGPU_FRAME_SAMPLES)))
                // every frame decodes as 960 samples (Q6): more frames than the room (as opusgpu_decode_packets); and the
                // reference's second stream is checked against the first one's 960-per-frame count (:880, frame_size = ret),
                // which frames of 40 / 60 ms fail -- decided here, before anything is decoded
                code = OPUSGPU_BUFFER_TOO_SMALL;
            else
                for (int s = 0; s < S; s++) { // the TOC an empty packet of this stream decodes as (:327-331)
                    const int h = half[1].has(s);
                    const int e = half[h].index(d, s);
                    remember_packet(decoded_plan(tcnt[s], tmp[s * 48].flags), &mem[h].last_count[e], &mem[h].last_flags[e]);
                    for (int k = 0; k < tcnt[s]; k++) {
                        tmp[s * 48 + k].stream = e;
                        tmp[s * 48 + k].offset += (int32_t)p.base[i];
                    }
                }
        }
        for (int s = 0; s < S; s++) {
            const size_t e = (size_t)i * S + s;
            p.first[e] = (int32_t)p.frames.size();
            if (code) {
                p.eres[e] = code;
                continue;
            }
            p.cnt[e] = tcnt[s];
            p.frames.insert(p.frames.end(), &tmp[s * 48], &tmp[s * 48] + tcnt[s]);
        }
    }
    return p.base[n] > 0x7fffffffu ? OPUSGPU_BAD_ARG : OPUSGPU_OK; // descriptor offsets are 32-bit
}

// the arena: packet i's bytes at base[i] (nothing for an empty or refused-as-negative one), 16 zero bytes of tail
inline std::vector<uint8_t> ms_fill_arena(const MsCallPlan &p, const uint8_t *const *packets) {
    std::vector<uint8_t> arena(p.base[p.n] + 16, 0);
    for (int i = 0; i < p.n; i++)
        if (p.base[i + 1] > p.base[i]) memcpy(arena.data() + p.base[i], packets[i], p.base[i + 1] - p.base[i]);
    return arena;
}

// Step k of a half: frame k of every elementary stream of the half that has one and has not failed, in (packet, stream) order.
// place: (row, at) per frame for k_ms_gather -- the half's accumulator row and the samples placed so far; owner: the frame's e.
struct MsStepTable {
    std::vector<opusgpu_frame_desc> tab;
    std::vector<int32_t> place, owner;
};
// false: no stream has a frame k left -- the call's steps are over
inline bool ms_step_tables(const opusgpu_ms_layout &L, const MsCallPlan &p, int k, MsStepTable t[2]) {
    const MsHalfLayout half[2] = {ms_half(L, 0), ms_half(L, 1)};
    for (int h = 0; h < 2; h++) t[h].tab.clear(), t[h].place.clear(), t[h].owner.clear();
    for (int i = 0; i < p.n; i++)
        for (int s = 0; s < p.S; s++) {
            const size_t e = (size_t)i * p.S + s;
            if (p.cnt[e] <= k || p.eres[e] < 0) continue;
            const int h = half[1].has(s);
            t[h].tab.push_back(p.frames[p.first[e] + k]);
            t[h].place.push_back(half[h].index(i, s));
            t[h].place.push_back(p.placed[e]);
            t[h].owner.push_back((int32_t)e);
        }
    return !t[0].tab.empty() || !t[1].tab.empty();
}
// ... and the codes a half's step returned, one per frame of its table
inline void ms_fold_step(MsCallPlan &p, const MsStepTable &t, const int32_t *got) {
    for (size_t j = 0; j < t.owner.size(); j++) {
        const size_t e = (size_t)t.owner[j];
        if (got[j] < 0)
            p.eres[e] = got[j]; // a failing frame ends its stream's packet, as opus_decode_native stops (:336-339)
        else {
            p.eres[e] += got[j];
            p.placed[e] += got[j];
        }
    }
}

// eres as k_ms_map reads it: a half's results, [n * half streams]
inline std::vector<int32_t> ms_half_results(const opusgpu_ms_layout &L, const MsCallPlan &p, int h) {
    const MsHalfLayout half = ms_half(L, h);
    std::vector<int32_t> r((size_t)p.n * half.streams);
    for (int i = 0; i < p.n; i++)
        for (int s = half.first; s < half.first + half.streams; s++) r[half.index(i, s)] = p.eres[(size_t)i * p.S + s];
    return r;
}

} // namespace ogh
