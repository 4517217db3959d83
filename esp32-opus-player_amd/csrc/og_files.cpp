// og_files.cpp -- the file planner (include/opusgpu.h, "WHOLE FILES"): N complete Ogg Opus files -> decode steps, a packet
// arena and, per step, the segments that place every decoded frame's kept samples in its file's track.  Host only.
//
// The container bookkeeping is the single-file reader's own (og_container.hpp): every file is opened and drained through
// OpusFile::next_planned / commit, which is fill() without the decode.  Three passes: (1) per file, in parallel: run the reader,
// split every packet into frames, keep the frames' bytes and placements in a per-file plan; (2) sequential and cheap: track
// offsets, arena offsets, per-step (and per-key) slot numbering in file order; (3) per file, in parallel: copy the bytes into the
// arena and write descriptors and segments into their slots.
// opusgpu_ms_files_plan (WHOLE FILES / MULTISTREAM) is the same three passes and the same reader loop; its frames are rows of
// `streams` descriptors, framed by opusgpu_ms_packet_to_frames.
// opusgpu_files_plan_cuts / opusgpu_ms_files_plan_cuts (WHOLE FILES / CUTS) are the same passes again: pass 1 over the FILES, once
// each, passes 2 and 3 over TRACKS -- a track is a run of a file's frames with a window on the file's track; a whole file is the
// track that has all of them -- so a file's bytes lie in the arena once however many cuts point into them.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <new>
#include <thread>
#include <vector>
#include "og_batch.hpp"
#include "og_container.hpp"
#include "og_packet.hpp"
#include "../../include/opusgpu.h"

namespace {

struct FramePlan {
    int32_t flags; // of the frame's first descriptor
    int32_t src_first, count, packet_seq;
    int64_t dst_rel; // position in the track
    uint8_t key;     // sort key within a step (0 without grouping)
    uint8_t kept;    // the file has decoded frames of this frame's mode only, up to and including it
};

struct FilePlan {
    std::vector<FramePlan> frames;
    std::vector<opusgpu_frame_desc> descs; // `width` per frame (1, or the layout's streams); offsets into the file's own bytes
    std::vector<uint8_t> bytes;
    std::vector<int64_t> packet_start; // packets + 1 entries: the last one is the track length
    // What cuts are taken from afterwards (WHOLE FILES / CUTS), per packet: where its frames and its bytes begin and the decoded
    // samples in front of it (packets + 1 entries each, the last one the total), and what the reader discards at its front.  Empty
    // for a file without a planned packet.
    std::vector<uint32_t> packet_frame, packet_byte;
    std::vector<int64_t> packet_decoded;
    std::vector<int32_t> packet_skip;
};

// A track of the batch: frames [f0, f0 + n) of file `file`.  A whole file is all of its frames as they are; a cut (`cut`) keeps of
// every frame what lies in [start, start + count) of the file's track and counts packets from first_packet.
struct Track {
    int file = 0;
    bool cut = false;
    size_t f0 = 0, n = 0;
    size_t kept_n = 0; // cut: its first frames that are all of the first one's mode
    int32_t first_packet = 0, packets = 0;
    int64_t start = 0, count = 0;
};

template <class F>
void parallel_for(int n, int threads, F f) { // f(begin, end)
    threads = threads < 1 ? 1 : threads;
    if (threads > n / 16 + 1) threads = n / 16 + 1;
    if (threads <= 1) {
        f(0, n);
        return;
    }
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++) {
        const int b = (int)((int64_t)n * t / threads), e = (int)((int64_t)n * (t + 1) / threads);
        th.emplace_back([=] { f(b, e); });
    }
    for (auto &x : th) x.join();
}

// Opens the file and reports its OpusHead.  Returns the reader's code (OP_EIMPL as OPUSGPU_UNIMPLEMENTED).
int open_file(ogc::OpusFile &of, opusgpu_file_info &fi) {
    const int r = of.open();
    const ogc::Head &h = of.head();
    fi.channels = h.channel_count, fi.pre_skip = (int32_t)h.pre_skip, fi.output_gain = h.output_gain, fi.mapping_family = h.mapping_family;
    return r == ogc::OP_EIMPL ? OPUSGPU_UNIMPLEMENTED : r;
}

int refuse(opusgpu_file_info &fi, FilePlan &fp, int code) {
    fp = FilePlan();
    fp.packet_start.assign(1, 0);
    fi.packets = fi.frames = 0;
    return code;
}

// An open file through the reader, the loop both planners share.  split(packet, base, fr, &spf) frames one packet whose bytes will
// lie at `base` of fp.bytes: it appends the descriptors of the packet's frames to fp.descs, frame after frame, fills flags, key
// and kept of fr[0 .. count) and returns the frame count and the frames' duration -- or OPUSGPU_UNIMPLEMENTED, which refuses the
// file, or another negative code, which ends the plan there.  Returns the status; `fp` holds whatever was planned before a failure.
template <class Split>
int plan_packets(ogc::OpusFile &of, bool rfc, opusgpu_file_info &fi, FilePlan &fp, Split split) {
    int64_t pos = 0; // samples of the track so far
    int status = 0;
    fp.packet_frame.assign(1, 0), fp.packet_byte.assign(1, 0), fp.packet_decoded.assign(1, 0);
    for (;;) {
        ogc::OpusFile::Planned pl;
        const int ret = of.next_planned(pl);
        if (ret == 0) break;
        if (ret == ogc::OP_HOLE) {
            fi.holes++;
            continue;
        }
        if (ret < 0) {
            status = ret;
            break;
        }
        const std::vector<uint8_t> &pk = pl.pkt->data;
        FramePlan fr[48];
        int spf = 0;
        const size_t n_descs = fp.descs.size();
        const int count = split(pk, (int32_t)fp.bytes.size(), fr, &spf);
        if (count < 0 && count != OPUSGPU_UNIMPLEMENTED) { // (the reader's decode callback fails here)
            fp.descs.resize(n_descs);
            status = count;
            break;
        }
        // reference mode decodes every frame as 960 samples (Q6): refused, see the header
        if (count < 0 || (!rfc && spf != OPUSGPU_FRAME_SAMPLES)) return refuse(fi, fp, OPUSGPU_UNIMPLEMENTED);
        fp.bytes.insert(fp.bytes.end(), pk.begin(), pk.end());
        for (int k = 0; k < count; k++) { // the packet's PCM is its frames' back to back; samples [skip, trimmed) are kept
            const int lo = k * spf, hi = lo + spf;
            const int a = lo > pl.skip ? lo : pl.skip, b = hi < pl.trimmed ? hi : pl.trimmed;
            FramePlan &f = fr[k];
            f.count = b > a ? b - a : 0;
            f.src_first = f.count ? a - lo : 0;
            f.dst_rel = pos + (f.count ? a - pl.skip : 0);
            f.packet_seq = fi.packets;
            fp.frames.push_back(f);
        }
        of.commit(pl);
        pos += pl.trimmed > pl.skip ? pl.trimmed - pl.skip : 0;
        fp.packet_start.push_back(pos);
        fp.packet_frame.push_back((uint32_t)fp.frames.size()), fp.packet_byte.push_back((uint32_t)fp.bytes.size());
        fp.packet_decoded.push_back(fp.packet_decoded.back() + (int64_t)count * spf), fp.packet_skip.push_back(pl.skip);
        fi.packets++;
        if (fp.bytes.size() > 0x7fffffffu || fp.descs.size() > 0x3fffffffu) { // (one file: 32-bit offsets)
            status = OPUSGPU_ALLOC_FAIL;
            break;
        }
    }
    fi.frames = (int32_t)fp.frames.size();
    return status;
}

// One stereo or mono file (opusgpu_files_plan).
int plan_file(const uint8_t *data, size_t len, int channels, int mode, int flags, opusgpu_file_info &fi, FilePlan &fp) {
    ogc::OpusFile of(data, len);
    fp.packet_start.assign(1, 0);
    const int r = open_file(of, fi);
    if (r < 0) return r;
    if (fi.mapping_family != 0) return OPUSGPU_UNIMPLEMENTED;
    if (fi.channels != channels) return OPUSGPU_BAD_ARG;
    const bool rfc = mode == OPUSGPU_MODE_RFC;
    const bool by_header = (flags & OPUSGPU_PAGES_ORDER_BY_HEADER) != 0;
    const bool group = by_header || (flags & OPUSGPU_PAGES_GROUP_BY_MODE) != 0;
    int first_mode = -1;
    bool kept = true;
    return plan_packets(of, rfc, fi, fp, [&](const std::vector<uint8_t> &pk, int32_t base, FramePlan *fr, int *spf) {
        int16_t size[48];
        uint8_t toc;
        int off = 0;
        const int count = ogh::parse_packet(pk.data(), (int32_t)pk.size(), 0, &toc, size, &off, nullptr);
        if (count < 0) return (int)ogc::OP_EBADPACKET;
        *spf = ogh::toc_samples_per_frame(toc, 48000);
        const int32_t fl = rfc ? ogh::toc_flags_rfc(toc) : ogh::toc_flags(toc);
        const int m = fl & 3;
        if (first_mode < 0) first_mode = m;
        if (m != first_mode) kept = false;
        for (int k = 0; k < count; k++) {
            fp.descs.push_back(opusgpu_frame_desc{0, base + off, size[k], fl});
            const int key = by_header ? ogh::header_order_key(fl, size[k] > 0 ? pk[(size_t)off] : 0, size[k]) : group ? m : 0;
            fr[k].flags = fl, fr[k].key = (uint8_t)key, fr[k].kept = kept;
            off += size[k];
        }
        return count;
    });
}

bool same_layout(const ogc::Head &h, const opusgpu_ms_layout &l) {
    return h.channel_count == l.channels && h.stream_count == l.streams && h.coupled_count == l.coupled &&
           memcmp(h.mapping, l.mapping, (size_t)h.channel_count) == 0;
}

// One file of the batch's layout (opusgpu_ms_files_plan): a frame is a row of `streams` descriptors.
int plan_ms_file(const uint8_t *data, size_t len, const opusgpu_ms_layout &lay, int mode, opusgpu_file_info &fi, FilePlan &fp) {
    ogc::OpusFile of(data, len);
    fp.packet_start.assign(1, 0);
    const int r = open_file(of, fi);
    if (r < 0) return r;
    if (!same_layout(of.head(), lay)) return OPUSGPU_BAD_ARG;
    const bool rfc = mode == OPUSGPU_MODE_RFC;
    const int S = lay.streams;
    std::vector<opusgpu_frame_desc> el((size_t)S * 48);
    std::vector<int32_t> cnt((size_t)S);
    return plan_packets(of, rfc, fi, fp, [&](const std::vector<uint8_t> &pk, int32_t base, FramePlan *fr, int *spf) {
        if (opusgpu_ms_packet_to_frames(&lay, pk.data(), (int32_t)pk.size(), 0, mode, el.data(), cnt.data()) < 0)
            return (int)ogc::OP_EBADPACKET;
        *spf = ogh::toc_samples_per_frame(pk[0], 48000); // the reader's own view of the packet: elementary stream 0's TOC
        // the device step takes rows of one duration (RFC mode; reference mode's framing has refused unequal counts already)
        for (int s = 1; s < S; s++)
            if (cnt[s] != cnt[0] || ((el[(size_t)s * 48].flags ^ el[0].flags) & (7 << 6))) return OPUSGPU_UNIMPLEMENTED;
        for (int k = 0; k < cnt[0]; k++) {
            for (int s = 0; s < S; s++) {
                opusgpu_frame_desc d = el[(size_t)s * 48 + k];
                d.offset += base;
                fp.descs.push_back(d);
            }
            fr[k].flags = el[k].flags, fr[k].key = 0, fr[k].kept = 1;
        }
        return (int)cnt[0];
    });
}

} // namespace

namespace {

// What a batch of cuts is planned from (WHOLE FILES / CUTS); null: one track per file.
struct CutArgs {
    int n_cuts;
    const opusgpu_cut *cuts;
    int64_t stride;
    opusgpu_cut_info *cut_info; // may be null
    bool keeps_mode;            // the step masks carry OPUSGPU_STEP_KEEPS_MODE (the stereo / mono planner)
};

// One cut of a planned file: which packets it decodes and what of the track it keeps (include/opusgpu.h, WHICH PACKETS).
void resolve_cut(const FilePlan &fp, const opusgpu_cut &c, bool keeps_mode, Track &t, opusgpu_cut_info &ci) {
    const int64_t L = fp.packet_start.back();
    const int64_t start = c.start < 0 ? 0 : c.start > L ? L : c.start;
    const int64_t count = c.count < 0 || c.count > L - start ? L - start : c.count;
    t.cut = true, t.start = start, t.count = count;
    ci = opusgpu_cut_info{0, 0, 0, 1, start};
    if (count == 0) return;
    const int64_t *ps = fp.packet_start.data(), *D = fp.packet_decoded.data();
    const size_t n_p = fp.packet_start.size() - 1; // > 0: the track has samples
    const size_t pa = (size_t)(std::upper_bound(ps, ps + n_p + 1, start) - ps) - 1;
    const size_t pb = (size_t)(std::upper_bound(ps, ps + n_p + 1, start + count - 1) - ps) - 1;
    const int64_t preroll = c.preroll < 0 ? OPUSGPU_CUT_PREROLL : c.preroll;
    const int64_t in_pa = fp.packet_skip[pa] + (start - ps[pa]); // decoded samples of pa in front of `start`
    const int64_t most = D[pa] + in_pa - preroll;               // D[p] of a first packet may be at most this
    const size_t p = most < 0 ? 0 : (size_t)(std::upper_bound(D, D + pa + 1, most) - D) - 1;
    t.first_packet = (int32_t)p, t.packets = (int32_t)(pb - p + 1);
    t.f0 = fp.packet_frame[p], t.n = fp.packet_frame[pb + 1] - t.f0;
    t.kept_n = t.n;
    if (keeps_mode)
        for (size_t k = 1; k < t.n; k++)
            if ((fp.frames[t.f0 + k].flags ^ fp.frames[t.f0].flags) & 3) {
                t.kept_n = k;
                break;
            }
    ci.first_packet = t.first_packet, ci.packets = t.packets, ci.lead = (int32_t)(D[pa] - D[p] + in_pa), ci.exact = p == 0;
}

// Frame k of a track as the batch holds it.
inline FramePlan track_frame(const FilePlan &fp, const Track &t, size_t k) {
    FramePlan f = fp.frames[t.f0 + k];
    if (!t.cut) return f;
    const int64_t a = f.dst_rel > t.start ? f.dst_rel : t.start;
    const int64_t e = f.dst_rel + f.count < t.start + t.count ? f.dst_rel + f.count : t.start + t.count;
    if (f.count > 0 && e > a) {
        f.src_first += (int32_t)(a - f.dst_rel), f.count = (int32_t)(e - a), f.dst_rel = a - t.start;
    } else { // wholly in the pre-roll, or behind the cut's end in its last packet: decoded, nothing kept
        f.src_first = 0, f.count = 0;
        f.dst_rel = f.dst_rel <= t.start ? 0 : f.dst_rel - t.start < t.count ? f.dst_rel - t.start : t.count;
    }
    f.packet_seq -= t.first_packet;
    f.kept = k < t.kept_n;
    return f;
}

// Passes 1 to 3 over a new batch `b` (n_files = its tracks, width and mode set): plan(i, info, file plan) is pass 1 for file i of
// the n_src files; G sort keys.  ca: the cuts that are the batch's tracks, or null for one track per file.
// Returns OPUSGPU_OK, OPUSGPU_BAD_ARG (32-bit offsets exceeded, a stride that does not hold its cuts) or OPUSGPU_ALLOC_FAIL.
template <class Plan>
int build_batch(og_batch *b, int n_src, int threads, int G, opusgpu_file_info *info, const CutArgs *ca, Plan plan) {
    const int n_tracks = b->n_files;
    const size_t W = (size_t)b->width;
    try {
        std::vector<opusgpu_file_info> file_info((size_t)n_src, opusgpu_file_info{});
        std::vector<FilePlan> plans((size_t)n_src);
        std::atomic<bool> oom{false};
        // pass 1: the reader over every file
        parallel_for(n_src, threads, [&](int lo, int hi) {
            try {
                for (int i = lo; i < hi; i++) file_info[i].status = plan(i, file_info[i], plans[i]);
            } catch (const std::bad_alloc &) {
                oom = true;
            }
        });
        if (oom) throw std::bad_alloc();
        // the tracks, and the bytes of every file that they need
        std::vector<Track> tracks((size_t)n_tracks);
        std::vector<size_t> byte_lo((size_t)n_src, 0), byte_hi((size_t)n_src, 0);
        if (!ca) {
            for (int i = 0; i < n_src; i++) {
                tracks[i].file = i, tracks[i].n = plans[i].frames.size(), tracks[i].count = plans[i].packet_start.back();
                byte_hi[i] = plans[i].bytes.size();
            }
        } else {
            std::vector<opusgpu_cut_info> own;
            opusgpu_cut_info *ci = ca->cut_info;
            if (!ci) own.resize((size_t)n_tracks), ci = own.data();
            parallel_for(n_tracks, threads, [&](int lo, int hi) {
                for (int t = lo; t < hi; t++) {
                    tracks[t].file = ca->cuts[t].file;
                    resolve_cut(plans[tracks[t].file], ca->cuts[t], ca->keeps_mode, tracks[t], ci[t]);
                }
            });
            std::vector<uint8_t> seen((size_t)n_src, 0);
            for (int t = 0; t < n_tracks; t++) {
                const Track &tr = tracks[t];
                if (!tr.packets) continue;
                const FilePlan &fp = plans[tr.file];
                const size_t lo = fp.packet_byte[tr.first_packet], hi = fp.packet_byte[tr.first_packet + tr.packets];
                if (!seen[tr.file]) seen[tr.file] = 1, byte_lo[tr.file] = lo, byte_hi[tr.file] = hi;
                if (lo < byte_lo[tr.file]) byte_lo[tr.file] = lo;
                if (hi > byte_hi[tr.file]) byte_hi[tr.file] = hi;
            }
        }
        // pass 2: tracks, arena, steps
        const int64_t stride = ca ? ca->stride : 0;
        std::vector<size_t> arena_at((size_t)n_src + 1, 0);
        for (int i = 0; i < n_src; i++) arena_at[i + 1] = arena_at[i] + (byte_hi[i] - byte_lo[i]);
        b->info.assign((size_t)n_tracks, opusgpu_file_info{});
        b->packet_begin.assign((size_t)n_tracks + 1, 0);
        size_t n_steps = 0, total = 0;
        int64_t at = 0;
        for (int t = 0; t < n_tracks; t++) {
            const Track &tr = tracks[t];
            opusgpu_file_info &fi = b->info[t];
            fi = file_info[tr.file];
            if (tr.cut) fi.packets = tr.packets, fi.frames = (int32_t)tr.n;
            fi.track_samples = tr.count;
            if (stride) {
                if (tr.count > stride) return OPUSGPU_BAD_ARG;
                fi.track_offset = (int64_t)t * stride;
                at = fi.track_offset + stride;
            } else {
                fi.track_offset = at;
                at = (at + fi.track_samples + 63) / 64 * 64; // every track begins on a 128-byte boundary (mono: 64 samples)
            }
            b->packet_begin[t + 1] = b->packet_begin[t] + (tr.cut ? (size_t)tr.packets + 1 : plans[tr.file].packet_start.size());
            if (tr.n > n_steps) n_steps = tr.n;
            total += tr.n;
        }
        b->track_samples = at;
        b->track_stride = stride;
        if (arena_at[n_src] > 0x7fffffffu || total * W > 0x7fffffffu) return OPUSGPU_BAD_ARG; // descriptor offsets and slots are 32-bit: split the call
        // a counting sort of the frames by (step, key), stable in track order
        std::vector<size_t> cur(n_steps * G + 1, 0);
        for (int t = 0; t < n_tracks; t++) {
            const FramePlan *fr = plans[tracks[t].file].frames.data() + tracks[t].f0;
            for (size_t k = 0; k < tracks[t].n; k++) cur[k * G + fr[k].key + 1]++;
        }
        for (size_t j = 1; j < cur.size(); j++) cur[j] += cur[j - 1];
        b->step_begin.resize(n_steps + 1);
        for (size_t s = 0; s <= n_steps; s++) b->step_begin[s] = cur[s * G];
        std::vector<std::vector<uint32_t>> slot_of((size_t)n_tracks);
        b->step_modes.assign(n_steps, 0);
        std::vector<uint8_t> step_broken(n_steps, 0);
        for (int t = 0; t < n_tracks; t++) {
            const Track &tr = tracks[t];
            const FramePlan *fr = plans[tr.file].frames.data() + tr.f0;
            slot_of[t].resize(tr.n);
            for (size_t k = 0; k < tr.n; k++) {
                const FramePlan &f = fr[k];
                slot_of[t][k] = (uint32_t)cur[k * G + f.key]++;
                b->step_modes[k] |= 1 << (f.flags & 3);
                if (tr.cut ? k >= tr.kept_n : !f.kept) step_broken[k] = 1;
            }
        }
        for (size_t s = 0; s < n_steps; s++)
            if (!step_broken[s]) b->step_modes[s] |= OPUSGPU_STEP_KEEPS_MODE;
        // pass 3: bytes, descriptors, segments
        b->descs.resize(total * W);
        b->segs.resize(total);
        b->slot_files.resize(total);
        b->arena.assign(arena_at[n_src] + 16, 0); // the kernels fetch packets as aligned 16-byte pieces: keep a tail
        b->packet_start.resize(b->packet_begin[n_tracks]);
        parallel_for(n_src, threads, [&](int lo, int hi) { // a file's bytes once, however many tracks point into them
            for (int i = lo; i < hi; i++)
                if (byte_hi[i] > byte_lo[i]) memcpy(b->arena.data() + arena_at[i], plans[i].bytes.data() + byte_lo[i], byte_hi[i] - byte_lo[i]);
        });
        parallel_for(n_tracks, threads, [&](int lo, int hi) {
            for (int t = lo; t < hi; t++) {
                const Track &tr = tracks[t];
                const FilePlan &fp = plans[tr.file];
                int64_t *ps = b->packet_start.data() + b->packet_begin[t];
                if (!tr.cut) {
                    memcpy(ps, fp.packet_start.data(), fp.packet_start.size() * sizeof(int64_t));
                } else { // the cut's own table: 0 for the pre-roll packets, the cut's length behind its last one
                    for (int32_t j = 0; j <= tr.packets; j++) {
                        const int64_t v = tr.packets ? fp.packet_start[(size_t)tr.first_packet + (size_t)j] - tr.start : 0;
                        ps[j] = v < 0 ? 0 : v > tr.count ? tr.count : v;
                    }
                }
                const size_t base = arena_at[tr.file] - byte_lo[tr.file];
                for (size_t k = 0; k < tr.n; k++) {
                    const FramePlan f = track_frame(fp, tr, k);
                    const size_t slot = slot_of[t][k];
                    for (size_t w = 0; w < W; w++) {
                        const opusgpu_frame_desc &d = fp.descs[(tr.f0 + k) * W + w];
                        b->descs[slot * W + w] = opusgpu_frame_desc{t, (int32_t)(base + (size_t)d.offset), d.len, d.flags};
                    }
                    opusgpu_track_seg &sg = b->segs[slot];
                    sg.slot = (int32_t)(slot - b->step_begin[k]);
                    sg.src_first = f.src_first, sg.count = f.count, sg.track = t;
                    sg.dst_first = b->info[t].track_offset + f.dst_rel;
                    sg.packet_seq = f.packet_seq, sg.reserved = 0;
                    b->slot_files[slot] = t;
                }
            }
        });
        if (info && n_tracks) memcpy(info, b->info.data(), sizeof(opusgpu_file_info) * (size_t)n_tracks);
        return OPUSGPU_OK;
    } catch (const std::bad_alloc &) {
        return OPUSGPU_ALLOC_FAIL;
    }
}

// What both cut planners refuse before any file is read.
bool cuts_ok(int n_files, int n_cuts, const opusgpu_cut *cuts, int64_t track_stride) {
    if (n_cuts < 0 || (n_cuts > 0 && !cuts) || track_stride < 0 || track_stride % 64) return false;
    for (int t = 0; t < n_cuts; t++)
        if (cuts[t].file < 0 || cuts[t].file >= n_files) return false;
    return true;
}

bool files_ok(int n_files, const uint8_t *const *files, const int64_t *file_lens) {
    if (n_files < 0 || (n_files > 0 && (!files || !file_lens))) return false;
    for (int i = 0; i < n_files; i++)
        if (file_lens[i] < 0 || (file_lens[i] > 0 && !files[i])) return false;
    return true;
}

int batch_step(const og_batch *b, int step, const opusgpu_frame_desc **descs, const int32_t **slot_files, int *modes) {
    if (!b || step < 0 || step + 1 >= (int)b->step_begin.size()) return OPUSGPU_BAD_ARG;
    const size_t at = b->step_begin[step];
    if (descs) *descs = b->descs.data() + at * (size_t)b->width;
    if (slot_files) *slot_files = b->slot_files.data() + at;
    if (modes) *modes = b->step_modes[step];
    return (int)(b->step_begin[step + 1] - at);
}

int batch_segments(const og_batch *b, int step, const opusgpu_track_seg **segs) {
    if (!b || step < 0 || step + 1 >= (int)b->step_begin.size()) return OPUSGPU_BAD_ARG;
    const size_t at = b->step_begin[step];
    if (segs) *segs = b->segs.data() + at;
    return (int)(b->step_begin[step + 1] - at);
}

const uint8_t *batch_arena(const og_batch *b, size_t *bytes) {
    if (!b) return nullptr;
    if (bytes) *bytes = b->arena.size();
    return b->arena.data();
}

} // namespace

namespace {

// opusgpu_files_plan (ca null) and opusgpu_files_plan_cuts.
int files_plan(int n_files, const uint8_t *const *files, const int64_t *file_lens, int channels, int mode, int flags, int threads,
               opusgpu_file_info *info, const CutArgs *ca, opusgpu_file_batch **out) {
    if (!out) return OPUSGPU_BAD_ARG;
    *out = nullptr;
    if (!files_ok(n_files, files, file_lens) || (channels != 1 && channels != 2) ||
        (mode != OPUSGPU_MODE_REFERENCE && mode != OPUSGPU_MODE_RFC) ||
        (flags & ~(OPUSGPU_PAGES_GROUP_BY_MODE | OPUSGPU_PAGES_ORDER_BY_HEADER)))
        return OPUSGPU_BAD_ARG;
    if (ca && !cuts_ok(n_files, ca->n_cuts, ca->cuts, ca->stride)) return OPUSGPU_BAD_ARG;
    opusgpu_file_batch *b = new (std::nothrow) opusgpu_file_batch;
    if (!b) return OPUSGPU_ALLOC_FAIL;
    b->n_files = ca ? ca->n_cuts : n_files, b->channels = channels, b->mode = mode;
    const int G = (flags & OPUSGPU_PAGES_ORDER_BY_HEADER) ? 9 : (flags & OPUSGPU_PAGES_GROUP_BY_MODE) ? 3 : 1;
    const int rc = build_batch(b, n_files, threads, G, info, ca, [&](int i, opusgpu_file_info &fi, FilePlan &fp) {
        return plan_file(files[i], (size_t)file_lens[i], channels, mode, flags, fi, fp);
    });
    if (rc) {
        delete b;
        return rc;
    }
    *out = b;
    return OPUSGPU_OK;
}

// opusgpu_ms_files_plan (ca null) and opusgpu_ms_files_plan_cuts.
int ms_files_plan(int n_files, const uint8_t *const *files, const int64_t *file_lens, const opusgpu_ms_layout *layout, int mode,
                  int threads, opusgpu_file_info *info, const CutArgs *ca, opusgpu_ms_file_batch **out) {
    if (!out) return OPUSGPU_BAD_ARG;
    *out = nullptr;
    if (!files_ok(n_files, files, file_lens) || !layout || (mode != OPUSGPU_MODE_REFERENCE && mode != OPUSGPU_MODE_RFC))
        return OPUSGPU_BAD_ARG;
    if (ca && !cuts_ok(n_files, ca->n_cuts, ca->cuts, ca->stride)) return OPUSGPU_BAD_ARG;
    // the layout checks are the multistream decoder's own: its framing answers OPUSGPU_BAD_ARG for a layout it would not take
    // (and OPUSGPU_INVALID_PACKET for this packet of no bytes otherwise)
    opusgpu_frame_desc none;
    int32_t count;
    if (opusgpu_ms_packet_to_frames(layout, (const uint8_t *)"", 0, 0, mode, &none, &count) == OPUSGPU_BAD_ARG) return OPUSGPU_BAD_ARG;
    opusgpu_ms_file_batch *b = new (std::nothrow) opusgpu_ms_file_batch;
    if (!b) return OPUSGPU_ALLOC_FAIL;
    b->n_files = ca ? ca->n_cuts : n_files, b->channels = layout->channels, b->mode = mode, b->width = layout->streams;
    b->layout = *layout;
    for (int c = layout->channels; c < 256; c++) b->layout.mapping[c] = 255;
    const int rc = build_batch(b, n_files, threads, 1, info, ca, [&](int i, opusgpu_file_info &fi, FilePlan &fp) {
        return plan_ms_file(files[i], (size_t)file_lens[i], b->layout, mode, fi, fp);
    });
    if (rc) {
        delete b;
        return rc;
    }
    *out = b;
    return OPUSGPU_OK;
}

} // namespace

extern "C" {

int opusgpu_files_plan(int n_files, const uint8_t *const *files, const int64_t *file_lens, int channels, int mode, int flags,
                       int threads, opusgpu_file_info *info, opusgpu_file_batch **out) {
    return files_plan(n_files, files, file_lens, channels, mode, flags, threads, info, nullptr, out);
}
int opusgpu_files_plan_cuts(int n_files, const uint8_t *const *files, const int64_t *file_lens, int n_cuts, const opusgpu_cut *cuts,
                            int64_t track_stride, int channels, int mode, int flags, int threads, opusgpu_file_info *info,
                            opusgpu_cut_info *cut_info, opusgpu_file_batch **out) {
    const CutArgs ca{n_cuts, cuts, track_stride, cut_info, true};
    return files_plan(n_files, files, file_lens, channels, mode, flags, threads, info, &ca, out);
}
int opusgpu_ms_files_plan_cuts(int n_files, const uint8_t *const *files, const int64_t *file_lens, int n_cuts, const opusgpu_cut *cuts,
                               int64_t track_stride, const opusgpu_ms_layout *layout, int mode, int threads, opusgpu_file_info *info,
                               opusgpu_cut_info *cut_info, opusgpu_ms_file_batch **out) {
    const CutArgs ca{n_cuts, cuts, track_stride, cut_info, false};
    return ms_files_plan(n_files, files, file_lens, layout, mode, threads, info, &ca, out);
}
int64_t opusgpu_file_batch_track_stride(const opusgpu_file_batch *b) { return b ? b->track_stride : -1; }
int64_t opusgpu_ms_file_batch_track_stride(const opusgpu_ms_file_batch *b) { return b ? b->track_stride : -1; }

int opusgpu_file_batch_steps(const opusgpu_file_batch *b) { return b ? (int)b->step_begin.size() - 1 : OPUSGPU_BAD_ARG; }
int opusgpu_file_batch_step(const opusgpu_file_batch *b, int step, const opusgpu_frame_desc **descs, const int32_t **slot_files,
                            int *modes) {
    return batch_step(b, step, descs, slot_files, modes);
}
int opusgpu_file_batch_segments(const opusgpu_file_batch *b, int step, const opusgpu_track_seg **segs) {
    return batch_segments(b, step, segs);
}
const uint8_t *opusgpu_file_batch_arena(const opusgpu_file_batch *b, size_t *bytes) { return batch_arena(b, bytes); }
int64_t opusgpu_file_batch_track_samples(const opusgpu_file_batch *b) { return b ? b->track_samples : -1; }
float opusgpu_head_gain_scale(int32_t output_gain_q8) { return (float)(pow(10.0, output_gain_q8 / 5120.0) / 32768.0); }
int64_t opusgpu_file_batch_packet_start(const opusgpu_file_batch *b, int file, int packet_seq) {
    return b ? b->packet_start_of(file, packet_seq) : -1;
}
void opusgpu_file_batch_free(opusgpu_file_batch *b) { delete b; }

// ---- multistream files (include/opusgpu.h, WHOLE FILES / MULTISTREAM) ------------------------------------------------------
int opusgpu_file_layout(const uint8_t *file, int64_t len, opusgpu_ms_layout *layout, opusgpu_file_info *info) {
    if (!layout || len < 0 || (len > 0 && !file)) return OPUSGPU_BAD_ARG;
    opusgpu_file_info fi{};
    int r = OPUSGPU_ALLOC_FAIL;
    try {
        ogc::OpusFile of(file, (size_t)len);
        r = open_file(of, fi);
        if (r >= 0) {
            const ogc::Head &h = of.head();
            r = OPUSGPU_OK;
            layout->channels = h.channel_count, layout->streams = h.stream_count, layout->coupled = h.coupled_count;
            memset(layout->mapping, 255, sizeof layout->mapping);
            memcpy(layout->mapping, h.mapping, (size_t)h.channel_count);
        }
    } catch (const std::bad_alloc &) {
    }
    fi.status = r;
    if (info) *info = fi;
    return r;
}

int opusgpu_ms_files_plan(int n_files, const uint8_t *const *files, const int64_t *file_lens, const opusgpu_ms_layout *layout,
                          int mode, int threads, opusgpu_file_info *info, opusgpu_ms_file_batch **out) {
    return ms_files_plan(n_files, files, file_lens, layout, mode, threads, info, nullptr, out);
}

int opusgpu_ms_file_batch_steps(const opusgpu_ms_file_batch *b) { return b ? (int)b->step_begin.size() - 1 : OPUSGPU_BAD_ARG; }
int opusgpu_ms_file_batch_step(const opusgpu_ms_file_batch *b, int step, const opusgpu_frame_desc **descs, const int32_t **slot_files) {
    return batch_step(b, step, descs, slot_files, nullptr);
}
int opusgpu_ms_file_batch_segments(const opusgpu_ms_file_batch *b, int step, const opusgpu_track_seg **segs) {
    return batch_segments(b, step, segs);
}
const uint8_t *opusgpu_ms_file_batch_arena(const opusgpu_ms_file_batch *b, size_t *bytes) { return batch_arena(b, bytes); }
int64_t opusgpu_ms_file_batch_track_samples(const opusgpu_ms_file_batch *b) { return b ? b->track_samples : -1; }
int64_t opusgpu_ms_file_batch_packet_start(const opusgpu_ms_file_batch *b, int file, int packet_seq) {
    return b ? b->packet_start_of(file, packet_seq) : -1;
}
void opusgpu_ms_file_batch_free(opusgpu_ms_file_batch *b) { delete b; }

} // extern "C"
