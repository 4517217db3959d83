// og_host_path.hpp -- the host-buffer path: opusgpu_decode_packets / opusgpu_decode_packets_fec (include/opusgpu.h), packets in
// host memory in, PCM in host memory out.  Included by og_api.hip behind og_step.hpp, whose steps it queues.
//
// What a packet becomes is og_host_framing.hpp's (CPU-tested: tests/test_host_framing.py); this file is the call around it -- a
// HostCall holds the call's tables, and every stage is one of its functions: the regular probe, plan (framing pass 1), prefix sums
// and staging, place (framing pass 2), per frame index the step table, the cut into pieces and parts, ONE of three launch flows
// (slices / parts as steps of their own / a single step) with copy_pieces behind the kernels, and deliver.
#pragma once
#include <sched.h>
#include <atomic>
#include <chrono>
#include "og_host_framing.hpp"

// OPUSGPU_HOST_TIMING=1: wall time of the phases of opusgpu_decode_packets on stderr (adds a stream synchronise after the
// kernels so that decode and copy-back can be told apart; for tuning only)
struct HostPhaseTimer {
    bool on, light; // on: OPUSGPU_HOST_TIMING=1, the one-batch flow with a wait after the kernels; light (=2): the flow as it is
    std::chrono::steady_clock::time_point t;
    HostPhaseTimer() : on(og_debug().host_timing == 1), light(og_debug().host_timing == 2), t(std::chrono::steady_clock::now()) {}
    void mark(const char *what) {
        if (!on && !light) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[opusgpu_decode_packets] %-34s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

static int grow_pinned(opusgpu_ctx *ctx, void **p, size_t *cap, size_t need) {
    if (*cap >= need) return OPUSGPU_OK;
    if (*p) HIPCHK(ctx, hipHostFree(*p));
    *p = nullptr;
    *cap = 0;
    const size_t want = need + need / 4;
    if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) return OPUSGPU_ALLOC_FAIL;
    *cap = want;
    return OPUSGPU_OK;
}

// CPUs this process may run on (its affinity mask: a container's share, not the machine's), at most `most`.
static int host_cpus(int most) {
    cpu_set_t set;
    int c = 8;
    if (sched_getaffinity(0, sizeof set, &set) == 0) c = CPU_COUNT(&set);
    return c < 1 ? 1 : (c > most ? most : c);
}

// Is [p, p + bytes) page-locked host memory the device can write?  ONE page-locked range must cover all of it: either one the
// caller registered through opusgpu_host_register (the context keeps the list), or one allocation / registration the runtime knows
// (its start and size are asked for: two ends that are each page-locked may have pageable memory between them).
static bool host_range_is_pinned(opusgpu_ctx *ctx, const void *p, size_t bytes) {
    if (!p || !bytes) return false;
    const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
    {
        std::lock_guard<std::mutex> lock(ctx->registered_mutex);
        for (const auto &r : ctx->registered)
            if (lo >= r.first && hi <= r.first + r.second) return true;
    }
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost) {
        (void)hipGetLastError(); // (pageable memory is reported as an error: not one of ours)
        return false;
    }
    void *start = nullptr;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)p) != hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return lo >= (uintptr_t)start && hi <= (uintptr_t)start + size;
}

namespace {
struct HostCall {
    opusgpu_ctx *const ctx; // the call's arguments
    const int n;
    const int32_t *const stream_ids;
    const uint8_t *const *const packets;
    const int32_t *const lens;
    int16_t *const pcm;
    const int frame_capacity;
    int32_t *const result;
    const bool fec, rfc;
    const int CC;
    const size_t frame_pcm, cap_pcm; // one frame's block in the device PCM buffer (20 ms, or room for a 60 ms frame in RFC mode); the caller's block per packet
    HostPhaseTimer timer;
    const int host_threads;
    // framing: one plan per packet; frames in (packet, frame) order from first[i], packet bytes at base[i] of the arena
    std::vector<ogh::PacketPlan> plans;
    std::vector<int32_t> conceal; // decode_fec: 48 flags words per packet (the concealment pieces)
    std::vector<int> first;
    std::vector<size_t> base;
    int max_frames = 0;
    bool regular = false, pipelined = false;
    opusgpu_frame_desc *all = nullptr;
    uint8_t *arena = nullptr;
    // the step of frame index k: m frames, frame j of packet owner[j] (regular: of packet j)
    std::vector<opusgpu_frame_desc> step;
    std::vector<int> owner;
    std::vector<int32_t> placed; // RFC mode: samples of packet i delivered so far (frames may differ in duration)
    int k = 0, m = 0, pieces = 1, parts = 1;
    bool sliced = false, direct = false;
    size_t bound[OPUSGPU_COPY_PIECES + 1]; // frames [bound[t], bound[t + 1]) make piece t; a part is pieces / parts consecutive pieces

    HostCall(opusgpu_ctx *c, int n_, const int32_t *ids, const uint8_t *const *pk, const int32_t *ln, int16_t *out, int cap, int32_t *res, bool fec_)
        : ctx(c), n(n_), stream_ids(ids), packets(pk), lens(ln), pcm(out), frame_capacity(cap), result(res), fec(fec_),
          rfc(c->mode == OPUSGPU_MODE_RFC), CC(c->channels), frame_pcm((size_t)(rfc ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES) * CC),
          cap_pcm((size_t)cap * OPUSGPU_FRAME_SAMPLES * CC), host_threads(n_ >= 4096 ? host_cpus(16) : 1), plans(n_),
          conceal(fec_ ? (size_t)n_ * 48 : 0), first(n_ + 1, 0), base(n_ + 1, 0), placed(rfc ? n_ : 0, 0) {}

    template <class F>
    void on_subranges(int from, int to, F &&f) { // f(lo, hi) over [from, to), on the host threads
        if (host_threads == 1 || to - from < 1024) {
            f(from, to);
            return;
        }
        const int64_t w = to - from;
        ctx->pool.run(host_threads, [&](int t) { f(from + (int)(w * t / host_threads), from + (int)(w * (t + 1) / host_threads)); });
    }
    void remember(int i) { ogh::remember_packet(plans[i], &ctx->last_count[stream_ids[i]], &ctx->last_flags[stream_ids[i]]); }

    // The common large call is REGULAR: every packet holds one frame (frame-count code 0) of a stream that exists, of a size and
    // duration the call has room for.  One look at the TOC bytes settles that, and then nothing of the first framing pass is
    // needed: packet i is frame i of the one step, its bytes lie at the running sum of the lengths, and the (only) framing pass
    // runs part by part next to the device (0.63 + 0.17 ms of host work less in front of the first kernel at 65,536 packets).
    // The probe only DECIDES (it keeps the TOC bytes it saw); the plans, codes and stream memory are written once it has.
    void probe_regular() {
        if (rfc || fec || n < 4096 || ctx->host_parts <= 1 || timer.on) return;
        std::vector<uint8_t> toc(n);
        std::atomic<int> irregular{0};
        on_subranges(0, n, [&](int lo, int hi) {
            for (int i = lo; i < hi; i++) {
                if (!ogh::is_regular_packet(packets[i], lens[i], stream_ids[i], ctx->n_streams, frame_capacity)) {
                    irregular.store(1, std::memory_order_relaxed);
                    return;
                }
                toc[i] = packets[i][0];
            }
        });
        if (irregular.load()) return;
        regular = true;
        on_subranges(0, n, [&](int lo, int hi) {
            for (int i = lo; i < hi; i++) {
                result[i] = 0;
                plans[i] = ogh::decoded_plan(1, ogh::toc_flags(toc[i]));
                remember(i); // (what an empty packet of this stream will be decoded as)
            }
        });
    }
    // framing pass 1.  (A stream appears at most once per call: no two threads touch the same entry of the stream memory.)
    void plan() {
        on_subranges(0, n, [&](int lo, int hi) {
            for (int i = lo; i < hi; i++) {
                const int sid = stream_ids[i];
                const bool known = sid >= 0 && sid < ctx->n_streams;
                plans[i] = ogh::plan_packet(packets[i], lens[i], sid, ctx->n_streams, ctx->mode, fec, CC, frame_capacity, known ? ctx->last_count[sid] : 0,
                                            known ? ctx->last_flags[sid] : 0, fec ? &conceal[(size_t)i * 48] : nullptr);
                result[i] = plans[i].code;
                if (known) remember(i);
            }
        });
    }
    void prefix_sums() { // where every packet's frames and bytes go
        for (int i = 0; i < n; i++) {
            first[i + 1] = first[i] + plans[i].frames;
            base[i + 1] = base[i] + (plans[i].in_arena ? (size_t)lens[i] : 0);
            if (plans[i].frames > max_frames) max_frames = plans[i].frames;
        }
        timer.mark("prefix sums");
    }
    int stage() { // the page-locked tables the frames and bytes go into
        if (base[n] > 0x7fffffffu) return OPUSGPU_BAD_ARG; // descriptor offsets are 32-bit: split the call
        if (int rc = grow_pinned(ctx, &ctx->h_descs, &ctx->cap_h_descs, sizeof(opusgpu_frame_desc) * (size_t)first[n])) return rc;
        if (int rc = grow_pinned(ctx, &ctx->h_arena, &ctx->cap_h_arena, base[n] + 1)) return rc;
        all = (opusgpu_frame_desc *)ctx->h_descs; // frames in (packet, frame) order
        arena = (uint8_t *)ctx->h_arena;
        timer.mark("staging");
        return OPUSGPU_OK;
    }
    void place(int from, int to) { // framing pass 2: descriptors and packet bytes of packets [from, to) to their places
        on_subranges(from, to, [&](int lo, int hi) {
            for (int i = lo; i < hi; i++) {
                if (plans[i].in_arena) memcpy(arena + base[i], packets[i], (size_t)lens[i]);
                (void)ogh::plan_descs(plans[i], packets[i], lens[i], stream_ids[i], ctx->mode, (int32_t)base[i],
                                      fec ? &conceal[(size_t)i * 48] : nullptr, all + first[i]);
            }
        });
    }

    void step_table() { // frame k of every packet that has one and has not failed
        step.clear();
        owner.clear();
        if (regular) // (frame j belongs to packet j)
            ;
        else if (pipelined) {
            owner.reserve(first[n]);
            for (int i = 0; i < n; i++)
                if (plans[i].frames) owner.push_back(i);
        } else
            for (int i = 0; i < n; i++)
                if (plans[i].frames > k && result[i] >= 0) {
                    step.push_back(all[first[i] + k]);
                    owner.push_back(i);
                }
        m = regular ? n : (int)owner.size();
    }
    int grow_step() { // the step's device tables and landing zones; the table itself goes up unless the flows send it in parts
        int rc;
        if ((rc = grow(ctx, &ctx->d_descs, &ctx->cap_descs, sizeof(opusgpu_frame_desc) * m))) return rc;
        if ((rc = grow(ctx, &ctx->d_pcm, &ctx->cap_pcm, frame_pcm * 2 * m))) return rc;
        if ((rc = grow(ctx, &ctx->d_result, &ctx->cap_result, sizeof(int32_t) * m))) return rc;
        if (!pipelined) HIPCHK(ctx, hipMemcpyAsync(ctx->d_descs, step.data(), sizeof(opusgpu_frame_desc) * m, hipMemcpyHostToDevice, ctx->stream));
        if ((rc = grow_pinned(ctx, &ctx->h_pcm, &ctx->cap_h_pcm, frame_pcm * 2 * m))) return rc;
        return grow_pinned(ctx, &ctx->h_res, &ctx->cap_h_res, sizeof(int32_t) * m);
    }
    // the modes a range of this step's frames contains (the kernels of the others are not launched).  The range indexes the
    // table that is uploaded: `all` itself in the pipelined flow (single-frame packets in packet order ARE the step table),
    // `step` otherwise -- step[j] = all[first[owner[j]] + k], a different set of frames than all[lo .. hi) as soon as one packet
    // of the call has more than one frame.
    int modes_of(size_t lo, size_t hi) const {
        const opusgpu_frame_desc *table = pipelined ? all : step.data();
        int mask = 0;
        for (size_t f = lo; f < hi && mask != 7; f++) mask |= 1 << (table[f].flags & 3);
        return mask & 7;
    }
    // The PCM comes back in pieces, each followed by an event: every packet owns its own block of the caller's buffer, and the
    // threads that fill the blocks start on a piece as soon as it has landed, while the later pieces are still on their way.  A
    // large batch goes in parts: a part's pieces travel (on the copy stream) while the next part's kernels run.  More parts start
    // the copy earlier but pay the parse kernels' fixed latency once per part: two is the measured optimum at 65,536 frames
    // (9.5 ms; one 11.8, four 10.7, eight 13.2).
    int cut_pieces() {
        pieces = m >= 4096 ? OPUSGPU_COPY_PIECES : 1;
        // (slices cost one more launch of the arithmetic kernels each; parts that are steps of their own pay the entropy kernels'
        // latency each: two of those at most)
        sliced = pipelined && og_debug().host_slices;
        parts = !(pieces > 1 && !timer.on) ? 1 : (sliced ? ctx->host_parts : OG_MIN(ctx->host_parts, 2));
        for (int t = 0; t < pieces; t++)
            if (!ctx->ev_piece[t]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_piece[t], hipEventDisableTiming));
        // Pipelined: a part is a range of PACKETS (its frames: first[] of the range's ends), cut evenly into its pieces.
        for (int h = 0; h < parts; h++) {
            const int t0 = h * pieces / parts, t1 = (h + 1) * pieces / parts;
            const size_t flo = pipelined ? (size_t)first[(int64_t)n * h / parts] : (size_t)((int64_t)m * t0 / pieces);
            const size_t fhi = pipelined ? (size_t)first[(int64_t)n * (h + 1) / parts] : (size_t)((int64_t)m * t1 / pieces);
            for (int t = t0; t <= t1; t++) bound[t] = flo + (size_t)((int64_t)(fhi - flo) * (t - t0) / (t1 - t0));
        }
        // DIRECT: the caller's PCM buffer is page-locked (opusgpu_host_register, hipHostMalloc, hipHostRegister) and the step table is
        // the packets in order, one 20 ms block each: the pieces travel straight into it -- no landing zone, no host copy behind it.
        direct = pipelined && m == n && frame_capacity == 1 && !rfc && host_range_is_pinned(ctx, pcm, (size_t)n * cap_pcm * 2);
        if (parts > 1) {
            hipStream_t made;
            if (int rc = copy_stream_of(ctx, &made)) return rc; // (opusgpu_upload_async makes it too, from another thread)
            for (int h = 0; h < parts; h++)
                if (!ctx->ev_part[h]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_part[h], hipEventDisableTiming));
        }
        return OPUSGPU_OK;
    }
    int copy_pieces(hipStream_t cs, int t0, int t1) { // results of the pieces' frames first, then the pieces
        const size_t flo = bound[t0], fhi = bound[t1];
        HIPCHK(ctx, hipMemcpyAsync((int32_t *)ctx->h_res + flo, (const int32_t *)ctx->d_result + flo, sizeof(int32_t) * (fhi - flo),
                                   hipMemcpyDeviceToHost, cs));
        for (int t = t0; t < t1; t++) {
            const size_t lo = bound[t], hi = bound[t + 1];
            HIPCHK(ctx, hipMemcpyAsync((direct ? (uint8_t *)pcm : (uint8_t *)ctx->h_pcm) + lo * frame_pcm * 2,
                                       (const uint8_t *)ctx->d_pcm + lo * frame_pcm * 2, (hi - lo) * frame_pcm * 2, hipMemcpyDeviceToHost, cs));
            HIPCHK(ctx, hipEventRecord(ctx->ev_piece[t], cs));
        }
        return OPUSGPU_OK;
    }
    int part_done(int h) { // the copy stream takes part h's pieces once the kernels queued so far are through
        HIPCHK(ctx, hipEventRecord(ctx->ev_part[h], ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_part[h], 0));
        return copy_pieces(ctx->copy_stream, h * pieces / parts, (h + 1) * pieces / parts);
    }

    // SLICES: everything placed and uploaded at once (0.2 ms of host work at 65,536 packets), the entropy kernels once over
    // the whole table, the arithmetic kernels slice by slice with the slice's PCM leaving behind them
    int flow_slices() {
        place(0, n);
        timer.mark("  all packets placed");
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_arena, arena, base[n], hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_descs, all, sizeof(opusgpu_frame_desc) * m, hipMemcpyHostToDevice, ctx->stream));
        size_t cut[OPUSGPU_COPY_PIECES + 1];
        for (int h = 0; h <= parts; h++) cut[h] = bound[h * pieces / parts];
        StepSlices sl;
        sl.count = parts;
        sl.bounds = cut;
        sl.after_slice = [&](int h) -> int { return part_done(h); };
        if (int rc = decode_step_impl(ctx, m, ctx->d_descs, ctx->d_arena, ctx->d_pcm, ctx->d_result, nullptr, false, modes_of(0, m), 0, &sl)) return rc;
        timer.mark("  uploaded, launched, copies queued");
        return OPUSGPU_OK;
    }
    // (A/B flow, OPUSGPU_HOST_SLICES=0: every part its own in-order step -- the entropy kernels' latency is paid per part.
    //  Measured also: the parts' chains alternating between two streams, 6.8 - 7.0 ms per 65,536 packets like the slices.)
    int flow_parts() {
        for (int h = 0; h < parts; h++) {
            const size_t flo = bound[h * pieces / parts], fhi = bound[(h + 1) * pieces / parts];
            if (pipelined) { // this part's packets: place, upload
                const int plo = (int)((int64_t)n * h / parts), phi = (int)((int64_t)n * (h + 1) / parts);
                place(plo, phi);
                timer.mark("  part placed");
                if (base[phi] > base[plo])
                    HIPCHK(ctx, hipMemcpyAsync((uint8_t *)ctx->d_arena + base[plo], arena + base[plo], base[phi] - base[plo],
                                               hipMemcpyHostToDevice, ctx->stream));
                if (fhi > flo)
                    HIPCHK(ctx, hipMemcpyAsync((opusgpu_frame_desc *)ctx->d_descs + flo, all + flo, sizeof(opusgpu_frame_desc) * (fhi - flo),
                                               hipMemcpyHostToDevice, ctx->stream));
            }
            if (int rc = decode_step_impl(ctx, (int)(fhi - flo), (const opusgpu_frame_desc *)ctx->d_descs + flo, ctx->d_arena,
                                          (uint8_t *)ctx->d_pcm + flo * frame_pcm * 2, (int32_t *)ctx->d_result + flo, nullptr, false, modes_of(flo, fhi)))
                return rc; // (an empty part launches nothing; its pieces' events are still recorded below)
            if (int rc = part_done(h)) return rc;
            timer.mark("  part uploaded, launched, copies queued");
        }
        timer.mark("table upload + kernels + copy-back in parts (enqueue)");
        return OPUSGPU_OK;
    }
    int flow_single() { // one step, its pieces behind it on the same stream
        if (int rc = decode_step_impl(ctx, m, ctx->d_descs, ctx->d_arena, ctx->d_pcm, ctx->d_result, nullptr, false, modes_of(0, m))) return rc;
        timer.mark("table upload + kernels (enqueue)");
        if (timer.on) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            timer.mark("kernels (wait)");
        }
        return copy_pieces(ctx->stream, 0, pieces);
    }

    // thread t of `threads` takes its share of every piece: the work left when the last piece lands is 1 / pieces of the PCM,
    // spread over all threads
    hipError_t deliver(int t, int threads) {
        const int16_t *h_pcm = (const int16_t *)ctx->h_pcm;
        const int32_t *h_res = (const int32_t *)ctx->h_res;
        for (int p = 0; p < pieces; p++) {
            if (hipError_t e = hipEventSynchronize(ctx->ev_piece[p])) return e;
            const int64_t plo = (int64_t)bound[p], phi = (int64_t)bound[p + 1];
            const int lo = (int)(plo + (phi - plo) * t / threads), hi = (int)(plo + (phi - plo) * (t + 1) / threads);
            for (int j = lo; j < hi; j++) {
                const int i = regular ? j : owner[j];
                if (h_res[j] < 0) {
                    result[i] = h_res[j];
                    if (direct) memset(pcm + (size_t)i * cap_pcm, 0, frame_pcm * 2); // (whatever the device buffer held: not the caller's)
                    continue;
                }
                if (direct) { // the PCM is in place already
                    result[i] += h_res[j];
                    continue;
                }
                if (rfc) { // a packet appears once per step: nobody else touches placed[i]
                    memcpy(pcm + (size_t)i * cap_pcm + (size_t)placed[i] * CC, &h_pcm[(size_t)j * frame_pcm], (size_t)h_res[j] * CC * 2);
                    placed[i] += h_res[j];
                } else
                    memcpy(pcm + (size_t)i * cap_pcm + (size_t)k * frame_pcm, &h_pcm[(size_t)j * frame_pcm], frame_pcm * 2);
                result[i] += h_res[j];
            }
        }
        return hipSuccess;
    }

    int run_step() { // the m frames of index k: kernels, then results and PCM back to the host
        timer.mark("step table");
        if (int rc = grow_step()) return rc;
        if (int rc = cut_pieces()) return rc;
        if (int rc = parts > 1 ? (sliced ? flow_slices() : flow_parts()) : flow_single()) return rc;
        timer.mark("copy-back (enqueue)");
        const int threads = pieces == 1 ? 1 : OPUSGPU_COPY_THREADS;
        hipError_t thread_err[OPUSGPU_COPY_THREADS];
        ctx->pool.run(threads, [&](int t) { thread_err[t] = deliver(t, threads); });
        for (int t = 0; t < threads; t++)
            if (thread_err[t] != hipSuccess) return fail(ctx, OPUSGPU_ERR_HIP, "hipEventSynchronize (PCM piece)", thread_err[t]);
        timer.mark("copy-back + delivery (wait)");
        return OPUSGPU_OK;
    }
};
} // namespace

// 1. frame the packets on the host (opus_decode_native, src/opus_decoder.cpp:280-348).  Large batches by ranges of packets on a
//    few threads, in two passes: frame counts and sizes, then (after the prefix sums that place every packet) descriptors and
//    packet bytes.  2. upload; 3. one step per frame index (frames of one packet are sequential).
static int decode_packets_impl(opusgpu_ctx *ctx, int n, const int32_t *stream_ids, const uint8_t *const *packets,
                               const int32_t *lens, int16_t *pcm, int frame_capacity, int32_t *result, const bool fec) {
    if (!ctx || n < 0 || !ctx->d_streams) return OPUSGPU_BAD_ARG;
    if (n == 0) return OPUSGPU_OK;
    if (!stream_ids || !packets || !lens || !pcm || !result || frame_capacity <= 0) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->pipeline) // (pipelined device-resident steps may still be in flight on the library's streams, which the parts below use)
        if (int rc = sync_in_flight(ctx)) return rc;
    if (fec && ctx->mode != OPUSGPU_MODE_RFC) return OPUSGPU_BAD_ARG;
    HostCall c(ctx, n, stream_ids, packets, lens, pcm, frame_capacity, result, fec);
    c.probe_regular();
    if (!c.regular) c.plan();
    c.timer.mark("framing pass 1 (counts)");
    c.prefix_sums();
    if (c.first[n] == 0) return OPUSGPU_OK;
    if (int rc = c.stage()) return rc;
    // The common large call -- one frame per packet -- is pipelined: the frames in packet order ARE the step table, so the call
    // goes in parts of packets, each placed (pass 2), uploaded and launched while the device works on the part before it and that
    // part's PCM travels back.  Anything else: everything placed and uploaded first, then one step per frame index.
    c.pipelined = c.max_frames == 1 && c.first[n] >= 4096 && ctx->host_parts > 1 && !c.timer.on;
    if (int rc = grow(ctx, &ctx->d_arena, &ctx->cap_arena, c.base[n] + 16)) return rc;
    if (!c.pipelined) {
        c.place(0, n);
        c.timer.mark("prefix + framing pass 2 (place)");
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_arena, c.arena, c.base[n], hipMemcpyHostToDevice, ctx->stream));
        c.timer.mark("arena upload (enqueue)");
    }
    for (c.k = 0; c.k < c.max_frames; c.k++) {
        c.step_table();
        if (c.m == 0) break;
        if (int rc = c.run_step()) return rc;
    }
    return OPUSGPU_OK;
}

extern "C" {
int opusgpu_decode_packets(opusgpu_ctx *ctx, int n, const int32_t *stream_ids, const uint8_t *const *packets,
                           const int32_t *lens, int16_t *pcm, int frame_capacity, int32_t *result) {
    return decode_packets_impl(ctx, n, stream_ids, packets, lens, pcm, frame_capacity, result, false);
}
int opusgpu_decode_packets_fec(opusgpu_ctx *ctx, int n, const int32_t *stream_ids, const uint8_t *const *packets,
                               const int32_t *lens, int16_t *pcm, int frame_capacity, int32_t *result) {
    return decode_packets_impl(ctx, n, stream_ids, packets, lens, pcm, frame_capacity, result, true);
}
} // extern "C"
