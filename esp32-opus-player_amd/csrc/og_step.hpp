// og_step.hpp -- the decode-step scheduler: which kernel of which step runs on which stream behind which event, and nothing else.
//
// Host code only.  Included by og_api.hip, which defines the launch wrappers declared below next to the kernels they start, and by
// the CPU ordering test (tests/emul/og_step_test.cpp), which defines them -- and the handful of HIP runtime entry points used here
// -- as a recording double: this file includes no kernel header and compiles with a plain host compiler.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <thread>

#define OG_SILK_SETS 3 // sets of SILK records and hand-offs that pipelined SILK / hybrid steps rotate through
static_assert(OG_SILK_SETS >= 2, "a pipelined SILK / hybrid step runs next to the step before it");

// The library's streams, the events between them and what the host remembers of the steps it has queued.
struct StepPipeline {
    // opusgpu_set_pipeline: the parse of step k + 1's CELT-only frames runs on parse_stream, next to step k's reconstruction
    // and its reconstruction on recon_stream; parse records and the reconstruction's per-frame output (d_recs, d_rout) rotate
    int slot = 0, front_recorded = 0, post_recorded[3] = {};
    hipStream_t parse_stream = nullptr, recon_stream = nullptr, last_step_stream = nullptr;
    hipStream_t side_stream = nullptr;                // in-order steps with SILK frames: the second half's chain (step_in_order)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_front = nullptr;  // step k: its front kernels have finished (on the step's stream)
    hipEvent_t ev_parsed = nullptr; // step k: its early parse has finished (on parse_stream)
    hipEvent_t ev_recon = nullptr;  // step k: its reconstruction has finished (on recon_stream)
    hipEvent_t ev_post[3] = {};     // by slot: k_celt_post of the last step that used it has finished (on the step's stream)
    // Pipelined SILK-only steps (a step the caller declares SILK-only): the parse kernel keeps what its next run needs of the past
    // in d_shadow (SilkShadow per stream, og_silk_parse.hpp) and runs for step k + 1 on parse_stream next to step k's synthesis.
    unsigned shadow_epoch = 1; // advanced by everything else that may change a stream's SILK state: stale copies are ignored
    int silk_slot = 0, sdone_recorded[OG_SILK_SETS] = {}, last_silk_mask = 0, last_kind = 0; // last_kind: 0 in order, 1 pipelined CELT-only, 2 pipelined SILK-only
    bool last_kind2_celt = false; // the last step of kind 2 held CELT-only frames too (enter_step_kind)
    hipEvent_t ev_sparsed = nullptr, ev_sdone[OG_SILK_SETS] = {}, ev_sp = nullptr, ev_spar = nullptr, ev_hrecon = nullptr; // ev_sp: a step's SILK parse is done; ev_spar: its parameter half; ev_hrecon: its CELT reconstruction
    // Steps queued as a window (opusgpu_decode_steps_device): the kernels of neighbouring steps are placed in the order that
    // works -- the next step's parse, then this step's reconstruction, then the de-emphasis of the step before -- by stream
    // memory waits on two counters the parse / reconstruction workgroups bump when they start (device words, 64 bytes apart;
    // the host keeps the totals they will reach).  Round 2 got that order from a spin-wait kernel watching the wall clock.
    uint32_t *d_started = nullptr; // [0] early-parse workgroups started, [16] every 64th reconstruction workgroup started
    uint32_t parse_started_total = 0, recon_started_total = 0;
    uint32_t window_parse_target = 0, window_recon_target = 0; // the counts the last queued step of an unfinished window waits for (0: none)

    // The device is drained: whatever was recorded has completed, nothing later waits for it.
    void drained() {
        front_recorded = post_recorded[0] = post_recorded[1] = post_recorded[2] = 0;
        for (int i = 0; i < OG_SILK_SETS; i++) sdone_recorded[i] = 0;
        last_silk_mask = 0;
    }
};

#include "og_ctx.hpp" // opusgpu_ctx (which holds a StepPipeline), fail, HIPCHK, grow

// One decode step, built once per call (decode_step_impl).
struct Step {
    hipStream_t s; // the step's stream: the caller's, or the context's
    int n;
    const void *descs, *arena;
    void *pcm, *result;
    int pcm_stride, modes; // modes: bit 0 SILK-only, 1 hybrid, 2 CELT-only frames may be present
    bool keeps_kind, any_silk, any_celt;
    int sset;                             // the set of SILK records and hand-offs this step uses (and of CELT records with them)
    void *recs, *rout, *handoff, *srecs; // of the chosen set; handoff, srecs: null when the step has no SILK records
};

// The kernels the scheduler starts, defined in og_api.hip next to them: frames [f0, f0 + cnt) of the step on stream q.
void launch_stream_stall(opusgpu_ctx *ctx, hipStream_t q);
void launch_decode_rfc(opusgpu_ctx *ctx, hipStream_t q, const Step &st);
// pass 0: every frame of the step, a wave each; 1: every frame that is not CELT-only; 2: the frames k_silk_synth parked (Q4)
void launch_decode_step(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, int pass);
void launch_silk_parse(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch);   // 32 frames per wave
void launch_silk_parse64(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch); // 64
void launch_silk_params(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch);
// early: the parse of a pipelined CELT-only step (CELT-only frames, parse_groups groups per workgroup, counts itself in at d_started);
// wide: 64 frames per wave (og_parse64.hip)
void launch_celt_parse(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool wide, bool early);
int celt_parse_early_grid(const opusgpu_ctx *ctx, int cnt, bool wide); // workgroups of such a parse over cnt frames
void launch_celt_recon_fb(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool counts_in); // counts_in: at d_started + 16
extern "C" int og_celt_recon_fb_signals(int n); // how often a launch over n frames bumps `started`
void launch_celt_recon(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt);
void launch_celt_post(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool others);
void launch_silk_synth(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, int nb_done);
void launch_silk_synth_nb(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt);
// bytes per frame of a step's records (the types live with the kernels)
extern const size_t og_parse_rec_bytes, og_recon_out_bytes, og_silk_handoff_bytes, og_silk_rec_bytes;

// Whatever pipelined steps still have in flight -- the last step's reconstruction on recon_stream, an early parse, the step's
// own stream when the caller supplied one -- works on state, records and ReconOut: a read-back waits for all of it, not only
// for the context's stream.
static int sync_in_flight(opusgpu_ctx *ctx) {
    if (ctx->sp.parse_stream) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->sp.parse_stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->sp.recon_stream));
    }
    if (ctx->sp.last_step_stream && ctx->sp.last_step_stream != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->sp.last_step_stream));
    return OPUSGPU_OK;
}
// opusgpu_set_pipeline(on), first time: the streams pipelined steps run ahead on, their events and the start counters.
static int pipeline_create(opusgpu_ctx *ctx) {
    StepPipeline &sp = ctx->sp;
    if (sp.parse_stream) return OPUSGPU_OK;
    // the early parse is a single round of long-running workgroups: it is placed first (highest priority), the
    // reconstruction it runs next to fills the slots around it
    int least = 0, greatest = 0;
    HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    if (!og_debug().parse_priority) greatest = least;
    HIPCHK(ctx, hipStreamCreateWithPriority(&sp.parse_stream, hipStreamNonBlocking, greatest));
    HIPCHK(ctx, hipStreamCreateWithFlags(&sp.recon_stream, hipStreamNonBlocking));
    HIPCHK(ctx, hipEventCreateWithFlags(&sp.ev_front, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&sp.ev_parsed, hipEventDisableTiming));
    HIPCHK(ctx, hipEventCreateWithFlags(&sp.ev_recon, hipEventDisableTiming));
    for (int i = 0; i < 3; i++) HIPCHK(ctx, hipEventCreateWithFlags(&sp.ev_post[i], hipEventDisableTiming));
    HIPCHK(ctx, hipMalloc((void **)&sp.d_started, 128));
    HIPCHK(ctx, hipMemset(sp.d_started, 0, 128));
    return OPUSGPU_OK;
}
// (opusgpu_ctx_destroy: whatever was created, here or on first use by a step)
static void pipeline_destroy(opusgpu_ctx *ctx) {
    StepPipeline &sp = ctx->sp;
    for (hipStream_t q : {sp.parse_stream, sp.recon_stream, sp.side_stream})
        if (q) (void)hipStreamSynchronize(q);
    for (hipEvent_t e : {sp.ev_front, sp.ev_parsed, sp.ev_recon, sp.ev_post[0], sp.ev_post[1], sp.ev_post[2], sp.ev_sparsed, sp.ev_sp, sp.ev_spar,
                         sp.ev_hrecon, sp.ev_fork, sp.ev_join})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : sp.ev_sdone)
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(sp.d_started);
    for (hipStream_t q : {sp.parse_stream, sp.recon_stream, sp.side_stream})
        if (q) (void)hipStreamDestroy(q);
    sp = StepPipeline();
}
// `tables_resident`: the step's descriptors and payload bytes are complete in device memory now (the public entry's contract
// when pipelining is on); false when this call's own uploads are still queued on the step's stream (opusgpu_decode_packets):
// such a step does not run ahead of anything.
// OPUSGPU_LAUNCH_DELAY_US (og_debug.hpp): the host dawdles before the launches of a decode step -- what a loaded host, a slow
// event hop or another thread's launches would do -- so that tools/launch_jitter.py can show the step time does not depend on it
#define OG_SILK_PARSE_WIDE_MIN 98304 // frames of an in-order launch from which the SILK parse runs with 64 frames per wave
#define OG_HALVES_MIN 4096 // frames per half below which an in-order step is not cut in two
static void launch_jitter() {
    if (const int us = og_debug().launch_delay_us) std::this_thread::sleep_for(std::chrono::microseconds(us));
}
// `next_n` (steps queued as a window, opusgpu_decode_steps_device): the number of frames of the step that the same call queues
// right behind this one with the same mode mask, 0 when there is none or it is not known.
// `slices` (opusgpu_decode_packets: PCM that leaves in pieces): the step's entropy kernels run once over all n frames -- they wait
// on latency, a fraction of the frames takes them as long as all -- and the arithmetic kernels slice by slice, frames
// [bounds[i], bounds[i + 1]); after_slice(i) is called behind slice i's last launch (to queue that slice's copies).
// A step is of one of three kinds: in order (0), pipelined CELT-only (1), pipelined SILK-only (2).  Going into or out of a run of
// pipelined SILK-only steps happens from an idle device (their parse reads the stream state when it has no current copy of its
// own, and whatever follows them reads what their last kernels write); every step of another kind ends the epoch of the parse
// kernel's copies (it may write SILK state, or prev_mode, behind that kernel's back).
// keeps_kind (OPUSGPU_STEP_KEEPS_MODE): the caller's word that no stream of this step has decoded a frame of another mode (SILK-only,
// hybrid, CELT-only) since its last reset.  Such a step shares no stream with anything of the other kind that is still in flight,
// so going from one pipelined kind to the other needs no drain, and a CELT-only step leaves the SILK parse kernel's copies (of
// other streams) as current as they were.
// ... as long as the two kinds really are about different streams: a kind-2 step that carries CELT-only frames along (any mix under
// OPUSGPU_STEP_KEEPS_MODE, `celt_frames`) reconstructs them on ITS stream, ordered only against other kind-2 steps, while a kind-1
// step's reconstruction runs on recon_stream and waits only for kind-1 steps.  Next to each other the two would work on the same
// CELT-only streams' state with nothing in between: that change of kind drains like an undeclared one.
static int enter_step_kind(opusgpu_ctx *ctx, int kind, hipStream_t s, bool keeps_kind = false, bool celt_frames = false) {
    const bool shares_celt = (kind == 1 && ctx->sp.last_kind == 2 && ctx->sp.last_kind2_celt) || (kind == 2 && celt_frames && ctx->sp.last_kind == 1);
    const bool disjoint = keeps_kind && kind != 0 && ctx->sp.last_kind != 0 && !shares_celt;
    if ((kind == 2) != (ctx->sp.last_kind == 2) && !disjoint) {
        if (int rc = sync_in_flight(ctx)) return rc;
        HIPCHK(ctx, hipStreamSynchronize(s));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->sp.drained();
    }
    if (kind != 2 && !(keeps_kind && kind == 1)) ctx->sp.shadow_epoch++;
    ctx->sp.last_kind = kind;
    if (kind == 2) ctx->sp.last_kind2_celt = celt_frames;
    return OPUSGPU_OK;
}

// Records and reconstruction output of slot `par` for a step of `need` frames.
static int grow_step_slot(opusgpu_ctx *ctx, int par, size_t need) {
    int rc;
    if (ctx->cap_recs[par] < og_parse_rec_bytes * need && (rc = grow(ctx, &ctx->d_recs[par], &ctx->cap_recs[par], og_parse_rec_bytes * need)))
        return rc;
    if (ctx->cap_rout[par] < og_recon_out_bytes * need && (rc = grow(ctx, &ctx->d_rout[par], &ctx->cap_rout[par], og_recon_out_bytes * need)))
        return rc;
    return OPUSGPU_OK;
}

// SILK records and hand-offs of set `sset` for a step of `need` frames.  `drain` (a pipelined step's stream): growing frees, not
// under kernels of the other sets that are still in flight.
static int grow_silk_set(opusgpu_ctx *ctx, int sset, size_t need, hipStream_t drain) {
    int rc;
    if (ctx->cap_handoff[sset] >= og_silk_handoff_bytes * need && ctx->cap_srecs[sset] >= og_silk_rec_bytes * need) return OPUSGPU_OK;
    if (drain) {
        if ((rc = sync_in_flight(ctx))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(drain));
    }
    if (ctx->cap_handoff[sset] < og_silk_handoff_bytes * need &&
        (rc = grow(ctx, &ctx->d_handoff[sset], &ctx->cap_handoff[sset], og_silk_handoff_bytes * need)))
        return rc;
    if (ctx->cap_srecs[sset] < og_silk_rec_bytes * need && (rc = grow(ctx, &ctx->d_srecs[sset], &ctx->cap_srecs[sset], og_silk_rec_bytes * need)))
        return rc;
    return OPUSGPU_OK;
}

// A window that ends early (a HIP error between two of its steps): the placement waits of the last step queued -- for workgroups
// of a step that will not come -- are let go by writing the counts they wait for; the waits are placement only (events carry the
// data dependencies), so whatever is queued completes.  Then the device drains and the counters restart from zero.
static void release_window_waits(opusgpu_ctx *ctx) {
    if (!ctx->sp.d_started || (!ctx->sp.window_parse_target && !ctx->sp.window_recon_target)) return;
    hipStream_t q = nullptr;
    if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) == hipSuccess) {
        if (ctx->sp.window_parse_target) (void)hipStreamWriteValue32(q, ctx->sp.d_started, ctx->sp.window_parse_target, 0);
        if (ctx->sp.window_recon_target) (void)hipStreamWriteValue32(q, ctx->sp.d_started + 16, ctx->sp.window_recon_target, 0);
        (void)hipStreamSynchronize(q);
        (void)hipStreamDestroy(q);
    }
    (void)sync_in_flight(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipMemset(ctx->sp.d_started, 0, 128);
    ctx->sp.parse_started_total = ctx->sp.recon_started_total = 0;
    ctx->sp.window_parse_target = ctx->sp.window_recon_target = 0;
    (void)hipGetLastError();
}

struct StepSlices {
    int count = 0;
    const size_t *bounds = nullptr;
    std::function<int(int)> after_slice;
};
// OPUSGPU_STALL_STREAM (og_debug.hpp): in front of every kernel of the step on the named stream, a wave that holds that stream --
// it falls behind the others by whole steps, and only the events between the streams keep the kernels in order
static void stall(opusgpu_ctx *ctx, const Step &st, hipStream_t q) {
    if (!ctx->stall_ticks) return;
    const int w = og_debug().stall_stream;
    hipStream_t const t = w == 1 ? st.s : w == 2 ? ctx->sp.parse_stream : w == 3 ? ctx->sp.recon_stream : ctx->sp.side_stream;
    if (t && q == t) launch_stream_stall(ctx, q);
}
// The in-order chain of frames [f0, f0 + cnt) of the step, in two halves: the ENTROPY kernels (one frame per lane) ...
// `pq` (pipelined SILK / hybrid steps): the stream the parameter half runs on -- behind this step's SILK parse and the parameter
// half of the step before, but off the entropy chain: the parse of the next step does not wait for it (SilkShadow's two sides)
static void front(opusgpu_ctx *ctx, const Step &st, hipStream_t q, size_t f0, int cnt, void *shadow = nullptr, uint32_t epoch = 0,
                  hipStream_t pq = nullptr) {
    if (st.srecs) {
        stall(ctx, st, q);
        // (64 frames per wave where the kernel's issue slots are what counts: pipelined steps, large batches; 32 for a small
        // in-order step, whose time is the latency of one wave's serial chain -- same-box: SILK-NB in order 1.36 / 1.41 ms)
        if (shadow || cnt >= OG_SILK_PARSE_WIDE_MIN || og_debug().parse_wide == 2)
            launch_silk_parse64(ctx, q, st, f0, cnt, shadow, epoch);
        else
            launch_silk_parse(ctx, q, st, f0, cnt, shadow, epoch);
        if (pq && pq != q) {
            (void)hipEventRecord(ctx->sp.ev_sp, q);
            (void)hipStreamWaitEvent(pq, ctx->sp.ev_sp, 0);
        }
        stall(ctx, st, pq ? pq : q);
        launch_silk_params(ctx, pq ? pq : q, st, f0, cnt, shadow, epoch);
        if (pq && pq != q) (void)hipEventRecord(ctx->sp.ev_spar, pq);
    }
    if (st.any_celt) stall(ctx, st, q);
    if (st.any_celt && ((shadow && og_debug().parse_wide) || og_debug().parse_wide == 2)) { // (a pipelined step: the wide parse, like pipelined CELT-only steps)
        launch_celt_parse(ctx, q, st, f0, cnt, true, false);
    } else if (st.any_celt)
        launch_celt_parse(ctx, q, st, f0, cnt, false, false);
}
// ... and the ARITHMETIC ones (one frame per wave), which also write the PCM and the result codes
// `rq` (pipelined SILK / hybrid steps): the stream the CELT reconstruction runs on, NEXT TO the SILK synthesis instead of behind
// it -- a hybrid frame's two halves share nothing until the de-emphasis adds them (the synthesis takes prev_mode from the record,
// SilkRec::prev_mode), and the reconstruction of step k touches nothing the de-emphasis of step k - 1 still reads (it appends to
// the history ring; k_celt_post reads at the position the reconstruction recorded, as in pipelined CELT-only steps).  The ring
// holds two frames (2 x 960 of 2,048 samples): the reconstruction of step k waits for the last kernel of step k - 2, whose
// de-emphasis reads where it writes -- nothing else orders the two (the parse of step k waits only for step k - OG_SILK_SETS)
static void back_half(opusgpu_ctx *ctx, const Step &st, hipStream_t q, size_t f0, int cnt, hipStream_t rq = nullptr) {
    const int modes = st.modes;
    bool others = false; // (the kernels that report stream-index errors for every mode)
    if (st.srecs) { // SILK-only frames and the SILK half of hybrid frames
        // (a step that may hold SILK-only frames: the narrowband ones in the kernel whose LDS is sized for them, og_silk_nb.hip)
        const int nb = (modes & 1) && og_debug().silk_nb_kernel;
        stall(ctx, st, q);
        if (nb) launch_silk_synth_nb(ctx, q, st, f0, cnt);
        if (nb) stall(ctx, st, q);
        launch_silk_synth(ctx, q, st, f0, cnt, nb);
        others = true;
    } else if (st.any_silk) { // every frame that is not CELT-only (OPUSGPU_SPLIT_HYBRID=0)
        stall(ctx, st, q);
        launch_decode_step(ctx, q, st, f0, cnt, 1);
        others = true;
    }
    if (st.any_celt) {
        hipStream_t const r = rq ? rq : q;
        if (rq) {
            (void)hipStreamWaitEvent(rq, ctx->sp.ev_sparsed, 0); // (this step's CELT parse)
            const int two_back = (st.sset + OG_SILK_SETS - 2) % OG_SILK_SETS; // (recorded after this step's kernels: still step k - 2's)
            if (ctx->sp.sdone_recorded[two_back]) (void)hipStreamWaitEvent(rq, ctx->sp.ev_sdone[two_back], 0);
        }
        stall(ctx, st, r);
        if (ctx->fast_recon) launch_celt_recon_fb(ctx, r, st, f0, cnt, false);
        if (ctx->fast_recon) stall(ctx, st, r);
        launch_celt_recon(ctx, r, st, f0, cnt);
        if (rq) {
            (void)hipEventRecord(ctx->sp.ev_hrecon, rq);
            (void)hipStreamWaitEvent(q, ctx->sp.ev_hrecon, 0);
        }
    }
    if (st.any_celt || !others || modes != 7) {
        stall(ctx, st, q);
        launch_celt_post(ctx, q, st, f0, cnt, others);
    }
    if (st.srecs && (modes & 1)) { // the rare hybrid -> SILK-only transition frames (Q4), parked by k_silk_synth, through the full kernel
        stall(ctx, st, q);
        launch_decode_step(ctx, q, st, f0, cnt, 2);
    }
}
// RFC mode and OPUSGPU_SPLIT=0: one kernel for every frame of the step, in order.
static int step_single_kernel(opusgpu_ctx *ctx, const Step &st, const StepSlices *slices) {
    if (int rc = enter_step_kind(ctx, 0, st.s)) return rc;
    stall(ctx, st, st.s);
    if (ctx->mode == OPUSGPU_MODE_RFC) // every frame on the one kernel of that mode (og_rfc.hip)
        launch_decode_rfc(ctx, st.s, st);
    else // OPUSGPU_SPLIT=0 (A/B measurements): every frame through the single kernel, in order
        launch_decode_step(ctx, st.s, st, 0, st.n, 0);
    HIPCHK(ctx, hipGetLastError());
    if (ctx->mode == OPUSGPU_MODE_RFC && ctx->pipeline) { // (a later pipelined step's early parse waits for all of this one)
        HIPCHK(ctx, hipEventRecord(ctx->sp.ev_front, st.s));
        ctx->sp.front_recorded = 1;
    }
    ctx->sp.last_step_stream = st.s;
    if (ctx->mode != OPUSGPU_MODE_RFC && slices) // (one kernel for the whole step: every slice's PCM is there behind it)
        for (int i = 0; i < slices->count; i++)
            if (int rc = slices->after_slice(i)) return rc;
    return OPUSGPU_OK;
}
static int step_pipelined_silk(opusgpu_ctx *ctx, const Step &st) {
    hipStream_t const s = st.s;
    const int n = st.n, modes = st.modes;
    const int sset = st.sset;
    const bool keeps_kind = st.keeps_kind;
    // PIPELINED SILK / HYBRID STEPS (no CELT-only frames).  k_silk_parse waits on latency (0.9 ms of one lane's serial chain for 0.27 ms of issue time at
    // 65,536 frames), k_silk_synth is bound by issue: they fit next to each other, but within a step the second needs the
    // first.  Across steps the parse needs of step k only what step k's parse already knows -- the indices' history, the gain
    // index, the NLSFs, the rate and channel count, prev_mode: all of it entropy-side -- so it keeps a copy of its own
    // (SilkShadow) and runs for step k + 1 on parse_stream while step k's synthesis is under way on the step's stream -- for
    // hybrid frames followed by their CELT parse, which resumes its range decoder and carries the band energies itself as in
    // pipelined CELT-only steps.  OG_SILK_SETS sets of records and hand-offs rotate; the parse of step k waits for the last kernel of step
    // k - OG_SILK_SETS (its set's last reader -- and with it for every write to the state of streams it may have no current copy of),
    // the CELT reconstruction beside the synthesis for the last kernel of step k - 2 (back_half: the history ring).
    if (!ctx->sp.ev_sparsed) {
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sp.ev_sparsed, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sp.ev_sp, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sp.ev_spar, hipEventDisableTiming));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sp.ev_hrecon, hipEventDisableTiming));
        for (int i = 0; i < OG_SILK_SETS; i++) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sp.ev_sdone[i], hipEventDisableTiming));
    }
    if (ctx->sp.sdone_recorded[sset]) HIPCHK(ctx, hipStreamWaitEvent(ctx->sp.parse_stream, ctx->sp.ev_sdone[sset], 0));
    // One thing of the step before is not entropy-side: a SILK-only frame right behind a hybrid one (Q4) decodes a 2.5 ms CELT
    // frame in the step's LAST kernel (the full kernel's second pass), which writes the band energies a hybrid frame's CELT parse
    // predicts from.  So a step that may hold hybrid frames does not run ahead of a step that may have held SILK-only ones.
    // (a stream that keeps its mode has no such frame: OPUSGPU_STEP_KEEPS_MODE)
    const int prev_set = (sset + OG_SILK_SETS - 1) % OG_SILK_SETS; // (the step before this one)
    if (!keeps_kind && (modes & 2) && (ctx->sp.last_silk_mask & 1) && ctx->sp.sdone_recorded[prev_set])
        HIPCHK(ctx, hipStreamWaitEvent(ctx->sp.parse_stream, ctx->sp.ev_sdone[prev_set], 0));
    ctx->sp.last_silk_mask = modes;
    // (Tried: the step's frames in chunks, the CELT parse of chunk c on the reconstruction's idle stream next to the SILK parse of
    // chunk c + 1, so that the two entropy kernels do not run one after the other: hybrid-256k 12.7 -> 13.1 / 13.3 / 18.7 ms with
    // 2 / 4 / 8 chunks.  The step is bound by what all its kernels issue together, not by the length of the entropy chain.)
    front(ctx, st, ctx->sp.parse_stream, 0, n, ctx->d_shadow, (uint32_t)ctx->sp.shadow_epoch, og_debug().silk_params_aside ? ctx->sp.recon_stream : nullptr);
    HIPCHK(ctx, hipEventRecord(ctx->sp.ev_sparsed, ctx->sp.parse_stream));
    HIPCHK(ctx, hipStreamWaitEvent(s, ctx->sp.ev_sparsed, 0));
    if (og_debug().silk_params_aside) HIPCHK(ctx, hipStreamWaitEvent(s, ctx->sp.ev_spar, 0));
    // (for steps without CELT-only frames: hybrid-256k 9.50 -> 9.35 ms; with them -- a mixed step's reconstruction is three times
    // the work -- next to the synthesis it loses: mixed pages 7.02 -> 7.22 ms)
    back_half(ctx, st, s, 0, n, (og_debug().hybrid_recon_aside == 2 || (og_debug().hybrid_recon_aside && (modes & 6) == 2)) ? ctx->sp.recon_stream : nullptr);
    HIPCHK(ctx, hipEventRecord(ctx->sp.ev_sdone[sset], s));
    ctx->sp.sdone_recorded[sset] = 1;
    HIPCHK(ctx, hipGetLastError());
    return OPUSGPU_OK;
}
// A step in order: one chain of kernels on the step's stream, two halves on two streams, or sliced (opusgpu_decode_packets).
static int step_in_order(opusgpu_ctx *ctx, const Step &st, const StepSlices *slices) {
    hipStream_t const s = st.s;
    const int n = st.n;
    if (!slices && n >= 2 * OG_HALVES_MIN && og_debug().halves) {
        // TWO HALVES.  A step with SILK-only / hybrid frames runs in order -- k_silk_parse reads state the step's later kernels
        // write, so nothing of the next step can start early -- and its kernels are of two kinds: the lane-per-frame parse
        // kernels wait on latency with 13 % of their lanes active (k_silk_parse: 3.97 of a 15.4 ms step of 262,144 hybrid
        // frames), the wave-per-frame ones are bound by vector-instruction issue.  The frames of a step belong to different
        // streams and share nothing, so the step is cut in two and the halves' chains run on two streams: while one half's
        // synthesis fills the SIMDs the other half parses in its gaps.  No state changes hands: each half is the in-order chain
        // of its own frames over its own part of the records; the caller's stream forks the second one and joins it.
        // (CELT-only steps too since round 5: 2.155 -> 2.07 ms per step of 65,536 -- the floor of an in-order step is one lane's
        // parse, 0.85 ms whatever the batch, plus the reconstruction; only steps queued ahead hide the parse, opusgpu_set_pipeline)
        if (!ctx->sp.ev_fork) {
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sp.ev_fork, hipEventDisableTiming));
            HIPCHK(ctx, hipEventCreateWithFlags(&ctx->sp.ev_join, hipEventDisableTiming));
        }
        // (the second chain's stream: the one pipelined steps reconstruct on when there is one -- it is idle here, the caller's
        // stream has waited for everything on it -- rather than one more: measured with a fourth stream of the context, the two
        // chains no longer overlapped at all, 2.14 instead of 1.89 ms per SILK-NB step; the hardware queues are few)
        if (!ctx->sp.recon_stream && !ctx->sp.side_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->sp.side_stream, hipStreamNonBlocking));
        hipStream_t const side = ctx->sp.recon_stream ? ctx->sp.recon_stream : ctx->sp.side_stream;
        // (Both chains start together.  Staggered -- the second one behind the first one's parse kernels, so that one half parses
        // while the other synthesises from the start -- was measured SLOWER, 14.9 against 14.5 ms per step of 262,144 hybrid
        // frames and 2.44 against 1.90 ms per SILK-NB step: half a batch's parse takes as long as a whole batch's.)
        HIPCHK(ctx, hipEventRecord(ctx->sp.ev_fork, s));
        HIPCHK(ctx, hipStreamWaitEvent(side, ctx->sp.ev_fork, 0));
        const int h = (n / 2 + 63) / 64 * 64; // (a multiple of the parse kernels' frames per workgroup)
        front(ctx, st, s, 0, h);
        back_half(ctx, st, s, 0, h);
        front(ctx, st, side, (size_t)h, n - h);
        back_half(ctx, st, side, (size_t)h, n - h);
        HIPCHK(ctx, hipEventRecord(ctx->sp.ev_join, side));
        HIPCHK(ctx, hipStreamWaitEvent(s, ctx->sp.ev_join, 0));
    } else if (slices && slices->count > 1) {
        front(ctx, st, s, 0, n);
        for (int i = 0; i < slices->count; i++) {
            const size_t lo = slices->bounds[i], hi = slices->bounds[i + 1];
            if (hi > lo) back_half(ctx, st, s, lo, (int)(hi - lo));
            if (int rc = slices->after_slice(i)) return rc;
        }
    } else {
        front(ctx, st, s, 0, n);
        back_half(ctx, st, s, 0, n);
    }
    HIPCHK(ctx, hipGetLastError());
    if (ctx->pipeline) { // (a step that ran in order: whatever a later pipelined step runs ahead waits for all of it)
        HIPCHK(ctx, hipEventRecord(ctx->sp.ev_front, s));
        ctx->sp.front_recorded = 1;
    }
    return OPUSGPU_OK;
}
// The kernels of a step and what orders them:
//   FRONT   k_silk_parse  k_celt_parse  k_silk_synth (or the full kernel)  k_decode_step[Q4]
//   BACK    k_celt_recon_fb  k_celt_recon  ->  k_celt_post
// In order (the default): all on the step's stream.  After k_silk_parse the SILK synthesis and the CELT parse +
// reconstruction are independent (SilkRec::prev_mode, og_silk_parse.hpp); running them on two streams was measured
// (DESIGN.md section 6): next to k_celt_recon the synthesis gains nothing; next to k_celt_parse it gains 5 % on mixed-mode
// steps but costs 13 % on CELT-only steps.
// Pipelined (opusgpu_set_pipeline, a step the caller declares CELT-only; the tables are resident, so nothing here waits for
// the caller's earlier work):
//   parse_stream   [the last in-order step, post of step k-3]  k_celt_parse
//   recon_stream   [the parse, post of step k-2; in a window: every workgroup of the parse of step k+1]  k_celt_recon_fb  k_celt_recon
//   step's stream  [reconstruction of step k; in a window: the first round of the reconstruction of step k+1]  k_celt_post
// The entropy half reads one thing of the stream's state, the band energies, and writes them itself (celt_parse_lane): the
// parse of step k+1 depends on the parse of step k only.  The reconstruction touches neither the caller's buffers (its result
// codes go through ReconOut) nor anything k_celt_post reads of the step BEFORE (the history ring is written 960 samples
// further on; the ring position travels in ReconOut), so the reconstruction of step k+1 starts while k_celt_post of step k
// runs; two steps on, it waits for it (the ring holds two frames; records and ReconOut rotate through three sets).
// A step that is not declared CELT-only runs in order (ev_front: a later pipelined step's parse waits for all of it).
// PLACEMENT.  The three kernels compete for LDS: the parse is one round of 14 KB workgroups that live ~1 ms, the
// reconstruction 65,536 workgroups of 7.5 KB that live ~0.15 ms, the de-emphasis 10 KB ones that nothing waits for.  A parse
// workgroup that arrives when the CUs are full of reconstruction workgroups finds no hole that fits it (3.1 ms per step
// instead of 2.3), so the order that works is: parse of step k+1, THEN reconstruction of step k, THEN de-emphasis of step
// k-1.  Events cannot say "that kernel's workgroups have started"; round 2 approximated it with a wave that watched the wall
// clock.  When the caller queues a window of steps (opusgpu_decode_steps_device) the next step is known, and the order is a
// real dependency: the parse and reconstruction workgroups count themselves in when they start, and the stream that
// launches the dependent kernel waits on that count (hipStreamWaitValue32) -- placement does not depend on how long a launch
// or an event takes to arrive.  A single step (opusgpu_decode_step_device) cannot know whether another follows: its kernels
// are released by their data dependencies alone.
static int step_pipelined_celt(opusgpu_ctx *ctx, const Step &st, int par, int next_n) {
    hipStream_t const s = st.s;
    const int n = st.n;
    const int par2 = (par + 1) % 3; // the slot of the step two before this one
    const bool window = next_n > 0; // the next step is queued by this very call: see PLACEMENT
    // (from here on: a pipelined step -- CELT-only frames, no SILK records, no hand-off)
    // the early parse: behind the front of the step before and its own slot's last user (three steps back)
    if (ctx->sp.front_recorded) HIPCHK(ctx, hipStreamWaitEvent(ctx->sp.parse_stream, ctx->sp.ev_front, 0));
    if (ctx->sp.post_recorded[par]) HIPCHK(ctx, hipStreamWaitEvent(ctx->sp.parse_stream, ctx->sp.ev_post[par], 0));
    const bool wide = og_debug().parse_wide != 0; // (64 frames per wave: next to the reconstruction the parse costs its issue slots, not its latency)
    {
        const int grid = celt_parse_early_grid(ctx, n, wide);
        launch_jitter();
        stall(ctx, st, ctx->sp.parse_stream);
        launch_celt_parse(ctx, ctx->sp.parse_stream, st, 0, n, wide, true);
        ctx->sp.parse_started_total += (uint32_t)grid;
    }
    HIPCHK(ctx, hipEventRecord(ctx->sp.ev_parsed, ctx->sp.parse_stream));
    hipStream_t const back = ctx->sp.recon_stream;
    HIPCHK(ctx, hipStreamWaitEvent(back, ctx->sp.ev_parsed, 0));
    if (ctx->sp.post_recorded[par2]) HIPCHK(ctx, hipStreamWaitEvent(back, ctx->sp.ev_post[par2], 0)); // (the ring: 2 x 960 of 2048)
    if (window) { // ... and every workgroup of the next step's parse has its place
        const int next_grid = celt_parse_early_grid(ctx, next_n, wide);
        ctx->sp.window_parse_target = ctx->sp.parse_started_total + (uint32_t)next_grid;
        HIPCHK(ctx, hipStreamWaitValue32(back, ctx->sp.d_started, ctx->sp.window_parse_target, hipStreamWaitValueGte, 0xffffffffu));
    }
    // reconstruct (one frame per wave) ...
    if (ctx->fast_recon) {
        launch_jitter();
        stall(ctx, st, back);
        launch_celt_recon_fb(ctx, back, st, 0, n, true);
        ctx->sp.recon_started_total += (uint32_t)og_celt_recon_fb_signals(n);
    }
    stall(ctx, st, back);
    launch_celt_recon(ctx, back, st, 0, n);
    HIPCHK(ctx, hipEventRecord(ctx->sp.ev_recon, back));
    HIPCHK(ctx, hipStreamWaitEvent(s, ctx->sp.ev_recon, 0));
    // Nothing waits for the de-emphasis for two steps, and placed before the next step's reconstruction its 10 KB workgroups
    // take room that kernel -- the critical one -- would use: in a window it is held until the first round of that
    // reconstruction has started (its count of started workgroups, one in 64 counted)
    if (window && ctx->fast_recon) {
        const int first_round = std::min(og_celt_recon_fb_signals(next_n), 32);
        ctx->sp.window_recon_target = ctx->sp.recon_started_total + (uint32_t)first_round;
        HIPCHK(ctx, hipStreamWaitValue32(s, ctx->sp.d_started + 16, ctx->sp.window_recon_target, hipStreamWaitValueGte, 0xffffffffu));
    }
    // ... -> de-emphasis and PCM (one (frame, channel) per lane); the result codes
    launch_jitter();
    stall(ctx, st, s);
    launch_celt_post(ctx, s, st, 0, n, false);
    HIPCHK(ctx, hipEventRecord(ctx->sp.ev_post[par], s));
    ctx->sp.post_recorded[par] = 1;
    HIPCHK(ctx, hipGetLastError());
    return OPUSGPU_OK;
}

static int decode_step_impl(opusgpu_ctx *ctx, int n, const void *d_descs, const void *d_arena, void *d_pcm, void *d_result,
                            void *hip_stream, bool tables_resident, int modes = 7, int next_n = 0, const StepSlices *slices = nullptr) {
    if (!ctx || n < 0 || !ctx->d_streams) return OPUSGPU_BAD_ARG;
    if (n == 0) return OPUSGPU_OK;
    if (!d_descs || !d_arena || !d_pcm || !d_result) return OPUSGPU_BAD_ARG;
    if ((uintptr_t)d_arena & 15) return OPUSGPU_BAD_ARG; // (the parse kernels fetch packets as aligned 16-byte pieces, og_range.hpp)
    StepPipeline &sp = ctx->sp;
    Step st = {};
    st.s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    st.n = n, st.descs = d_descs, st.arena = d_arena, st.pcm = d_pcm, st.result = d_result;
    st.pcm_stride = (ctx->mode == OPUSGPU_MODE_RFC ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES) * ctx->channels;
    ctx->last_descs = d_descs;
    ctx->last_n = ctx->mode == OPUSGPU_MODE_RFC || !ctx->split_celt ? 0 : n;
    ctx->last_had_silk_recs = ctx->split_celt && ctx->split_hybrid;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->mode == OPUSGPU_MODE_RFC || !ctx->split_celt) return step_single_kernel(ctx, st, slices);
    // `modes` (bit 0 SILK-only, 1 hybrid, 2 CELT-only frames may be present; 7 = not known): the kernels of modes the caller
    // rules out are not launched; k_celt_post reports a frame of such a mode as OPUSGPU_BAD_ARG
    st.keeps_kind = (modes & OPUSGPU_STEP_KEEPS_MODE) != 0;
    modes &= 7;
    if (!modes) modes = 7;
    st.modes = modes;
    st.any_silk = (modes & 3) != 0, st.any_celt = (modes & 6) != 0;
    // Only a step the caller declares CELT-only runs ahead of the step before it.  (Round 2 also ran the CELT-only part of a
    // mixed step's parse ahead: 4 % on the mixed-pages workload.  Cutting such a step into two halves -- step_in_order -- gains 6 %,
    // and the two do not combine: a mixed or undeclared step takes the halves.)
    const bool pipe = ctx->pipeline && tables_resident && modes == 4;
    // ... and a step declared free of CELT-only frames runs its parse kernels ahead (PIPELINED SILK / HYBRID STEPS, step_pipelined_silk)
    // -- or, with the caller's word that no stream of the step ever changes its mode (OPUSGPU_STEP_KEEPS_MODE), a step of ANY mix with
    // SILK-only / hybrid frames in it: its CELT-only frames' parse carries the band energies like a pipelined CELT-only step's, and a
    // CELT-only frame cannot make another stream's SILK copy stale
    const bool pipe_silk = ctx->pipeline && tables_resident && ((modes & 4) == 0 || st.keeps_kind) && (modes & 3) != 0 && ctx->split_hybrid && !slices &&
                           (modes == 1 ? og_debug().silk_pipeline : og_debug().hybrid_pipeline);
    if (int rc = enter_step_kind(ctx, pipe ? 1 : pipe_silk ? 2 : 0, st.s, st.keeps_kind, (modes & 4) != 0)) return rc;
    if (ctx->pipeline && sp.last_step_stream && sp.last_step_stream != st.s) {
        // consecutive steps on different streams: nothing orders them but the caller, so nothing may run ahead either
        // (sync_in_flight leaves the context's own stream to its caller: the last step's stream is waited for by name)
        HIPCHK(ctx, hipStreamSynchronize(sp.last_step_stream));
        if (int rc = sync_in_flight(ctx)) return rc;
        sp.drained();
    }
    sp.last_step_stream = st.s;
    // The records, the reconstruction's per-frame output and the hand-off buffers only grow; growing frees the old one, which
    // waits for the device to go idle.  Records and reconstruction output exist twice: pipelined steps alternate.
    if (pipe) sp.slot = (sp.slot + 1) % 3;
    if (pipe_silk) sp.silk_slot = (sp.silk_slot + 1) % OG_SILK_SETS;
    st.sset = pipe_silk ? sp.silk_slot : 0;
    const int par = pipe ? sp.slot : pipe_silk ? 3 + st.sset : 0; // this step's slot of records and reconstruction output
    if (int rc = grow_step_slot(ctx, par, (size_t)n)) return rc; // (a window's slots were sized before its first launch)
    if (ctx->split_hybrid && st.any_silk)
        if (int rc = grow_silk_set(ctx, st.sset, (size_t)n, pipe_silk ? st.s : nullptr)) return rc;
    st.recs = ctx->d_recs[par], st.rout = ctx->d_rout[par];
    st.handoff = ctx->split_hybrid && st.any_silk ? ctx->d_handoff[st.sset] : nullptr;
    st.srecs = ctx->split_hybrid && st.any_silk ? ctx->d_srecs[st.sset] : nullptr;
    ctx->last_recs = st.recs;
    ctx->last_srecs = st.srecs;
    ctx->last_had_silk_recs = st.srecs != nullptr;
    if (pipe_silk) return step_pipelined_silk(ctx, st);
    if (pipe) return step_pipelined_celt(ctx, st, par, next_n);
    return step_in_order(ctx, st, slices);
}

// opusgpu_decode_steps_device: n_steps steps queued as a window (the arguments are checked, max_n is the largest step's frames)
static int decode_window(opusgpu_ctx *ctx, int n_steps, const int32_t *n, int max_n, const void *const *d_descs, const void *const *d_arena,
                         void *const *d_pcm, void *const *d_result, void *hip_stream, int m) {
    if (ctx->sp.d_started && (ctx->sp.parse_started_total > 0x70000000u || ctx->sp.recon_started_total > 0x70000000u)) {
        // the start counters only grow: long before they could wrap they restart from zero, on an idle device
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if (int rc = sync_in_flight(ctx)) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemset(ctx->sp.d_started, 0, 128));
        ctx->sp.parse_started_total = ctx->sp.recon_started_total = 0;
    }
    if (ctx->pipeline && m == 4 && ctx->split_celt && ctx->mode != OPUSGPU_MODE_RFC) {
        // ... and so is every allocation: the record slots only grow, growing frees the old buffer, and hipFree waits for ALL
        // streams of the device -- among them the one whose head is such a wait for a parse that this thread has yet to launch.
        // All three slots take the window's largest step now, while nothing of the window is queued.
        HIPCHK(ctx, hipSetDevice(ctx->device));
        for (int par = 0; par < 3; par++)
            if (int rc = grow_step_slot(ctx, par, (size_t)max_n)) return rc;
    }
    for (int k = 0; k < n_steps; k++) {
        const int next_n = k + 1 < n_steps ? n[k + 1] : 0;
        const int rc = decode_step_impl(ctx, n[k], d_descs[k], d_arena[k], d_pcm[k], d_result[k], hip_stream, true, m, next_n > 0 ? next_n : 0);
        if (rc) { // (a HIP error in the middle of a window: let go of what the steps before it wait for, then report it)
            release_window_waits(ctx);
            return rc;
        }
    }
    ctx->sp.window_parse_target = ctx->sp.window_recon_target = 0; // (every wait of this window has its kernel queued behind it)
    return OPUSGPU_OK;
}
