// TEST-ONLY: the decode-step scheduler (csrc/og_step.hpp) against a RECORDING DOUBLE of what it calls -- the HIP runtime entry
// points and the launch wrappers that og_api.hip defines next to the kernels.  Nothing of the HIP runtime is linked and no GPU is
// opened: every call appends one line to a trace, from which tests/test_step_order.py checks the ordering rules (what happens
// before what, through streams, events and host synchronisation).  The double is never linked into the product.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include "og_step.hpp"

static std::string g_trace;
static opusgpu_ctx *g_ctx;
static int g_step = -1, g_fail_step = -1;
static std::map<const void *, std::string> g_names; // the caller's streams, and the scheduler's short-lived ones
static uint32_t g_parse_started, g_recon_started;    // what the kernels would have counted at d_started / d_started + 16
static int g_handles;
static char g_tables[4096]; // step k's descriptor table is g_tables + k: the wrappers tell the step from it

static void say(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_trace += buf;
    g_trace += '\n';
}
static std::string stream_name(hipStream_t q) {
    const StepPipeline &sp = g_ctx->sp;
    if (q == g_ctx->stream) return "ctx";
    if (q && q == sp.parse_stream) return "parse";
    if (q && q == sp.recon_stream) return "recon";
    if (q && q == sp.side_stream) return "side";
    auto it = g_names.find(q);
    return it != g_names.end() ? it->second : "?";
}
static std::string event_name(hipEvent_t e) {
    const StepPipeline &sp = g_ctx->sp;
    const struct {
        hipEvent_t e;
        const char *name;
    } one[] = {{sp.ev_front, "front"}, {sp.ev_parsed, "parsed"}, {sp.ev_recon, "recon"}, {sp.ev_sparsed, "sparsed"}, {sp.ev_sp, "sp"},
               {sp.ev_spar, "spar"},   {sp.ev_hrecon, "hrecon"}, {sp.ev_fork, "fork"},   {sp.ev_join, "join"}};
    for (auto &o : one)
        if (e && e == o.e) return o.name;
    for (int i = 0; i < 3; i++)
        if (e && e == sp.ev_post[i]) return "post" + std::to_string(i);
    for (int i = 0; i < OG_SILK_SETS; i++)
        if (e && e == sp.ev_sdone[i]) return "sdone" + std::to_string(i);
    return "?";
}
template <class T>
static T new_handle() { return (T)(uintptr_t)(0x1000 + 16 * ++g_handles); }

// ---- the HIP runtime, as far as the scheduler calls it ---------------------------------------------------------------
extern "C" {
const char *hipGetErrorString(hipError_t) { return "injected"; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { return *least = 0, *greatest = -1, hipSuccess; }
hipError_t hipStreamCreateWithPriority(hipStream_t *q, unsigned, int) { return *q = new_handle<hipStream_t>(), hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *q, unsigned) {
    *q = new_handle<hipStream_t>();
    g_names[*q] = "temp"; // (the library's own streams are named by the field that holds them)
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return *e = new_handle<hipEvent_t>(), hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipMalloc(void **p, size_t bytes) { return *p = calloc(1, bytes), hipSuccess; }
hipError_t hipFree(void *p) { return free(p), hipSuccess; }
hipError_t hipMemset(void *p, int, size_t) {
    if (p == g_ctx->sp.d_started) say("memset started"), g_parse_started = g_recon_started = 0;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t q) { return say("sync %s", stream_name(q).c_str()), hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t q) {
    if (g_step >= 0 && g_step == g_fail_step) return hipErrorUnknown; // (the injected error: this step queues nothing more)
    return say("record %s stream=%s", event_name(e).c_str(), stream_name(q).c_str()), hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t q, hipEvent_t e, unsigned) {
    return say("wait %s stream=%s", event_name(e).c_str(), stream_name(q).c_str()), hipSuccess;
}
static const char *counter_name(void *p) { return p == g_ctx->sp.d_started ? "parse" : p == g_ctx->sp.d_started + 16 ? "recon" : "?"; }
hipError_t hipStreamWaitValue32(hipStream_t q, void *p, uint32_t v, unsigned flags, uint32_t mask) {
    say("waitvalue %s>=%u stream=%s%s", counter_name(p), v, stream_name(q).c_str(), flags == hipStreamWaitValueGte && mask == 0xffffffffu ? "" : " ?");
    return hipSuccess;
}
hipError_t hipStreamWriteValue32(hipStream_t q, void *p, uint32_t v, unsigned) {
    return say("writevalue %s=%u stream=%s", counter_name(p), v, stream_name(q).c_str()), hipSuccess;
}
int og_celt_recon_fb_signals(int n) { return (n + 4095) / 4096; }
} // extern "C"

// ---- the launch wrappers ---------------------------------------------------------------------------------------------
const size_t og_parse_rec_bytes = 8, og_recon_out_bytes = 4, og_silk_handoff_bytes = 2, og_silk_rec_bytes = 16;
static int grow(opusgpu_ctx *, void **p, size_t *cap, size_t need) { // (as in og_api.hip: freeing waits for the device)
    say("grow");
    free(*p);
    *p = calloc(1, need);
    *cap = need;
    return OPUSGPU_OK;
}
static void launched(const char *kernel, hipStream_t q, const Step *st, size_t f0, int cnt, int grid, const char *fmt = "", ...) {
    if (st) g_step = (int)((const char *)st->descs - g_tables);
    char extra[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(extra, sizeof(extra), fmt, ap);
    va_end(ap);
    say("launch %s stream=%s step=%d frames=[%zu,%zu) grid=%d%s", kernel, stream_name(q).c_str(), g_step, f0, f0 + (size_t)cnt, grid, extra);
}
// which set of records the step was given (by buffer: the context's sets are distinct allocations)
static int recs_set(const Step &st) {
    for (int i = 0; i < 6; i++)
        if (st.recs == g_ctx->d_recs[i] && st.rout == g_ctx->d_rout[i]) return i;
    return -1;
}
static int silk_set(const Step &st) {
    for (int i = 0; i < OG_SILK_SETS; i++)
        if (st.srecs && st.srecs == g_ctx->d_srecs[i] && st.handoff == g_ctx->d_handoff[i]) return i;
    return -1;
}
void launch_stream_stall(opusgpu_ctx *, hipStream_t q) { launched("k_stream_stall", q, nullptr, 0, 0, 1); }
void launch_decode_rfc(opusgpu_ctx *, hipStream_t q, const Step &st) { launched("k_decode_rfc", q, &st, 0, st.n, st.n); }
void launch_decode_step(opusgpu_ctx *, hipStream_t q, const Step &st, size_t f0, int cnt, int pass) {
    launched("k_decode_step", q, &st, f0, cnt, pass == 2 ? (cnt + 63) / 64 : cnt, " pass=%d silk=%d", pass, pass == 2 ? silk_set(st) : -1);
}
void launch_silk_parse(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch) {
    launched("k_silk_parse", q, &st, f0, cnt, (cnt + 31) / 32, " silk=%d shadow=%d epoch=%u", silk_set(st), shadow ? shadow == ctx->d_shadow : 0, epoch);
}
void launch_silk_parse64(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch) {
    launched("k_silk_parse64", q, &st, f0, cnt, (cnt + 63) / 64, " silk=%d shadow=%d epoch=%u", silk_set(st), shadow ? shadow == ctx->d_shadow : 0, epoch);
}
void launch_silk_params(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch) {
    launched("k_silk_params", q, &st, f0, cnt, (cnt + 31) / 32, " silk=%d shadow=%d epoch=%u", silk_set(st), shadow ? shadow == ctx->d_shadow : 0, epoch);
}
int celt_parse_early_grid(const opusgpu_ctx *ctx, int cnt, bool wide) {
    const int per = (wide ? 64 : 32) * ctx->parse_groups;
    return (cnt + per - 1) / per;
}
void launch_celt_parse(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool wide, bool early) {
    const int per = wide ? 64 : 32, grid = early ? celt_parse_early_grid(ctx, cnt, wide) : (cnt + per - 1) / per;
    if (early) g_parse_started += (uint32_t)grid;
    launched(wide ? "k_celt_parse64" : "k_celt_parse", q, &st, f0, cnt, grid, " recs=%d silk=%d early=%d started=%u", recs_set(st), silk_set(st), (int)early,
             early ? g_parse_started : 0u);
}
void launch_celt_recon_fb(opusgpu_ctx *, hipStream_t q, const Step &st, size_t f0, int cnt, bool counts_in) {
    const uint32_t before = g_recon_started;
    if (counts_in) g_recon_started += (uint32_t)og_celt_recon_fb_signals(cnt);
    launched("k_celt_recon_fb", q, &st, f0, cnt, cnt, " recs=%d hybrid=%d started=%u+%u", recs_set(st), st.handoff ? 1 : 0, counts_in ? before : 0u,
             g_recon_started - before);
}
void launch_celt_recon(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt) {
    launched("k_celt_recon", q, &st, f0, cnt, ctx->fast_recon ? (cnt + 63) / 64 : cnt, " recs=%d hybrid=%d rest_only=%d", recs_set(st), st.handoff ? 1 : 0,
             ctx->fast_recon);
}
void launch_celt_post(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool others) {
    launched("k_celt_post", q, &st, f0, cnt, (cnt * ctx->channels + 63) / 64, " recs=%d silk=%d modes=%d others=%d", recs_set(st), silk_set(st), st.modes,
             (int)others);
}
void launch_silk_synth(opusgpu_ctx *, hipStream_t q, const Step &st, size_t f0, int cnt, int nb_done) {
    launched("k_silk_synth", q, &st, f0, cnt, cnt, " silk=%d nb_done=%d", silk_set(st), nb_done);
}
void launch_silk_synth_nb(opusgpu_ctx *, hipStream_t q, const Step &st, size_t f0, int cnt) {
    launched("k_silk_synth_nb", q, &st, f0, cnt, cnt, " silk=%d", silk_set(st));
}

// ---- the driver ------------------------------------------------------------------------------------------------------
// One scenario on a fresh context: steps k = 0 .. n_steps - 1 of n[k] frames with mode mask modes[k] (as for
// opusgpu_decode_step_device_modes; OPUSGPU_STEP_KEEPS_MODE included) on stream stream_id[k] (0: the context's, else the caller's
// stream of that number).  window[k] > 1: steps k .. k + window[k] - 1 are queued by one opusgpu_decode_steps_device call.
// flags[k]: 1 = the tables are not resident (the host-buffer path's steps), 2 = two slices.  fail_step: the step at which the
// runtime reports an error (-1: none).  -> the trace; "step k ..." lines separate the steps, "rc ..." follows each call.
extern "C" const char *og_step_test_run(int pipeline, int rfc, int n_steps, const int *n, const int *modes, const int *stream_id, const int *window,
                                        const int *flags, int fail_step) {
    g_trace.clear();
    g_names.clear();
    g_parse_started = g_recon_started = 0;
    g_step = -1;
    g_fail_step = fail_step;
    opusgpu_ctx *ctx = g_ctx = new opusgpu_ctx();
    ctx->device = 0;
    ctx->stream = new_handle<hipStream_t>();
    ctx->d_streams = (og::StreamState *)calloc(1, 64);
    ctx->d_shadow = calloc(1, 64);
    ctx->n_streams = 1 << 20;
    ctx->channels = 2;
    ctx->split_celt = og_debug().split; // (as opusgpu_ctx_create does)
    ctx->split_hybrid = og_debug().split_hybrid;
    ctx->fast_recon = og_debug().fast_recon;
    ctx->parse_groups = og_debug().parse_groups;
    ctx->stall_ticks = og_debug().stall_us;
    ctx->mode = rfc ? OPUSGPU_MODE_RFC : OPUSGPU_MODE_REFERENCE;
    if (pipeline && pipeline_create(ctx)) return "pipeline_create failed";
    ctx->pipeline = pipeline ? 1 : 0;
    g_trace.clear(); // (the trace is about the steps)
    hipStream_t user[8];
    for (int i = 1; i < 8; i++) g_names[user[i] = new_handle<hipStream_t>()] = "user" + std::to_string(i);
    static char arena[64] __attribute__((aligned(16)));
    char *const tables = g_tables;
    for (int k = 0; k < n_steps;) {
        void *const s = stream_id[k] ? (void *)user[stream_id[k] & 7] : nullptr;
        int rc;
        if (window[k] > 1) {
            const int w = window[k];
            const void *dd[64], *aa[64];
            void *pp[64], *rr[64];
            int max_n = 0;
            for (int i = 0; i < w; i++) dd[i] = tables + k + i, aa[i] = arena, pp[i] = tables, rr[i] = tables, max_n = std::max(max_n, n[k + i]);
            say("window %d steps=%d", k, w);
            g_step = k;
            rc = decode_window(ctx, w, n + k, max_n, dd, aa, pp, rr, s, modes[k] & 7);
            k += w;
        } else {
            g_step = k;
            say("step %d n=%d modes=%d stream=%s", k, n[k], modes[k], s ? g_names[s].c_str() : "ctx");
            StepSlices sl;
            size_t b[3] = {0, (size_t)n[k] / 2, (size_t)n[k]};
            sl.count = 2, sl.bounds = b, sl.after_slice = [](int i) { return say("after_slice %d", i), 0; };
            rc = decode_step_impl(ctx, n[k], tables + k, arena, tables, tables, s, !(flags[k] & 1), modes[k], 0, (flags[k] & 2) ? &sl : nullptr);
            k++;
        }
        say("rc %d", rc);
    }
    g_step = -1;
    pipeline_destroy(ctx);
    for (int i = 0; i < 6; i++) free(ctx->d_recs[i]), free(ctx->d_rout[i]);
    for (int i = 0; i < OG_SILK_SETS; i++) free(ctx->d_handoff[i]), free(ctx->d_srecs[i]);
    free(ctx->d_streams);
    free(ctx->d_shadow);
    delete ctx;
    g_ctx = nullptr;
    return g_trace.c_str();
}
