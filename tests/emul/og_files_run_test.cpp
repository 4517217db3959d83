// TEST-ONLY: the whole-file decode driver (csrc/og_files_run.hpp) against a RECORDING DOUBLE of what it calls -- four HIP runtime
// entry points and the operations the two decode calls supply.  Nothing of the HIP runtime is linked and no GPU is opened: every
// call appends one line to a trace, from which tests/test_files_run.py checks what is uploaded before what, what a failing step
// leaves queued, what is freed when and what the caller's arrays hold afterwards.  The double is never linked into the product.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "og_files_run.hpp"

static std::string g_trace;
static int g_mallocs, g_memcpys, g_fail_malloc, g_fail_memcpy; // calls so far; the call (1-based) that fails, 0: none

static void say(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_trace += buf;
    g_trace += '\n';
}

// ---- the HIP runtime, as far as the driver calls it ------------------------------------------------------------------
extern "C" {
hipError_t hipSetDevice(int device) { return say("setdevice %d", device), hipSuccess; }
hipError_t hipMalloc(void **p, size_t bytes) {
    if (++g_mallocs == g_fail_malloc) return say("malloc FAILED bytes=%zu", bytes), hipErrorOutOfMemory;
    *p = calloc(1, bytes);
    return say("malloc %p bytes=%zu", *p, bytes), hipSuccess;
}
hipError_t hipFree(void *p) { return say("free %p", p), free(p), hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    const char *dir = kind == hipMemcpyHostToDevice ? "h2d" : kind == hipMemcpyDeviceToHost ? "d2h" : "?";
    if (++g_memcpys == g_fail_memcpy) return say("memcpy %s FAILED", dir), hipErrorUnknown;
    memcpy(dst, src, bytes);
    return say("memcpy %s dst=%p src=%p bytes=%zu", dir, dst, src, bytes), hipSuccess;
}
} // extern "C"

// The batch every scenario runs: 3 files, 3 steps of 3, 2 and 1 slots (file 2 has one frame, file 1 two, file 0 three).
// Descriptors and segments carry their slot number, so that a trace line names what a pointer points at.
// shape 1: the same files with no frame at all; shape 2: a step without slots between steps 0 and 1 (the planner makes none).
static og_batch make_batch(int width, int shape) {
    og_batch b;
    b.n_files = 3, b.channels = 2, b.mode = 0, b.width = width;
    const bool empty = shape == 1;
    if (empty)
        b.step_begin = {0};
    else if (shape == 2)
        b.step_begin = {0, 3, 3, 5, 6}, b.step_modes = {4 | 8, 0, 4, 2};
    else
        b.step_begin = {0, 3, 5, 6}, b.step_modes = {4 | 8, 4, 2};
    const size_t total = b.step_begin.back();
    for (size_t s = 0; s < total; s++) {
        for (int w = 0; w < width; w++) b.descs.push_back(opusgpu_frame_desc{0, (int32_t)(100 * s + w), 1, 0});
        opusgpu_track_seg sg{};
        sg.slot = (int32_t)s;
        b.segs.push_back(sg);
    }
    b.slot_files.assign(total, 0);
    b.arena.assign(empty ? 16 : 48, 0x5a);
    b.info.assign(3, opusgpu_file_info{});
    for (int i = 0; i < 3; i++) b.info[i].status = i == 1 ? -136 : 0, b.info[i].track_samples = 1000 * (i + 1);
    // packets + 1 entries per file: 4, 3 and 2
    b.packet_start = {0, 300, 600, 1000, 0, 900, 2000, 0, 3000};
    b.packet_begin = {0, 4, 7, 9};
    return b;
}

// One scenario -> the trace.  shape: make_batch's.  fail_malloc / fail_memcpy: the n-th such call fails (1-based, 0: none);
// fail_step / fail_code: step fail_step returns fail_code (-1: none); bad_file / bad_seq / bad_code: what the "device" leaves in the state record of file
// bad_file while it drains (-1: nothing).  The out arrays hold -77 before the call; "out ..." lines report them after it.
extern "C" const char *og_files_run_test(int width, int extra, int shape, int null_tracks, int fail_malloc, int fail_memcpy, int fail_step,
                                         int fail_code, int bad_file, int bad_seq, int bad_code) {
    g_trace.clear();
    g_mallocs = g_memcpys = 0;
    g_fail_malloc = fail_malloc, g_fail_memcpy = fail_memcpy;
    const og_batch b = make_batch(width, shape);
    void *d_state_seen = nullptr;
    FilesRunOps ops;
    ops.device = 5;
    if (extra) ops.extra_slot_bytes[0] = 1000, ops.extra_slot_bytes[1] = 4;
    ops.reset = [&](int n) { return say("reset %d", n), 0; };
    ops.step = [&](int k, int n, const void *d_descs, const void *d_arena, int modes, void *const *x) {
        // (the pointers lie in the double's "device" memory, which the uploads have filled: the first descriptor names its slot)
        say("step %d n=%d descs=%p first_offset=%d arena=%p modes=%d extra=%p,%p", k, n, d_descs, ((const opusgpu_frame_desc *)d_descs)->offset,
            d_arena, modes, x[0], x[1]);
        return k == fail_step ? fail_code : 0;
    };
    ops.assemble = [&](int k, int n, const void *d_segs, void *const *x, void *d_state) {
        d_state_seen = d_state;
        return say("assemble %d n=%d segs=%p first_slot=%d extra=%p,%p state=%p", k, n, d_segs, ((const opusgpu_track_seg *)d_segs)->slot, x[0],
                   x[1], d_state),
               0;
    };
    ops.drain = [&] {
        if (bad_file >= 0 && d_state_seen) ((opusgpu_track_state *)d_state_seen)[bad_file] = opusgpu_track_state{bad_seq, bad_code};
        return say("drain"), 0;
    };
    ops.hip_failed = [&](int code, const char *what, hipError_t) { return say("hip_failed %d %.24s", code, what), code; };
    ops.loop_begin = [&] { say("loop_begin"); };
    ops.loop_end = [&] { say("loop_end"); };
    int64_t lengths[3] = {-77, -77, -77};
    int32_t status[6] = {-77, -77, -77, -77, -77, -77};
    static char tracks[256] __attribute__((aligned(128)));
    const int rc = files_run(b, ops, null_tracks ? nullptr : tracks, lengths, status);
    say("rc %d", rc);
    for (int i = 0; i < 3; i++) say("out %d length=%lld status=%d bad_packet=%d", i, (long long)lengths[i], status[2 * i], status[2 * i + 1]);
    return g_trace.c_str();
}

// fold_track_outcome alone over two files: file 0 clean (planned 1000 samples, status -136), file 1 with the given state; its
// packets start at 0, 480 and 960.  which: bit 0 a lengths array, bit 1 a status array (else null).  out: 2 lengths, 4 status words.
extern "C" void og_files_fold_test(int first_bad, int code, int which, int64_t *out_lengths, int32_t *out_status) {
    const opusgpu_track_state st[2] = {{INT32_MAX, 0}, {first_bad, code}};
    opusgpu_file_info info[2] = {};
    info[0].track_samples = 1000, info[0].status = -136;
    info[1].track_samples = 1440, info[1].status = 0;
    const int64_t starts[4] = {0, 480, 960, 1440};
    fold_track_outcome(2, st, info, [&](int file, int seq) { return file == 1 && seq >= 0 && seq < 4 ? starts[seq] : (int64_t)-1; },
                       (which & 1) ? out_lengths : nullptr, (which & 2) ? out_status : nullptr);
}
