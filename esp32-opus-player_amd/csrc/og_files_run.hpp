// og_files_run.hpp -- the whole-file decode driver: a planned batch (og_batch.hpp) through its steps, the assembly of step k behind
// step k, and the tracks' outcome back to the caller's arrays.  What is uploaded before what, what a failing step leaves queued,
// what is freed when and what the caller's arrays hold after a failure is decided here and nowhere else.
//
// Host code only.  Included by og_api.hip in front of og_tracks.hpp and og_ms_tracks.hpp, whose opusgpu_files_decode and
// opusgpu_ms_files_decode supply the operations, and by the CPU test (tests/emul/og_files_run_test.cpp), which supplies a recording
// double of them and of the four HIP runtime entry points used here: this file compiles with a plain host compiler.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <vector>
#include "og_batch.hpp"

// What the two kinds of decoder do differently.  Every callable returns an OPUSGPU_* code.
struct FilesRunOps {
    int device = 0;
    // Extra device buffers, bytes per slot of the largest step (0: none): the stereo path's PCM rows and result codes.  The
    // multistream object brings its own elementary buffers.
    size_t extra_slot_bytes[2] = {0, 0};
    std::function<int(int n_files)> reset; // decoders 0 .. n_files - 1, fully
    // step k: n slots, their descriptors (n * width) and the arena in device memory, the planner's mode mask
    std::function<int(int k, int n, const void *d_descs, const void *d_arena, int modes, void *const *extra)> step;
    // its assembly: n segments in device memory, the track states
    std::function<int(int k, int n, const void *d_segs, void *const *extra, void *d_state)> assemble;
    std::function<int()> drain; // everything queued has completed
    std::function<int(int code, const char *what, hipError_t e)> hip_failed; // keeps the message, returns `code`
    std::function<void()> loop_begin, loop_end; // optional: around the step loop, on the queuing thread
};

// The tracks' outcome from their state records: a track with a failed frame ends at the planned start of its first failing packet
// and reports that frame's code, any other has the plan's length and status.  Both out arrays may be null.
template <class PacketStart> // (file, packet_seq) -> samples
inline void fold_track_outcome(int n_files, const opusgpu_track_state *state, const opusgpu_file_info *info, PacketStart packet_start,
                               int64_t *track_lengths_out, int32_t *status_out) {
    for (int i = 0; i < n_files; i++) {
        const bool bad = state[i].first_bad != INT32_MAX;
        if (track_lengths_out) track_lengths_out[i] = bad ? packet_start(i, state[i].first_bad) : info[i].track_samples;
        if (status_out) {
            status_out[2 * i] = bad ? state[i].code : info[i].status;
            status_out[2 * i + 1] = bad ? state[i].first_bad : -1;
        }
    }
}

// Runs the batch.  A batch without a slot touches no device call (d_tracks may be null then).  On any failure the caller's arrays
// are left as they were; whatever was queued has been drained and every device buffer of this call is free again.
inline int files_run(const og_batch &b, const FilesRunOps &ops, void *d_tracks, int64_t *track_lengths_out, int32_t *status_out) {
#define OGF_CHK(call)                                                                  \
    do {                                                                               \
        const hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return ops.hip_failed(OPUSGPU_ERR_HIP, #call, e_);       \
    } while (0)
    const size_t n_steps = b.step_begin.empty() ? 0 : b.step_begin.size() - 1;
    const size_t total = n_steps ? b.step_begin[n_steps] : 0, W = (size_t)b.width;
    size_t max_n = 0;
    for (size_t k = 0; k < n_steps; k++) max_n = std::max(max_n, b.step_begin[k + 1] - b.step_begin[k]);
    std::vector<opusgpu_track_state> st((size_t)b.n_files, opusgpu_track_state{INT32_MAX, 0});
    if (total > 0) {
        if (!d_tracks || ((uintptr_t)d_tracks & 127)) return OPUSGPU_BAD_ARG;
        OGF_CHK(hipSetDevice(ops.device));
        // device copies of the batch; the tables of every step lie step after step behind step 0's (og_files.cpp)
        struct Bufs {
            void *p[6] = {};
            ~Bufs() {
                for (void *q : p)
                    if (q) (void)hipFree(q);
            }
        } d;
        void *&d_descs = d.p[0], *&d_segs = d.p[1], *&d_arena = d.p[2], *&d_state = d.p[3];
        void *const *extra = d.p + 4;
        // One buffer of each extra kind, sized for the largest step, serves every step: whatever of step k + 1 runs ahead of step k
        // (parse, reconstruction) touches neither, and the kernels that write them are queued on the steps' stream -- or on one
        // that forks from it -- behind the assembly that reads them.
        const size_t sizes[6] = {total * W * sizeof(opusgpu_frame_desc), total * sizeof(opusgpu_track_seg), b.arena.size(),
                                 (size_t)b.n_files * sizeof(opusgpu_track_state), max_n * ops.extra_slot_bytes[0],
                                 max_n * ops.extra_slot_bytes[1]};
        for (int i = 0; i < 6; i++) {
            if (i >= 4 && !sizes[i]) continue;
            const hipError_t e = hipMalloc(&d.p[i], sizes[i] + 16);
            if (e != hipSuccess) return ops.hip_failed(OPUSGPU_ALLOC_FAIL, "hipMalloc(files)", e);
        }
        // complete in device memory before the first step: what pipelined steps ask of their tables
        OGF_CHK(hipMemcpy(d_descs, b.descs.data(), sizes[0], hipMemcpyHostToDevice));
        OGF_CHK(hipMemcpy(d_segs, b.segs.data(), sizes[1], hipMemcpyHostToDevice));
        OGF_CHK(hipMemcpy(d_arena, b.arena.data(), sizes[2], hipMemcpyHostToDevice));
        OGF_CHK(hipMemcpy(d_state, st.data(), sizes[3], hipMemcpyHostToDevice));
        int rc = ops.reset(b.n_files);
        if (rc) return rc;
        // The steps, the assembly of step k behind step k.  The first failure ends the queuing; what is queued still drains.
        if (ops.loop_begin) ops.loop_begin();
        for (size_t k = 0; k < n_steps && !rc; k++) {
            const size_t at = b.step_begin[k];
            const int n = (int)(b.step_begin[k + 1] - at);
            if (n <= 0) continue;
            rc = ops.step((int)k, n, (const char *)d_descs + at * W * sizeof(opusgpu_frame_desc), d_arena, b.step_modes[k], extra);
            if (!rc) rc = ops.assemble((int)k, n, (const char *)d_segs + at * sizeof(opusgpu_track_seg), extra, d_state);
        }
        if (ops.loop_end) ops.loop_end();
        const int rd = ops.drain();
        if (!rc) rc = rd;
        if (rc) return rc;
        OGF_CHK(hipMemcpy(st.data(), d_state, sizes[3], hipMemcpyDeviceToHost));
    }
    fold_track_outcome(b.n_files, st.data(), b.info.data(), [&](int file, int seq) { return b.packet_start_of(file, seq); }, track_lengths_out,
                       status_out);
    return OPUSGPU_OK;
}
#undef OGF_CHK
