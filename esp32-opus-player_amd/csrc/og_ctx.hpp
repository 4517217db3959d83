// og_ctx.hpp -- the context behind the C ABI (include/opusgpu.h): host-side state only, no device code.
//
// Included by og_step.hpp behind StepPipeline (the context holds one), and through it by og_api.hip -- and by the CPU ordering
// test (tests/emul/og_step_test.cpp), which is why nothing here needs a kernel header or a device compiler.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>
#include "../../include/opusgpu.h"
#include "og_debug.hpp"

namespace og {
struct StreamState; // og_state.hpp
}
enum { OPUSGPU_COPY_PIECES = 16, OPUSGPU_COPY_THREADS = 8 };

// ---- context ----------------------------------------------------------------------------------------
// Worker threads of the host-buffer path, started once per context: a large opusgpu_decode_packets call hands them ranges of its
// packets four times (scan, place per part, delivery); starting 16 threads each time cost 0.6 ms per hand-over at 65,536 packets.
struct HostPool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable wake, done;
    std::function<void(int)> job;
    int generation = 0, want = 0, pending = 0;
    bool quit = false;
    ~HostPool() {
        {
            std::lock_guard<std::mutex> l(m);
            quit = true;
        }
        wake.notify_all();
        for (auto &t : th) t.join();
    }
    void worker(int id) {
        int seen = 0;
        for (;;) {
            std::function<void(int)> f;
            {
                std::unique_lock<std::mutex> l(m);
                wake.wait(l, [&] { return quit || (generation != seen && id < want); });
                if (quit) return;
                seen = generation;
                f = job;
            }
            f(id);
            {
                std::lock_guard<std::mutex> l(m);
                if (--pending == 0) done.notify_all();
            }
        }
    }
    // f(t) for t = 0 .. count - 1, t = 0 on the calling thread; returns when all are through
    void run(int count, const std::function<void(int)> &f) {
        if (count <= 1) {
            f(0);
            return;
        }
        while ((int)th.size() < count - 1) {
            const int id = (int)th.size();
            th.emplace_back([this, id] { worker(id); });
        }
        {
            std::lock_guard<std::mutex> l(m);
            job = [&f](int id) { f(id + 1); };
            want = count - 1;
            pending = count - 1;
            generation++;
        }
        wake.notify_all();
        f(0);
        std::unique_lock<std::mutex> l(m);
        done.wait(l, [&] { return pending == 0; });
    }
};

// TRACK LOUDNESS: the request that holds for the whole-file calls that follow (opusgpu_set_loudness), and what the last of them
// measured and applied (opusgpu_last_loudness).  One per context of either kind.
struct LoudnessState {
    opusgpu_loudness_req req{}; // mode 0: off
    std::vector<opusgpu_loudness> records;
    std::vector<double> gains;
};

// FEATURE BATCHES: the request that holds for the whole-file feature calls that follow (opusgpu_set_feature_batch), with its own
// copies of the AFFINE vectors.  One per context of either kind.
struct FeatBatchState {
    opusgpu_feat_batch_req req{}; // enabled 0: off
    std::vector<float> sub, mul;
};

// WAVE BATCHES: the request that holds for the whole-file calls that follow (opusgpu_set_wave_batch), and the records of the last
// of them that ran the stage (opusgpu_last_wave_stats).  One per context of either kind.
struct WaveBatchState {
    opusgpu_wave_batch_req req{}; // enabled 0: off
    std::vector<opusgpu_wave_stat> records;
};

// WAVE TRIM: the request that holds for the whole-file calls that follow (opusgpu_set_wave_trim), and the records and activity flags
// of the last of them that ran the stage (opusgpu_last_wave_trim, opusgpu_last_wave_trim_flags).  One per context of either kind.
struct WaveTrimState {
    opusgpu_wave_trim_req req{}; // enabled 0: off
    std::vector<opusgpu_wave_trim_stat> records;
    std::vector<uint8_t> flags;
};

// STFT BATCHES: the request that holds for the whole-file STFT calls that follow (opusgpu_set_stft_batch), with its own copies of
// the AFFINE vectors.  One per context of either kind.
struct StftBatchState {
    opusgpu_stft_batch_req req{}; // enabled 0: off
    std::vector<float> sub, mul;
};

struct opusgpu_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    og::StreamState *d_streams = nullptr;
    int n_streams = 0, channels = 0;
    // staging for the host-buffer path
    void *d_descs = nullptr, *d_arena = nullptr, *d_pcm = nullptr, *d_result = nullptr;
    size_t cap_descs = 0, cap_arena = 0, cap_pcm = 0, cap_result = 0;
    // pinned host landing zone of the host-buffer path's PCM and result codes (DMA at full PCIe rate, no zero-filling of
    // a fresh temporary per call); the caller's pageable buffer is filled from it by a few host threads
    void *h_pcm = nullptr, *h_res = nullptr;
    size_t cap_h_pcm = 0, cap_h_res = 0;
    // ... and of the way in: the call's packet bytes and step table are gathered in page-locked memory that lives as long as the
    // context (a fresh 10 MB allocation per call is 2,600 page faults in front of the first upload, and a copy from pageable
    // memory holds the calling thread until the runtime has staged it)
    void *h_arena = nullptr, *h_descs = nullptr;
    size_t cap_h_arena = 0, cap_h_descs = 0;
    HostPool pool;
    uint32_t *d_crc_tables = nullptr; // 8 x 256 words, made on first use (opusgpu_pages_crc_device)
    hipEvent_t ev_piece[OPUSGPU_COPY_PIECES] = {}; // one per piece of the PCM's way back to the host (opusgpu_decode_packets)
    // large batches on the host-buffer path run in parts: a part's PCM travels back (on a stream of its own) while the next
    // part's kernels run
    hipStream_t copy_stream = nullptr;
    std::mutex registered_mutex;
    std::vector<std::pair<uintptr_t, size_t>> registered; // host ranges page-locked through opusgpu_host_register
    hipEvent_t ev_part[OPUSGPU_COPY_PIECES] = {};
    int host_parts = 8; // OPUSGPU_HOST_PARTS=1: one batch, copy after the kernels (A/B measurements); 2, 4, 8, 16
    // parse records of the split CELT path (one per frame of a step), grown on demand
    // (five sets: pipelined CELT-only steps rotate through 0 - 2 -- in-order steps use 0 --, pipelined SILK-only / hybrid steps
    // alternate 3 and 4: steps of the two kinds may be in flight together, OPUSGPU_STEP_KEEPS_MODE)
    void *d_recs[6] = {}, *d_rout[6] = {}; // (sets 0 - 2: pipelined CELT-only steps and everything in order; 3 - 5: pipelined SILK / hybrid steps)
    size_t cap_recs[6] = {}, cap_rout[6] = {};
    // (OG_SILK_SETS sets: pipelined SILK / hybrid steps rotate; everything else uses set 0.  Three since round 5: with two the parse
    // of step k + 1 had to wait for the synthesis of step k - 1 to let go of its set, and the chain parse -> parameters of a small
    // step -- 0.58 + 0.45 ms at 65,536 SILK-NB frames -- was then longer than the synthesis it should have hidden under)
    void *d_handoff[OG_SILK_SETS] = {}, *d_srecs[OG_SILK_SETS] = {};
    size_t cap_handoff[OG_SILK_SETS] = {}, cap_srecs[OG_SILK_SETS] = {};
    const void *last_srecs = nullptr; // the SILK records of the last step (opusgpu_debug_stage_taps)
    // Pipelined SILK-only steps (a step the caller declares SILK-only): the parse kernel keeps what its next run needs of the past
    // in d_shadow (SilkShadow per stream, og_silk_parse.hpp) and runs for step k + 1 on parse_stream next to step k's synthesis.
    void *d_shadow = nullptr;
    StepPipeline sp; // everything that orders the kernels of decode steps (og_step.hpp)
    int split_celt = 1;   // OPUSGPU_SPLIT=0 forces the single-kernel path for every mode (A/B measurements)
    int split_hybrid = 1; // OPUSGPU_SPLIT_HYBRID=0 keeps SILK-only and hybrid frames entirely on the single-kernel path
    int fast_recon = 1;   // OPUSGPU_FAST_RECON=0: every CELT frame through the general reconstruction kernel (A/B measurements)
    bool recon_fb_took_rest = false; // the last launch_celt_recon_fb also finished the frames without leaves: launch_celt_recon has nothing to launch
    int mode = OPUSGPU_MODE_REFERENCE; // opusgpu_set_mode
    int pipeline = 0;               // opusgpu_set_pipeline: declared steps run ahead of the step before them (og_step.hpp)
    long long stall_ticks = 0;      // OPUSGPU_STALL_US in ticks of the device wall clock (0: no stalls, og_debug.hpp)
    const void *last_recs = nullptr;
    // (OPUSGPU_PARSE_GROUPS) groups of frames per workgroup of the early parse, one after the other.  Round 2 measured two as the
    // best (half as many parse workgroups resident for twice as long: 2.545 / 2.50 / 2.52 / 2.97 ms per step at 1 / 2 / 3 / 4).  Round 4:
    // a group takes a parse wave 0.85 ms, so two groups are a chain of 1.7 ms -- which had become the step (a reconstruction doing
    // 40 % of its work: still 1.69 ms).  With one group the parse is done after 1.0 ms of the step and what counts is how many of the
    // reconstruction's waves fit a CU next to it: the parse kernel's LDS went from 46 KB to 36 KB per 128 frames for that
    // (og_celt_parse.hpp: ParseLds), 1.83 -> 1.74 ms.
    int parse_groups = 1;
    // the last decode step's tables, for opusgpu_debug_stage_taps
    const void *last_descs = nullptr;
    int last_n = 0, last_had_silk_recs = 0;
    // RFC mode, host side of the loss path: per stream, the frame count and descriptor flags of the last packet framed by
    // opusgpu_decode_packets -- what a lost packet of that stream is concealed as (0 frames: nothing framed yet)
    std::vector<int32_t> last_count, last_flags;
    LoudnessState loud;
    FeatBatchState fbatch;
    WaveBatchState wave;
    WaveTrimState trim;
    StftBatchState sbatch;
    char err[256] = {0};
};

static int fail(opusgpu_ctx *ctx, int code, const char *what, hipError_t e) {
    if (ctx) snprintf(ctx->err, sizeof(ctx->err), "%s: %s", what, hipGetErrorString(e));
    return code;
}
#define HIPCHK(ctx, call)                                                \
    do {                                                                 \
        hipError_t e_ = (call);                                          \
        if (e_ != hipSuccess) return fail(ctx, OPUSGPU_ERR_HIP, #call, e_); \
    } while (0)
static int grow(opusgpu_ctx *ctx, void **p, size_t *cap, size_t need); // (og_api.hip: device memory that only grows)
