// og_tracks.hpp -- whole files (include/opusgpu.h, WHOLE FILES): the track assembly kernel and what the driver of a planned batch
// (og_files_run.hpp) needs of a context.  Included at the end of og_api.hip, whose contexts (og_ctx.hpp) and decode_step_impl
// (og_step.hpp) it uses.
#pragma once
#include <cmath>

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_assemble: one workgroup per segment.  The work is split by DESTINATION: lane q of the workgroup owns the q-th aligned
// 16-byte piece of the track buffer that the segment touches and stores it whole (a wave: 1 KB of contiguous track per
// instruction); only the segment's first and last piece, where it covers them in part, go out as 16-bit stores.  The source is
// not aligned to the destination -- a pre-skip of 312 shifts a stereo track by 1,248 bytes, a mono one by any even count -- so a
// lane fetches the two aligned 16-byte pieces of the PCM row that hold its 16 bytes and shifts them together in registers: the
// shift is a whole number of 16-bit samples, the same for every piece of a segment (selects on a wave-uniform value, no indexed
// registers: no scratch).  Pieces of the row that hold no byte of the segment are not fetched: nothing outside the row is read.
struct TrackSeg {
    i32 slot, src_first, count, track;
    long long dst_first;
    i32 packet_seq, reserved;
};
struct TrackState {
    i32 first_bad, code;
};
static_assert(sizeof(opusgpu_track_seg) == sizeof(TrackSeg) && sizeof(TrackSeg) == 32, "segment layout");
static_assert(sizeof(opusgpu_track_state) == sizeof(TrackState) && sizeof(TrackState) == 8, "track state layout");
static_assert(sizeof(opusgpu_file_info) == 48, "file info layout");

__global__ void __launch_bounds__(256) k_tracks_assemble(const TrackSeg *__restrict__ segs, const i16 *__restrict__ pcm, int row_samples,
                                                          int channels, const i32 *__restrict__ result, i16 *__restrict__ tracks,
                                                          TrackState *__restrict__ state) {
    const TrackSeg sg = segs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    const i32 res = result[sg.slot];
    if (res < 0) { // a failed frame: nothing is written, the track ends at its packet
        if (tid == 0) {
            const i32 old = atomicMin(&state[sg.track].first_bad, sg.packet_seq);
            if (sg.packet_seq < old) state[sg.track].code = res;
        }
        return;
    }
    if (sg.packet_seq >= state[sg.track].first_bad) return;
    if (sg.count <= 0 || sg.src_first < 0 || sg.src_first + sg.count > row_samples) return;
    const long long unit = 2 * channels; // bytes per sample of every channel
    const long long S0 = ((long long)sg.slot * row_samples + sg.src_first) * unit, D0 = sg.dst_first * unit, B = sg.count * unit;
    const long long c0 = D0 >> 4;
    const int pieces = (int)(((D0 + B - 1) >> 4) - c0) + 1;
    const char *src = reinterpret_cast<const char *>(pcm);
    char *dst = reinterpret_cast<char *>(tracks);
    for (int q = tid; q < pieces; q += 256) {
        const long long d = (c0 + q) << 4;  // the piece's place in the track buffer
        const long long s = S0 + (d - D0);  // where its first byte comes from (before the segment for a partial first piece)
        const long long p0 = s & ~15LL;
        const int sh = (int)(s - p0); // 0, 2 .. 14
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (p0 + 16 > S0 && p0 < S0 + B) a = *reinterpret_cast<const uint4 *>(src + p0);
        if (sh && p0 + 32 > S0 && p0 + 16 < S0 + B) b = *reinterpret_cast<const uint4 *>(src + p0 + 16);
        const u32 W[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        const int w = sh >> 2;
        const bool half = (sh & 2) != 0;
        u32 v[5], r[4];
#pragma unroll
        for (int i = 0; i < 5; i++) v[i] = w == 0 ? W[i] : w == 1 ? W[i + 1] : w == 2 ? W[i + 2] : W[(i + 3) & 7];
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = half ? (v[i] >> 16) | (v[i + 1] << 16) : v[i];
        if (d >= D0 && d + 16 <= D0 + B) {
            *reinterpret_cast<uint4 *>(dst + d) = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int h = 0; h < 8; h++) {
                const long long at = d + 2 * h;
                if (at >= D0 && at < D0 + B) *reinterpret_cast<uint16_t *>(dst + at) = (uint16_t)(r[h >> 1] >> (16 * (h & 1)));
            }
        }
    }
}

// ---- float tracks (OPUSGPU_TRACKS_F32, OPUSGPU_TRACKS_F32_PLANAR) ---------------------------------------
// The same pass with the consumer's format as its store: every sample leaves as (float)s * scale[track], one IEEE multiply, where
// k_tracks_assemble stores s.  2 bytes in and 4 bytes out per sample; the S16 kernel above is not touched.
struct TrackPlace {
    long long track_offset, plane_samples;
    float scale;
    i32 reserved;
};
static_assert(sizeof(opusgpu_track_place) == sizeof(TrackPlace) && sizeof(TrackPlace) == 24, "track place layout");

// k_tracks_assemble's protocol for a segment whose frame's result is `res`: true when the segment is to be copied
__device__ __forceinline__ bool track_seg_kept(const TrackSeg &sg, i32 res, int tid, int row_samples, TrackState *__restrict__ state) {
    if (res < 0) { // a failed frame: nothing is written, the track ends at its packet
        if (tid == 0) {
            const i32 old = atomicMin(&state[sg.track].first_bad, sg.packet_seq);
            if (sg.packet_seq < old) state[sg.track].code = res;
        }
        return false;
    }
    if (sg.packet_seq >= state[sg.track].first_bad) return false;
    return sg.count > 0 && sg.src_first >= 0 && sg.src_first + sg.count <= row_samples;
}
__device__ __forceinline__ float track_f32(u32 s16, float k) { return __fmul_rn((float)(i16)s16, k); } // never contracted
// A whole 16-byte piece, as ONE vector store: a float4 assigned through its struct is four scalar stores to the optimiser, which
// then shares the last of them with the partial path's and leaves 12 + 4 bytes.
typedef float og_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void track_store4(float *d, const float f[4]) { *reinterpret_cast<og_f32x4 *>(d) = og_f32x4{f[0], f[1], f[2], f[3]}; }

// k_tracks_assemble_f32: interleaved float tracks of a mono or stereo context (and the planar tracks of a mono one: a mono track IS
// its plane).  Split by DESTINATION as above: lane q owns the q-th aligned 16-byte piece of the track buffer that the segment
// touches -- 4 floats, which come from 8 bytes of the PCM row at any 2-byte alignment -- and stores it whole; the first and last
// piece, where covered in part, go out as 32-bit stores.  The 8 bytes lie in one aligned 16-byte piece of the row or in two (shift
// above 8); the shift is the same for every piece of a segment.  Pieces of the row without a byte of the segment are not fetched.
__global__ void __launch_bounds__(256) k_tracks_assemble_f32(const TrackSeg *__restrict__ segs, const i16 *__restrict__ pcm, int row_samples,
                                                              int channels, const i32 *__restrict__ result,
                                                              const TrackPlace *__restrict__ place, float *__restrict__ tracks,
                                                              TrackState *__restrict__ state) {
    const TrackSeg sg = segs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    if (!track_seg_kept(sg, result[sg.slot], tid, row_samples, state)) return;
    const float k = place[sg.track].scale;
    const long long E0 = sg.dst_first * channels, EN = (long long)sg.count * channels; // the segment in elements of the track buffer
    const long long S0 = ((long long)sg.slot * row_samples + sg.src_first) * channels * 2, B = EN * 2; // and in bytes of the PCM
    const long long c0 = E0 >> 2;
    const int pieces = (int)(((E0 + EN - 1) >> 2) - c0) + 1;
    const char *src = reinterpret_cast<const char *>(pcm);
    for (int q = tid; q < pieces; q += 256) {
        const long long e = (c0 + q) << 2;      // the piece's first element
        const long long s = S0 + (e - E0) * 2;  // where its first sample comes from (before the segment for a partial first piece)
        const long long p0 = s & ~15LL;
        const int sh = (int)(s - p0); // 0, 2 .. 14
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (p0 + 16 > S0 && p0 < S0 + B) a = *reinterpret_cast<const uint4 *>(src + p0);
        if (sh > 8 && p0 + 32 > S0 && p0 + 16 < S0 + B) b = *reinterpret_cast<const uint4 *>(src + p0 + 16);
        const u32 W[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        const int w = sh >> 2;
        const bool half = (sh & 2) != 0;
        u32 v[3], r[2];
#pragma unroll
        for (int i = 0; i < 3; i++) v[i] = w == 0 ? W[i] : w == 1 ? W[i + 1] : w == 2 ? W[i + 2] : W[i + 3];
#pragma unroll
        for (int i = 0; i < 2; i++) r[i] = half ? (v[i] >> 16) | (v[i + 1] << 16) : v[i];
        const float f[4] = {track_f32(r[0], k), track_f32(r[0] >> 16, k), track_f32(r[1], k), track_f32(r[1] >> 16, k)};
        if (e >= E0 && e + 4 <= E0 + EN) {
            track_store4(tracks + e, f);
        } else {
#pragma unroll
            for (int h = 0; h < 4; h++)
                if (e + h >= E0 && e + h < E0 + EN) tracks[e + h] = f[h];
        }
    }
}

// k_tracks_assemble_f32_planar2: planar float tracks of a stereo context.  Lane q owns the q-th aligned group of 4 samples of the
// track that the segment touches: 4 L/R pairs, 16 bytes of the PCM row at a 4-byte alignment (two aligned pieces and a shift of
// whole pairs, as above), and one 16-byte store into each plane.  Both planes of a track begin on a 256-byte boundary (offset and
// plane length are multiples of 64), so one cut serves both; the first and last group, where covered in part, go out as 32-bit
// stores.
__global__ void __launch_bounds__(256) k_tracks_assemble_f32_planar2(const TrackSeg *__restrict__ segs, const i16 *__restrict__ pcm,
                                                                      int row_samples, const i32 *__restrict__ result,
                                                                      const TrackPlace *__restrict__ place, float *__restrict__ tracks,
                                                                      TrackState *__restrict__ state) {
    const TrackSeg sg = segs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    if (!track_seg_kept(sg, result[sg.slot], tid, row_samples, state)) return;
    const TrackPlace pl = place[sg.track];
    const float k = pl.scale;
    float *const left = tracks + 2 * pl.track_offset, *const right = left + pl.plane_samples;
    const long long N0 = sg.dst_first - pl.track_offset; // the segment's first sample in its track
    const long long S0 = ((long long)sg.slot * row_samples + sg.src_first) * 4, B = (long long)sg.count * 4;
    const long long c0 = N0 >> 2;
    const int pieces = (int)(((N0 + sg.count - 1) >> 2) - c0) + 1;
    const char *src = reinterpret_cast<const char *>(pcm);
    for (int q = tid; q < pieces; q += 256) {
        const long long n = (c0 + q) << 2;
        const long long s = S0 + (n - N0) * 4;
        const long long p0 = s & ~15LL;
        const int w = (int)(s - p0) >> 2; // 0 .. 3 pairs
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (p0 + 16 > S0 && p0 < S0 + B) a = *reinterpret_cast<const uint4 *>(src + p0);
        if (w && p0 + 32 > S0 && p0 + 16 < S0 + B) b = *reinterpret_cast<const uint4 *>(src + p0 + 16);
        const u32 W[7] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z};
        float l[4], r[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const u32 v = w == 0 ? W[i] : w == 1 ? W[i + 1] : w == 2 ? W[i + 2] : W[i + 3];
            l[i] = track_f32(v, k), r[i] = track_f32(v >> 16, k);
        }
        if (n >= N0 && n + 4 <= N0 + sg.count) {
            track_store4(left + n, l);
            track_store4(right + n, r);
        } else {
#pragma unroll
            for (int h = 0; h < 4; h++)
                if (n + h >= N0 && n + h < N0 + sg.count) left[n + h] = l[h], right[n + h] = r[h];
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------
static int tracks_assemble_launch(opusgpu_ctx *ctx, hipStream_t s, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                  const void *d_result, void *d_tracks, void *d_track_state) {
    hipLaunchKernelGGL(k_tracks_assemble, dim3((unsigned)n_segs), dim3(256), 0, s, (const TrackSeg *)d_segs, (const i16 *)d_pcm, row_samples,
                       ctx->channels, (const i32 *)d_result, (i16 *)d_tracks, (TrackState *)d_track_state);
    HIPCHK(ctx, hipGetLastError());
    return OPUSGPU_OK;
}
static int tracks_assemble_f32_launch(opusgpu_ctx *ctx, hipStream_t s, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                      const void *d_result, int format, const void *d_place, void *d_tracks, void *d_track_state) {
    if (format == OPUSGPU_TRACKS_F32_PLANAR && ctx->channels == 2)
        hipLaunchKernelGGL(k_tracks_assemble_f32_planar2, dim3((unsigned)n_segs), dim3(256), 0, s, (const TrackSeg *)d_segs, (const i16 *)d_pcm,
                           row_samples, (const i32 *)d_result, (const TrackPlace *)d_place, (float *)d_tracks, (TrackState *)d_track_state);
    else
        hipLaunchKernelGGL(k_tracks_assemble_f32, dim3((unsigned)n_segs), dim3(256), 0, s, (const TrackSeg *)d_segs, (const i16 *)d_pcm,
                           row_samples, ctx->channels, (const i32 *)d_result, (const TrackPlace *)d_place, (float *)d_tracks,
                           (TrackState *)d_track_state);
    HIPCHK(ctx, hipGetLastError());
    return OPUSGPU_OK;
}

// The place table of a batch for a float format: where every track and its planes lie, and its scale (NULL: 1 / 32768 each).
// OPUSGPU_BAD_ARG for a format that does not exist, a scale with OPUSGPU_TRACKS_S16, a scale entry that is not finite.
static int track_places(const og_batch &b, int format, const float *scale, std::vector<TrackPlace> &places) {
    if (format != OPUSGPU_TRACKS_S16 && format != OPUSGPU_TRACKS_F32 && format != OPUSGPU_TRACKS_F32_PLANAR) return OPUSGPU_BAD_ARG;
    if (format == OPUSGPU_TRACKS_S16) return scale ? OPUSGPU_BAD_ARG : OPUSGPU_OK;
    places.resize((size_t)b.n_files);
    for (int i = 0; i < b.n_files; i++) {
        const float k = scale ? scale[i] : 1.0f / 32768;
        if (!std::isfinite(k)) return OPUSGPU_BAD_ARG;
        // a track's planes lie its planned length, rounded up to 64, apart; those of a strided batch (WHOLE FILES / CUTS) its stride
        places[i] = TrackPlace{b.info[i].track_offset, b.track_stride ? b.track_stride : (b.info[i].track_samples + 63) / 64 * 64, k, 0};
    }
    return OPUSGPU_OK;
}
// What the host side of every track header shares.
// A HIP call inside a function that has a `hip_failed(code, what, e)` in reach: a failure leaves through it.
#define TRK_CHK(call)                                                             \
    do {                                                                          \
        const hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) return hip_failed(OPUSGPU_ERR_HIP, #call, e_);      \
    } while (0)
// hip_failed: keeps the message of the object the call belongs to and returns `code`.
typedef std::function<int(int code, const char *what, hipError_t e)> TrackFail;
static TrackFail track_fail(opusgpu_ctx *ctx) {
    return [ctx](int code, const char *what, hipError_t e) { return fail(ctx, code, what, e); };
}
// A device buffer for the length of one call: freed on every way out.
struct RsDevBuf {
    void *p = nullptr;
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes + 16); }
    hipError_t upload(const void *src, size_t bytes) {
        const hipError_t e = alloc(bytes);
        return e != hipSuccess || !bytes ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    }
    ~RsDevBuf() {
        if (p) (void)hipFree(p);
    }
};

// files_run, and behind it the zeroed tails of a strided batch (og_tracks_tail.hpp: first = the final length, end = the stride), on
// the stream `s` the steps ran on.  A packed batch is files_run alone: nothing new is queued.
static int batch_fill_tails(const og_batch &b, int device, hipStream_t s, int format, const int64_t *final_lengths, void *d_tracks,
                            const TrackFail &hip_failed);
static int files_run_tails(const og_batch &b, const FilesRunOps &ops, hipStream_t s, int format, void *d_tracks, int64_t *track_lengths_out,
                           int32_t *status_out) {
    if (!b.track_stride) return files_run(b, ops, d_tracks, track_lengths_out, status_out);
    std::vector<int64_t> lengths((size_t)b.n_files, 0);
    if (int rc = files_run(b, ops, d_tracks, lengths.data(), status_out)) return rc;
    if (int rc = batch_fill_tails(b, ops.device, s, format, lengths.data(), d_tracks, ops.hip_failed)) return rc;
    if (track_lengths_out) std::copy(lengths.begin(), lengths.end(), track_lengths_out);
    return OPUSGPU_OK;
}
// What a whole-file call that ends in another kernel answers for a strided batch: its output has a grid of its own.
#define OG_STRIDE_REFUSED                                                                                                    \
    "the batch has a track stride, which only the tracks at 48 kHz of opusgpu_files_decode and opusgpu_files_decode_as keep: " \
    "resampled, mixed and feature outputs have grids of their own -- plan the cuts with track_stride 0 for these calls"

// opusgpu_files_decode and opusgpu_files_decode_as: `places` is null for int16 tracks, else the batch's table for `format`.
// Nothing of the driver depends on the format: the PCM rows and result codes the steps write are the same, and the float assembly
// is queued where the int16 one is -- on the steps' stream behind its step -- so one PCM buffer still serves any pipeline depth.
static int files_decode_run(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int format, const std::vector<TrackPlace> *places,
                            void *d_tracks, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    if (!ctx->d_streams || ctx->n_streams < batch->n_files || ctx->channels != batch->channels || ctx->mode != batch->mode)
        return OPUSGPU_BAD_ARG;
    RsDevBuf d_place; // the place table, for the length of this call
    if (places && !batch->segs.empty()) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, d_place.upload(places->data(), places->size() * sizeof(TrackPlace)));
    }
    const int row = batch->mode == OPUSGPU_MODE_RFC ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES;
    FilesRunOps ops;
    ops.device = ctx->device;
    ops.extra_slot_bytes[0] = (size_t)row * batch->channels * 2, ops.extra_slot_bytes[1] = sizeof(int32_t); // PCM rows, result codes
    ops.reset = [&](int n_files) { return opusgpu_streams_reset(ctx, 0, n_files, 1); };
    ops.step = [&](int, int n, const void *d_descs, const void *d_arena, int modes, void *const *x) {
        return decode_step_impl(ctx, n, d_descs, d_arena, x[0], x[1], nullptr, true, modes);
    };
    ops.assemble = [&](int, int n, const void *d_segs, void *const *x, void *d_state) {
        if (places) return tracks_assemble_f32_launch(ctx, ctx->stream, n, d_segs, x[0], row, x[1], format, d_place.p, d_tracks, d_state);
        return tracks_assemble_launch(ctx, ctx->stream, n, d_segs, x[0], row, x[1], d_tracks, d_state);
    };
    ops.drain = [&] {
        (void)sync_in_flight(ctx);
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        return e == hipSuccess ? (int)OPUSGPU_OK : fail(ctx, OPUSGPU_ERR_HIP, "hipStreamSynchronize(files)", e);
    };
    ops.hip_failed = track_fail(ctx);
    return files_run_tails(*batch, ops, ctx->stream, format, d_tracks, track_lengths_out, status_out);
}

// The owner of a whole-file call that ends in another kernel (TRACK RATES and all behind it): the batch, where its work runs, the
// decoder that turns the batch into scratch S16 tracks, and who keeps the message of a HIP error.  One maker per kind of decoder:
// here and in og_ms_tracks.hpp.
struct FilesOwner {
    const og_batch &b;
    int device;
    hipStream_t stream;
    std::function<int(void *d_s16, int64_t *lengths, int32_t *status)> decode;
    TrackFail hip_failed;
    LoudnessState *loud = nullptr; // TRACK LOUDNESS (og_tracks_loudness.hpp): the owner's request and what the call measures
    bool scale_later = false;      // the S16 tracks of this call feed a feature kernel, which applies the scale and a gain with it
    const FeatBatchState *fbatch = nullptr;  // FEATURE BATCHES (og_feat_batch.hpp): the owner's request, read by files_feature_run alone
    std::function<void(const char *why)> refused; // keeps the reason of a refusal where opusgpu_last_error finds it
    WaveBatchState *wave = nullptr; // WAVE BATCHES (og_wave_batch.hpp): the owner's request and records, read by files_resampled_to alone
    const StftBatchState *sbatch = nullptr; // STFT BATCHES (og_stft_batch.hpp): the owner's request, read by files_stft_run alone
    WaveTrimState *trim = nullptr; // WAVE TRIM (og_wave_trim.hpp): the owner's request, records and flags, read by files_resampled_to alone
};
static FilesOwner files_owner(opusgpu_ctx *ctx, const opusgpu_file_batch *batch) {
    return FilesOwner{*batch, ctx->device, ctx->stream,
                      [=](void *d_s16, int64_t *lengths, int32_t *status) {
                          if (batch->track_stride) {
                              snprintf(ctx->err, sizeof(ctx->err), "%s", OG_STRIDE_REFUSED);
                              return (int)OPUSGPU_BAD_ARG;
                          }
                          return files_decode_run(ctx, batch, OPUSGPU_TRACKS_S16, nullptr, d_s16, lengths, status);
                      },
                      track_fail(ctx), &ctx->loud, false, &ctx->fbatch,
                      [=](const char *why) { snprintf(ctx->err, sizeof(ctx->err), "%s", why); }, &ctx->wave, &ctx->sbatch, &ctx->trim};
}

// With a loudness request on, the int16 tracks of `run` are measured where the caller has them (og_tracks_loudness.hpp); without one
// this is run(track_lengths_out, status_out).
template <class Run>
static int files_decode_measured(const FilesOwner &own, void *d_tracks, int64_t *track_lengths_out, int32_t *status_out, Run run);
// What opusgpu_files_decode_as and its multistream twin answer for a float format while a request is on: the float store is fused
// into the assembly, so there is never an S16 track to measure.
#define OG_LOUD_AS_REFUSED                                                                                                       \
    "a loudness request is on and this call has no int16 track to measure: use the _mixed call at rate 48000 with the identity " \
    "matrix (16384 on the diagonal), which writes the same elements"

extern "C" {

int opusgpu_tracks_assemble_device_as(opusgpu_ctx *ctx, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                      const void *d_result, int format, const void *d_place, void *d_tracks, void *d_track_state,
                                      void *hip_stream) {
    const bool f32 = format == OPUSGPU_TRACKS_F32 || format == OPUSGPU_TRACKS_F32_PLANAR;
    if (!f32 && (format != OPUSGPU_TRACKS_S16 || d_place)) return OPUSGPU_BAD_ARG;
    if (!ctx || n_segs < 0 || (ctx->channels != 1 && ctx->channels != 2)) return OPUSGPU_BAD_ARG;
    if (n_segs == 0) return OPUSGPU_OK;
    if (!d_segs || !d_pcm || !d_result || !d_tracks || !d_track_state || row_samples <= 0 || ((uintptr_t)d_pcm & 15) ||
        ((uintptr_t)d_tracks & 127) || ((uintptr_t)d_segs & 7) || ((size_t)row_samples * ctx->channels * 2) % 16)
        return OPUSGPU_BAD_ARG;
    if (f32 && (!d_place || ((uintptr_t)d_place & 7))) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    if (f32) return tracks_assemble_f32_launch(ctx, s, n_segs, d_segs, d_pcm, row_samples, d_result, format, d_place, d_tracks, d_track_state);
    return tracks_assemble_launch(ctx, s, n_segs, d_segs, d_pcm, row_samples, d_result, d_tracks, d_track_state);
}

int opusgpu_tracks_assemble_device(opusgpu_ctx *ctx, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                   const void *d_result, void *d_tracks, void *d_track_state, void *hip_stream) {
    return opusgpu_tracks_assemble_device_as(ctx, n_segs, d_segs, d_pcm, row_samples, d_result, OPUSGPU_TRACKS_S16, nullptr, d_tracks,
                                             d_track_state, hip_stream);
}

int opusgpu_files_decode(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, void *d_tracks, int64_t *track_lengths_out,
                         int32_t *status_out) {
    if (!ctx || !batch || ctx->loud.req.mode == OPUSGPU_LOUDNESS_OFF)
        return files_decode_run(ctx, batch, OPUSGPU_TRACKS_S16, nullptr, d_tracks, track_lengths_out, status_out);
    return files_decode_measured(files_owner(ctx, batch), d_tracks, track_lengths_out, status_out, [&](int64_t *lengths, int32_t *status) {
        return files_decode_run(ctx, batch, OPUSGPU_TRACKS_S16, nullptr, d_tracks, lengths, status);
    });
}

int opusgpu_files_decode_as(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int format, const float *scale, void *d_tracks,
                            int64_t *track_lengths_out, int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    std::vector<TrackPlace> places;
    if (int rc = track_places(*batch, format, scale, places)) return rc;
    if (format == OPUSGPU_TRACKS_S16) return opusgpu_files_decode(ctx, batch, d_tracks, track_lengths_out, status_out);
    if (ctx->loud.req.mode != OPUSGPU_LOUDNESS_OFF) {
        snprintf(ctx->err, sizeof(ctx->err), "%s", OG_LOUD_AS_REFUSED);
        return OPUSGPU_BAD_ARG;
    }
    return files_decode_run(ctx, batch, format, &places, d_tracks, track_lengths_out, status_out);
}

} // extern "C"
