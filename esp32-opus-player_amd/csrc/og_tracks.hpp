// og_tracks.hpp -- whole files (include/opusgpu.h, WHOLE FILES): the track assembly kernel and what the driver of a planned batch
// (og_files_run.hpp) needs of a context.  Included at the end of og_api.hip, whose contexts (og_ctx.hpp) and decode_step_impl
// (og_step.hpp) it uses.
#pragma once

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

// ---- host side ----------------------------------------------------------------------------------------
static int tracks_assemble_launch(opusgpu_ctx *ctx, hipStream_t s, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                  const void *d_result, void *d_tracks, void *d_track_state) {
    hipLaunchKernelGGL(k_tracks_assemble, dim3((unsigned)n_segs), dim3(256), 0, s, (const TrackSeg *)d_segs, (const i16 *)d_pcm, row_samples,
                       ctx->channels, (const i32 *)d_result, (i16 *)d_tracks, (TrackState *)d_track_state);
    HIPCHK(ctx, hipGetLastError());
    return OPUSGPU_OK;
}

extern "C" {

int opusgpu_tracks_assemble_device(opusgpu_ctx *ctx, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                   const void *d_result, void *d_tracks, void *d_track_state, void *hip_stream) {
    if (!ctx || n_segs < 0 || (ctx->channels != 1 && ctx->channels != 2)) return OPUSGPU_BAD_ARG;
    if (n_segs == 0) return OPUSGPU_OK;
    if (!d_segs || !d_pcm || !d_result || !d_tracks || !d_track_state || row_samples <= 0 || ((uintptr_t)d_pcm & 15) ||
        ((uintptr_t)d_tracks & 127) || ((uintptr_t)d_segs & 7) || ((size_t)row_samples * ctx->channels * 2) % 16)
        return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return tracks_assemble_launch(ctx, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_segs, d_segs, d_pcm, row_samples, d_result,
                                  d_tracks, d_track_state);
}

int opusgpu_files_decode(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, void *d_tracks, int64_t *track_lengths_out,
                         int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    if (!ctx->d_streams || ctx->n_streams < batch->n_files || ctx->channels != batch->channels || ctx->mode != batch->mode)
        return OPUSGPU_BAD_ARG;
    const int row = batch->mode == OPUSGPU_MODE_RFC ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES;
    FilesRunOps ops;
    ops.device = ctx->device;
    ops.extra_slot_bytes[0] = (size_t)row * batch->channels * 2, ops.extra_slot_bytes[1] = sizeof(int32_t); // PCM rows, result codes
    ops.reset = [&](int n_files) { return opusgpu_streams_reset(ctx, 0, n_files, 1); };
    ops.step = [&](int, int n, const void *d_descs, const void *d_arena, int modes, void *const *x) {
        return decode_step_impl(ctx, n, d_descs, d_arena, x[0], x[1], nullptr, true, modes);
    };
    ops.assemble = [&](int, int n, const void *d_segs, void *const *x, void *d_state) {
        return tracks_assemble_launch(ctx, ctx->stream, n, d_segs, x[0], row, x[1], d_tracks, d_state);
    };
    ops.drain = [&] {
        (void)sync_in_flight(ctx);
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        return e == hipSuccess ? (int)OPUSGPU_OK : fail(ctx, OPUSGPU_ERR_HIP, "hipStreamSynchronize(files)", e);
    };
    ops.hip_failed = [&](int code, const char *what, hipError_t e) { return fail(ctx, code, what, e); };
    return files_run(*batch, ops, d_tracks, track_lengths_out, status_out);
}

} // extern "C"
