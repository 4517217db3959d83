// og_tracks_tail.hpp -- zeroed tails (include/opusgpu.h, WHOLE FILES / CUTS): what lies between a track's final length and the stride
// of a strided batch is set to zero, so the track buffer is a tensor.  Included by og_api.hip behind og_tracks.hpp, whose
// files_run_tails calls batch_fill_tails behind the last step of a strided batch.
#pragma once

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_fill_tail: a range is the tail of one track (interleaved) or of one plane of it (planar), a run of elements of the track
// buffer.  blockIdx.y walks the ranges, blockIdx.x and the lanes the aligned 16-byte pieces of the buffer that a range touches, as
// k_tracks_assemble splits its work: a lane owns a piece and stores it whole -- a wave 1 KB of contiguous track per instruction,
// eight 128-byte lines --, and only the first and the last piece of a range, where it covers them in part, go out as element stores,
// so a neighbour's samples are never touched.  Nothing is read but the span; no LDS.
struct TailSpan {
    long long track_offset, plane_samples, first, end;
};
static_assert(sizeof(opusgpu_tail_span) == sizeof(TailSpan) && sizeof(TailSpan) == 32, "tail span layout");
static_assert(sizeof(opusgpu_cut) == 24 && sizeof(opusgpu_cut_info) == 24, "cut layout");

__global__ void __launch_bounds__(64) k_tracks_fill_tail(const TailSpan *__restrict__ spans, int n_ranges, int planes, int channels,
                                                         int wide, char *__restrict__ tracks) {
    const int sh = wide ? 2 : 1; // log2 of the element size: float32 or int16
    for (int r = (int)blockIdx.y; r < n_ranges; r += (int)gridDim.y) {
        const int t = r / planes, c = r - t * planes;
        const TailSpan sp = spans[t];
        // the range in elements of the buffer
        const long long e0 = planes > 1 ? sp.track_offset * channels + c * sp.plane_samples + sp.first : (sp.track_offset + sp.first) * channels;
        const long long en = planes > 1 ? sp.end - sp.first : (sp.end - sp.first) * channels;
        if (en <= 0) continue;
        const long long B0 = e0 << sh, B1 = (e0 + en) << sh; // and in bytes
        const long long c0 = B0 >> 4, pieces = ((B1 - 1) >> 4) - c0 + 1;
        for (long long q = (long long)blockIdx.x * 64 + threadIdx.x; q < pieces; q += (long long)gridDim.x * 64) {
            const long long d = (c0 + q) << 4;
            if (d >= B0 && d + 16 <= B1) {
                *reinterpret_cast<uint4 *>(tracks + d) = make_uint4(0, 0, 0, 0);
            } else if (wide) {
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (d + 4 * h >= B0 && d + 4 * h < B1) *reinterpret_cast<u32 *>(tracks + d + 4 * h) = 0;
            } else {
#pragma unroll
                for (int h = 0; h < 8; h++)
                    if (d + 2 * h >= B0 && d + 2 * h < B1) *reinterpret_cast<uint16_t *>(tracks + d + 2 * h) = 0;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------
// The kernel over n tracks: checks the spans, uploads them, launches on `s` and waits.
static int tracks_fill_tail_run(int device, hipStream_t s, int n_tracks, const opusgpu_tail_span *spans, int format, int channels,
                                void *d_tracks, const TrackFail &hip_failed) {
    if (format != OPUSGPU_TRACKS_S16 && format != OPUSGPU_TRACKS_F32 && format != OPUSGPU_TRACKS_F32_PLANAR) return OPUSGPU_BAD_ARG;
    if (channels < 1 || channels > 8 || n_tracks < 0 || (n_tracks && !spans)) return OPUSGPU_BAD_ARG;
    const bool planar = format == OPUSGPU_TRACKS_F32_PLANAR && channels > 1;
    const int esize = format == OPUSGPU_TRACKS_S16 ? 2 : 4;
    const int64_t most = INT64_MAX / 256; // every byte offset stays an int64
    int64_t longest = 0;                  // bytes of the longest range
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_tail_span &sp = spans[t];
        if (sp.track_offset < 0 || sp.track_offset > most || sp.first < 0 || sp.end < sp.first || sp.end > most) return OPUSGPU_BAD_ARG;
        if (planar && (sp.plane_samples < sp.end || sp.plane_samples > most)) return OPUSGPU_BAD_ARG;
        longest = std::max(longest, (sp.end - sp.first) * (planar ? 1 : channels) * esize);
    }
    if (!longest) return OPUSGPU_OK;
    if (!d_tracks || ((uintptr_t)d_tracks & 127)) return OPUSGPU_BAD_ARG;
    const int64_t n_ranges = (int64_t)n_tracks * (planar ? channels : 1);
    if (n_ranges > 0x7fffffff) return OPUSGPU_BAD_ARG;
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans;
    TRK_CHK(d_spans.upload(spans, (size_t)n_tracks * sizeof(TailSpan)));
    // a wave per 8 KB of the longest range: 8 pieces a lane there, fewer in every other range
    const int64_t gx = std::min<int64_t>((longest / 16 + 2 + 511) / 512, 1024);
    hipLaunchKernelGGL(k_tracks_fill_tail, dim3((unsigned)gx, (unsigned)std::min<int64_t>(n_ranges, 65535)), dim3(64), 0, s,
                       (const TailSpan *)d_spans.p, (int)n_ranges, planar ? channels : 1, channels, esize == 4 ? 1 : 0, (char *)d_tracks);
    TRK_CHK(hipGetLastError());
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// A strided batch whose tracks have been decoded: every track from its final length to the stride.
static int batch_fill_tails(const og_batch &b, int device, hipStream_t s, int format, const int64_t *final_lengths, void *d_tracks,
                            const TrackFail &hip_failed) {
    std::vector<opusgpu_tail_span> spans((size_t)b.n_files);
    for (size_t i = 0; i < spans.size(); i++) spans[i] = opusgpu_tail_span{b.info[i].track_offset, b.track_stride, final_lengths[i], b.track_stride};
    return tracks_fill_tail_run(device, s, b.n_files, spans.data(), format, b.channels, d_tracks, hip_failed);
}

extern "C" int opusgpu_tracks_fill_tail_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_tail_span *spans, int format, int channels,
                                               void *d_tracks, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_fill_tail_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, format, channels, d_tracks,
                                track_fail(ctx));
}
