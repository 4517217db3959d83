// og_wave_batch.hpp -- waveform batches (include/opusgpu.h, WAVE BATCHES): the packed int16 tracks that a resampling kernel wrote,
// collated into one dense float32 tensor of n * S * C floats, every track normalised by exact integer statistics of its own real
// samples and padded to S samples, with an optional attention mask.  Included by og_api.hip behind og_feat_batch.hpp;
// files_resampled_to (og_tracks_resample.hpp) calls wave_batch_run behind its kernel when the owner holds a request.  DESIGN.md
// section 13l.
#pragma once

// ---- kernels ------------------------------------------------------------------------------------------
// A streaming stage over 2-byte samples: the tracks are read once for the statistics (ZMUV and PEAK) and once for the tensor, the
// tensor and the mask are written once.  Three kernels, all plain vector loads and stores:
//   k_wave_stats  a workgroup per (track, chunk of WBAT_CHUNK elements): aligned 16-byte pieces, eight a lane; sum, sum of squares
//                 and peak as integers, folded over the wave by a butterfly and added to the track's record by one integer atomic
//                 each -- exact, so the order of arrival changes no bit;
//   k_wave_fold   a lane per track: sub and mul in double from the three integers, V = N sumsq - sum^2 in 128 bits;
//   k_wave_batch  a lane owns an aligned 16-byte piece of the DESTINATION -- four floats of the tensor, or sixteen bytes of the mask.
constexpr int WBAT_CHUNK = 16384; // elements a workgroup of k_wave_stats takes: 256 lanes, 8 pieces of 8
struct WbatSpan {
    long long in_offset, samples;
    float scale;
    i32 reserved;
};
struct WbatTile {
    i32 track, chunk;
};
struct WbatStat { // opusgpu_wave_stat as the kernels see it
    long long count, sum;
    unsigned long long sumsq;
    double sub, mul;
    i32 peak, reserved;
};
struct WbatArgs {
    long long S;
    double eps, target;
    int C, planar, norm, mask;
    float pad_value;
};
static_assert(sizeof(opusgpu_wave_batch_req) == 64 && sizeof(opusgpu_wave_span) == 24 && sizeof(opusgpu_wave_stat) == 48, "wave batch records");
static_assert(sizeof(WbatSpan) == sizeof(opusgpu_wave_span) && sizeof(WbatStat) == sizeof(opusgpu_wave_stat), "wave batch records");

// The track's record starts as zeros (a memset on the stream in front of this kernel).
__global__ void __launch_bounds__(256) k_wave_stats(const WbatTile *__restrict__ tiles, const WbatSpan *__restrict__ spans,
                                                    const i16 *__restrict__ in, int C, WbatStat *__restrict__ stat) {
    const WbatTile tile = tiles[blockIdx.x];
    const WbatSpan sp = spans[tile.track];
    const long long N = sp.samples * C;                       // the track's real elements
    const long long first = (long long)tile.chunk * WBAT_CHUNK; // this chunk's first, a multiple of 8
    const int left = (int)(N - first < WBAT_CHUNK ? N - first : WBAT_CHUNK); // its elements, >= 1
    const i16 *src = in + sp.in_offset * C + first;           // 16-byte aligned: in_offset is a multiple of 8
    i32 s = 0, peak = 0; // a lane's 64 elements: |s| <= 2^21
    u64 q = 0;
#pragma unroll
    for (int k = 0; k < WBAT_CHUNK / (256 * 8); k++) {
        const int e = 8 * ((int)threadIdx.x + 256 * k);
        if (e < left) { // the piece holds a real element: nothing behind the track's last piece is read
            const uint4 v = *reinterpret_cast<const uint4 *>(src + e);
            const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const i32 a = e + 2 * h < left ? (i32)(i16)w[h] : 0, b = e + 2 * h + 1 < left ? (i32)(i16)(w[h] >> 16) : 0;
                s += a + b;
                // a pair of -32768 squares to 2^31: an unsigned word holds it, a signed dot product would not
                q += (u64)((u32)(a * a) + (u32)(b * b));
                const i32 ma = a < 0 ? -a : a, mb = b < 0 ? -b : b;
                peak = peak > ma ? peak : ma;
                peak = peak > mb ? peak : mb;
            }
        }
    }
    long long s64 = s;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        s64 += __shfl_xor(s64, d, 64);
        q += __shfl_xor(q, d, 64);
        const i32 o = __shfl_xor(peak, d, 64);
        peak = peak > o ? peak : o;
    }
    if (((int)threadIdx.x & 63) == 0) {
        WbatStat *r = stat + tile.track;
        atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum), (unsigned long long)s64); // two's complement: the signed sum
        atomicAdd(&r->sumsq, q);
        atomicMax(&r->peak, peak);
    }
}

// (double)v of a 128-bit unsigned integer below 2^93, in two roundings.
__device__ __forceinline__ double wbat_f64(unsigned __int128 v) { return (double)(u64)(v >> 64) * 18446744073709551616.0 + (double)(u64)v; }

__global__ void __launch_bounds__(64) k_wave_fold(const WbatSpan *__restrict__ spans, int n_tracks, WbatArgs A, WbatStat *__restrict__ stat) {
    const int t = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (t >= n_tracks) return;
    const WbatSpan sp = spans[t];
    WbatStat r = stat[t];
    const long long N = sp.samples * A.C;
    const double k = (double)sp.scale, n = (double)N;
    r.count = N;
    r.sub = 0.0;
    if (A.norm == OPUSGPU_WAVE_NORM_ZMUV) {
        double var = 0.0;
        if (N) {
            const unsigned long long a = (unsigned long long)(r.sum < 0 ? -r.sum : r.sum);
            const unsigned __int128 V = (unsigned __int128)(unsigned long long)N * r.sumsq - (unsigned __int128)a * a; // >= 0 (Cauchy-Schwarz)
            r.sub = k * ((double)r.sum / n); // sum / N first: exact for a constant track, whose cells are then exactly 0
            var = k * k * wbat_f64(V) / n / n;
        }
        r.mul = 1.0 / sqrt(var + A.eps);
    } else { // PEAK
        const double d = (double)r.peak * k; // exact: 16 x 24 bits
        r.mul = d != 0.0 ? A.target / d : 1.0;
    }
    stat[t] = r;
}

// A real cell: NONE is the float formats' own store, (float)y * scale; ZMUV and PEAK follow the record in double -- y * scale is
// exact there, so the fused subtraction is the rounded subtraction, then one rounded multiplication and one conversion.
__device__ __forceinline__ float wbat_cell(bool plain, u32 y, float k, double sub, double mul) {
    if (plain) return track_f32(y, k);
    return (float)__dmul_rn(__fma_rn((double)(i16)y, (double)k, -sub), mul);
}

// blockIdx.y walks the tracks, blockIdx.x and the lanes the aligned 16-byte pieces that a track's S * C floats touch and, behind
// them, those that its S mask bytes touch -- as k_feat_batch splits its work.  A piece that lies wholly inside the track goes out as
// one 16-byte store; a track's first and last piece, where a neighbour shares them or the tensor ends, as guarded 4-byte stores
// (1-byte stores in the mask) of this track's elements alone, so every element is written once.
// Interleaved, element i of a track is element i of its int16 source: the piece's four samples are 8 bytes at any 2-byte alignment
// against the 16-byte aligned track (t * S * C mod 4 is anything), fetched as the one or two aligned 16-byte source pieces that hold
// them and shifted together in registers, as k_tracks_assemble_f32 does; pieces without a real sample are not fetched.  Planar
// (C > 1), element i is (c, m) = (i / S, i % S) and comes from element m * C + c: four 2-byte loads C apart.
__global__ void __launch_bounds__(256) k_wave_batch(const WbatSpan *__restrict__ spans, int n_tracks, const i16 *__restrict__ in, WbatArgs A,
                                                    const WbatStat *__restrict__ stat, float *__restrict__ out, unsigned char *__restrict__ mask) {
    const u32 C = (u32)A.C, S = (u32)A.S, n = S * C; // S * C <= 0x7fffffff (wave_batch_run)
    const bool plain = A.norm == OPUSGPU_WAVE_NORM_NONE;
    for (int t = (int)blockIdx.y; t < n_tracks; t += (int)gridDim.y) {
        const WbatSpan sp = spans[t];
        const u32 L = (u32)sp.samples, N = L * C; // L <= S
        double sub = 0.0, mul = 1.0;
        if (!plain) sub = stat[t].sub, mul = stat[t].mul;
        const float k = sp.scale;
        const i16 *src = in + sp.in_offset * C;                         // 16-byte aligned
        const long long e0 = (long long)t * n;                          // the track's first element of the tensor
        const long long p0 = e0 >> 2, pieces = ((e0 + n - 1) >> 2) - p0 + 1;
        const long long b0 = (long long)t * S;                          // its first byte of the mask
        const long long q0 = b0 >> 4, mpieces = A.mask ? ((b0 + S - 1) >> 4) - q0 + 1 : 0;
        for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pieces + mpieces; p += (long long)gridDim.x * 256) {
            if (p >= pieces) { // a piece of the mask: byte j of the track is j < L
                const long long g = (q0 + (p - pieces)) << 4;
                const long long j0 = g - b0; // -15 .. S - 1
                if (j0 >= 0 && j0 + 16 <= (long long)S) {
                    const long long ones = (long long)L - j0; // bytes of the piece that are 1, where 0 .. 16
                    u32 w[4];
#pragma unroll
                    for (int h = 0; h < 4; h++) {
                        const long long c = ones - 4 * h;
                        w[h] = c <= 0 ? 0u : c >= 4 ? 0x01010101u : 0x01010101u >> (8 * (4 - (int)c));
                    }
                    *reinterpret_cast<uint4 *>(mask + g) = make_uint4(w[0], w[1], w[2], w[3]);
                } else {
#pragma unroll
                    for (int h = 0; h < 16; h++)
                        if (j0 + h >= 0 && j0 + h < (long long)S) mask[g + h] = j0 + h < (long long)L ? 1 : 0;
                }
                continue;
            }
            const long long g = (p0 + p) << 2;
            const long long i0 = g - e0; // -3 .. n - 1
            float v[4];
            if (!A.planar) {
                // the 8 bytes from element i0 of the source (in front of the track for a partial first piece)
                const long long s = i0 * 2, B = (long long)N * 2;
                const long long a0 = s & ~15LL;
                const int sh = (int)(s - a0); // 0, 2 .. 14
                const char *base = reinterpret_cast<const char *>(src);
                uint4 a = make_uint4(0, 0, 0, 0), b = a;
                if (a0 >= 0 && a0 < B) a = *reinterpret_cast<const uint4 *>(base + a0);
                if (sh > 8 && a0 + 16 >= 0 && a0 + 16 < B) b = *reinterpret_cast<const uint4 *>(base + a0 + 16);
                const u32 W[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
                const int w = sh >> 2;
                const bool half = (sh & 2) != 0;
                u32 x[3], r[2];
#pragma unroll
                for (int i = 0; i < 3; i++) x[i] = w == 0 ? W[i] : w == 1 ? W[i + 1] : w == 2 ? W[i + 2] : W[i + 3];
#pragma unroll
                for (int i = 0; i < 2; i++) r[i] = half ? (x[i] >> 16) | (x[i + 1] << 16) : x[i];
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const long long i = i0 + h;
                    v[h] = i >= 0 && i < (long long)N ? wbat_cell(plain, r[h >> 1] >> (16 * (h & 1)), k, sub, mul) : A.pad_value;
                }
            } else {
                const u32 first = i0 < 0 ? 0u : (u32)i0;
                u32 c = first / S, m = first - c * S;
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const long long i = i0 + h;
                    v[h] = A.pad_value;
                    if (i >= 0 && i < (long long)n) {
                        if (m < L) v[h] = wbat_cell(plain, (u32)(unsigned short)src[(long long)m * C + c], k, sub, mul);
                        if (++m == S) m = 0, c++;
                    }
                }
            }
            if (i0 >= 0 && i0 + 4 <= (long long)n) {
                track_store4(out + g, v);
            } else {
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (i0 + h >= 0 && i0 + h < (long long)n) out[g + h] = v[h];
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------
// What a request must be, wherever it comes from: -> nullptr, or what is wrong with it.
static const char *wave_batch_req_wrong(const opusgpu_wave_batch_req *r) {
    if (!r) return "wave batch: no request";
    if (r->norm != OPUSGPU_WAVE_NORM_NONE && r->norm != OPUSGPU_WAVE_NORM_ZMUV && r->norm != OPUSGPU_WAVE_NORM_PEAK) return "wave batch: an unknown norm";
    if (!std::isfinite(r->pad_value) || !std::isfinite(r->eps) || !std::isfinite(r->target)) return "wave batch: a field that is not finite";
    if (r->norm == OPUSGPU_WAVE_NORM_ZMUV && !(r->eps > 0)) return "wave batch: eps must be > 0";
    if (r->norm == OPUSGPU_WAVE_NORM_PEAK && !(r->target > 0)) return "wave batch: target must be > 0";
    if (r->stride_samples < 1) return "wave batch: stride_samples must be >= 1";
    if (r->mask != 0 && r->mask != 1) return "wave batch: mask must be 0 or 1";
    for (int32_t w : r->reserved)
        if (w) return "wave batch: a reserved word that is not 0";
    return nullptr;
}
// What ties a request to tracks of C channels in `format`: -> nullptr, or the reason of the refusal.
static const char *wave_batch_shape_wrong(const opusgpu_wave_batch_req &r, int C, int format) {
    if (format == OPUSGPU_TRACKS_S16) return "wave batch: a request is on and the format is int16 -- the dense tensor is float32";
    if (format != OPUSGPU_TRACKS_F32 && format != OPUSGPU_TRACKS_F32_PLANAR) return "wave batch: an unknown format";
    if (C < 1 || C > 8) return "wave batch: the channels must be 1 - 8";
    if (r.stride_samples > 0x7fffffffLL / C) return "wave batch: stride_samples * channels is above 0x7fffffff";
    return nullptr;
}
#define OG_WAVE_STRIDE_SHORT "wave batch: stride_samples is below the samples of a track"

// The stage over n tracks: checks, the chunk table, the uploads, the launches on `s`, the records' way back and the wait; every
// device buffer of the call is freed on every way out.  d_out holds opusgpu_wave_batch_layout's floats.  recs: n records out, or
// null.  why(reason) is told what a refusal was.
static int wave_batch_run(int device, hipStream_t s, int n_tracks, const opusgpu_wave_span *spans, int C, int format,
                          const opusgpu_wave_batch_req *req, const void *d_s16, void *d_out, opusgpu_wave_stat *recs,
                          const TrackFail &hip_failed, const std::function<void(const char *)> &why) {
    auto refuse = [&](const char *reason) {
        if (why) why(reason);
        return (int)OPUSGPU_BAD_ARG;
    };
    if (n_tracks < 0 || (n_tracks && !spans)) return refuse("wave batch: no spans");
    if (const char *bad = wave_batch_req_wrong(req)) return refuse(bad);
    if (const char *bad = wave_batch_shape_wrong(*req, C, format)) return refuse(bad);
    const int64_t S = req->stride_samples;
    const bool stats = req->norm != OPUSGPU_WAVE_NORM_NONE;
    std::vector<WbatTile> tiles;
    bool any = false;
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_wave_span &u = spans[t];
        if (u.in_offset < 0 || u.in_offset % 8 || u.samples < 0 || u.in_offset > INT64_MAX / 64 || !std::isfinite(u.scale) || u.reserved)
            return refuse("wave batch: a span that breaks a rule");
        if (u.samples > S) return refuse(OG_WAVE_STRIDE_SHORT);
        const int64_t chunks = (u.samples * C + WBAT_CHUNK - 1) / WBAT_CHUNK;
        if ((int64_t)tiles.size() + chunks > 0x7fffffff) return refuse("wave batch: too many chunks");
        if (stats)
            for (int64_t g = 0; g < chunks; g++) tiles.push_back(WbatTile{t, (i32)g});
        any |= u.samples > 0;
    }
    if (!n_tracks) return OPUSGPU_OK;
    int64_t mask_at = 0;
    if (opusgpu_wave_batch_layout(n_tracks, C, S, req->mask, &mask_at) < 0) return refuse("wave batch: there is no such tensor");
    if (!d_out || ((uintptr_t)d_out & 127) || (any && (!d_s16 || ((uintptr_t)d_s16 & 15)))) return refuse("wave batch: a buffer that is NULL or not aligned");
    // one channel's plane is its interleaved track
    const WbatArgs A{S, req->eps, req->target, C, format == OPUSGPU_TRACKS_F32_PLANAR && C > 1 ? 1 : 0, req->norm, req->mask, req->pad_value};
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles, d_stat;
    TRK_CHK(d_spans.upload(spans, (size_t)n_tracks * sizeof(WbatSpan)));
    if (stats) {
        TRK_CHK(d_stat.alloc((size_t)n_tracks * sizeof(WbatStat)));
        TRK_CHK(hipMemsetAsync(d_stat.p, 0, (size_t)n_tracks * sizeof(WbatStat), s));
        if (!tiles.empty()) {
            TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(WbatTile)));
            hipLaunchKernelGGL(k_wave_stats, dim3((unsigned)tiles.size()), dim3(256), 0, s, (const WbatTile *)d_tiles.p, (const WbatSpan *)d_spans.p,
                               (const i16 *)d_s16, C, (WbatStat *)d_stat.p);
            TRK_CHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_wave_fold, dim3((unsigned)((n_tracks + 63) / 64)), dim3(64), 0, s, (const WbatSpan *)d_spans.p, n_tracks, A,
                           (WbatStat *)d_stat.p);
        TRK_CHK(hipGetLastError());
    }
    // a workgroup per 16 KB of a track's tensor (4 pieces a lane), at most 1024 of them a track
    const int64_t pieces = S * C / 4 + 2 + (req->mask ? S / 16 + 2 : 0);
    const int64_t gx = std::min<int64_t>((pieces + 1023) / 1024, 1024);
    hipLaunchKernelGGL(k_wave_batch, dim3((unsigned)gx, (unsigned)std::min(n_tracks, 65535)), dim3(256), 0, s, (const WbatSpan *)d_spans.p, n_tracks,
                       (const i16 *)d_s16, A, (const WbatStat *)d_stat.p, (float *)d_out, (unsigned char *)d_out + mask_at);
    TRK_CHK(hipGetLastError());
    if (recs && stats) {
        TRK_CHK(hipMemcpyAsync(recs, d_stat.p, (size_t)n_tracks * sizeof(WbatStat), hipMemcpyDeviceToHost, s));
    } else if (recs) { // NONE measures nothing
        for (int t = 0; t < n_tracks; t++) recs[t] = opusgpu_wave_stat{spans[t].samples * C, 0, 0, 0.0, 1.0, 0, 0};
    }
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// What a request must keep (opusgpu_set_wave_batch): -> the state a context holds, off for NULL or `enabled` 0.
static int wave_batch_set(WaveBatchState &st, const opusgpu_wave_batch_req *req) {
    if (!req || !req->enabled) {
        st.req = opusgpu_wave_batch_req{};
        return OPUSGPU_OK;
    }
    if (wave_batch_req_wrong(req)) return OPUSGPU_BAD_ARG;
    st.req = *req;
    return OPUSGPU_OK;
}
static int wave_batch_last(const WaveBatchState &st, int n, opusgpu_wave_stat *recs) {
    if (n < 0) return OPUSGPU_BAD_ARG;
    const int have = (int)st.records.size();
    for (int i = 0; i < n && i < have && recs; i++) recs[i] = st.records[(size_t)i];
    return have;
}

extern "C" {

int64_t opusgpu_wave_batch_layout(int n, int channels, int64_t stride_samples, int mask, int64_t *mask_byte_offset) {
    if (n < 0 || channels < 1 || channels > 8 || stride_samples < 1 || stride_samples > 0x7fffffffLL / channels || (mask != 0 && mask != 1))
        return OPUSGPU_BAD_ARG;
    const int64_t floats = (int64_t)n * stride_samples * channels;
    if (!mask) return floats;
    const int64_t at = (floats * 4 + 127) / 128 * 128;
    if (mask_byte_offset) *mask_byte_offset = at;
    return (at + (int64_t)n * stride_samples + 3) / 4;
}

int opusgpu_set_wave_batch(opusgpu_ctx *ctx, const opusgpu_wave_batch_req *req) { return ctx ? wave_batch_set(ctx->wave, req) : OPUSGPU_BAD_ARG; }

int opusgpu_ms_set_wave_batch(opusgpu_ms *ms, const opusgpu_wave_batch_req *req) { return ms ? wave_batch_set(ms->wave, req) : OPUSGPU_BAD_ARG; }

int opusgpu_last_wave_stats(const opusgpu_ctx *ctx, int n, opusgpu_wave_stat *records) {
    return ctx ? wave_batch_last(ctx->wave, n, records) : OPUSGPU_BAD_ARG;
}

int opusgpu_ms_last_wave_stats(const opusgpu_ms *ms, int n, opusgpu_wave_stat *records) {
    return ms ? wave_batch_last(ms->wave, n, records) : OPUSGPU_BAD_ARG;
}

int opusgpu_tracks_wave_batch_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_wave_span *spans, int channels, int format,
                                     const opusgpu_wave_batch_req *req, const void *d_s16, void *d_out, opusgpu_wave_stat *stats_out,
                                     void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return wave_batch_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, channels, format, req, d_s16, d_out,
                          stats_out, track_fail(ctx), [ctx](const char *why) { snprintf(ctx->err, sizeof(ctx->err), "%s", why); });
}

} // extern "C"
