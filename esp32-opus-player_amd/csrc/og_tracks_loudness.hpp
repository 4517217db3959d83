// og_tracks_loudness.hpp -- integrated loudness (ITU-R BS.1770-4) and sample peak of packed int16 tracks (include/opusgpu.h, TRACK
// LOUDNESS): the two kernels, their host side, the request a context holds and what the whole-file calls do with it.  Included
// at the end of og_api.hip behind og_tracks.hpp (RsDevBuf, TrackFail, FilesOwner) and in front of og_tracks_resample.hpp, whose
// files_resampled_to measures the scratch S16 tracks through files_loudness below.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>

// ---- kernels ------------------------------------------------------------------------------------------
// k_tracks_loudness_seg<C>: one wave per entry of a tile table built on the host, a tile being LOUD_TILE consecutive segments of one
// track, a segment 4,800 samples (100 ms) of every channel.  A LANE owns one segment with all C channels in its loop: 8 samples of
// C interleaved channels are exactly C aligned 16-byte pieces (in_offset and 4,800 are multiples of 8), every byte of which the
// lane uses, and the recurrence -- serial in n -- runs 64 segments side by side in a wave, C independent chains per lane.
//   STATE.  The K-weighting's state at a segment's first sample comes from a WARM-UP: the filter starts from zero state one segment
//   earlier and runs over those 4,800 samples without summing (segment 0 starts from zero state at the track's first sample, which
//   is the definition).  The slowest pole has radius 0.99502: what a warm-up leaves out has decayed by 0.99502^4800 = 4e-11, far
//   below float32 rounding.  It costs the filter twice, and keeps every segment a function of the track alone.
//   ARITHMETIC.  Two biquads in transposed direct form II per channel, float32, every product and sum rounded on its own
//   (plain * and + under fp contract(off) in both functions -- __fmul_rn and __fadd_rn are * and + in a header compiled with
//   contraction on, which the compiler fuses after inlining: no fused multiply-add anywhere in the loop), the energy summed
//   sample by sample in the lane: the result is the same bits in every run and in every call, and tests/test_tracks_loudness.py
//   restates it in numpy.
//   A segment that is not whole (the track's last) has no energy that counts; its lane only takes the peak of the samples below
//   the track's length.  Pieces without a sample of the track are not fetched, elements at or past the length never used.
// C is a template parameter, so that every element position is a literal and the 4 C words, 4 C state values and C sums stay in
// registers: no scratch.
constexpr int LOUD_SEG = 4800;  // samples of a segment: 100 ms, a quarter of a block
constexpr int LOUD_TILE = 64;   // segments of a tile: one per lane of the wave
struct LoudSpan {
    long long in_offset, in_samples;
    long long seg_base; // the track's first place in the segment table
    long long reserved;
};
struct LoudTile {
    i32 track, first; // the tile's first segment
};
struct LoudWeights {
    float g[8];
};
static_assert(sizeof(opusgpu_loudness_span) == 16 && sizeof(opusgpu_loudness) == 16 && sizeof(opusgpu_loudness_req) == 48, "loudness records");

// BS.1770-4's two biquads at 48 kHz, {b0, b1, b2, a1, a2}
#define OG_LOUD_K1 1.53512485958697f, -2.69169618940638f, 1.19839281085285f, -1.69065929318241f, 0.73248077421585f
#define OG_LOUD_K2 1.0f, -2.0f, 1.0f, -1.99004745483398f, 0.99007225036621f

// one sample through one biquad: s[0], s[1] its state
__device__ __forceinline__ float loud_biquad(float x, float b0, float b1, float b2, float a1, float a2, float *s) {
#pragma clang fp contract(off)
    const float y = b0 * x + s[0];
    s[0] = (b1 * x - a1 * y) + s[1];
    s[1] = b2 * x - a2 * y;
    return y;
}
// 8 samples of C channels (w: their 4 C words) through the filter; SUM: into the energies and the peak as well
template <int C, bool SUM>
__device__ __forceinline__ void loud_group(const u32 *w, float (*st)[4], float *e, int &peak) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < 8; s++) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            const int at = s * C + c;
            const int v = (int)(i16)(w[at >> 1] >> (16 * (at & 1)));
            const float z = loud_biquad(loud_biquad((float)v * (1.0f / 32768), OG_LOUD_K1, st[c]), OG_LOUD_K2, st[c] + 2);
            if constexpr (SUM) {
                e[c] = e[c] + z * z;
                const int a = v < 0 ? -v : v;
                peak = a > peak ? a : peak;
            }
        }
    }
}

template <int C>
__global__ void __launch_bounds__(LOUD_TILE) k_tracks_loudness_seg(const LoudTile *__restrict__ tiles, const LoudSpan *__restrict__ spans,
                                                                    const i16 *__restrict__ in, float *__restrict__ seg) {
    const LoudTile tl = tiles[blockIdx.x];
    const LoudSpan sp = spans[tl.track];
    const long long j = (long long)tl.first + (int)threadIdx.x; // the lane's segment
    const long long n0 = j * LOUD_SEG;
    if (n0 >= sp.in_samples) return;
    const long long left = sp.in_samples - n0;
    const int own = left < LOUD_SEG ? (int)left : LOUD_SEG; // the segment's samples that lie in the track
    float st[C][4], e[C];
#pragma unroll
    for (int c = 0; c < C; c++) st[c][0] = st[c][1] = st[c][2] = st[c][3] = e[c] = 0.f;
    int peak = 0;
    const uint4 *p = reinterpret_cast<const uint4 *>(in + (sp.in_offset + n0) * C); // 16-byte aligned: both are multiples of 8
    if (j > 0 && own == LOUD_SEG) { // (a last segment that is not whole has no energy: no state to warm up)
        const uint4 *q = p - (LOUD_SEG / 8) * C;
        for (int g = 0; g < LOUD_SEG / 8; g++, q += C) {
            u32 w[4 * C];
#pragma unroll
            for (int k = 0; k < C; k++) {
                const uint4 v = q[k];
                w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
            }
            loud_group<C, false>(w, st, e, peak);
        }
    }
    const int full = own >> 3;
    for (int g = 0; g < full; g++, p += C) {
        u32 w[4 * C];
#pragma unroll
        for (int k = 0; k < C; k++) {
            const uint4 v = p[k];
            w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
        loud_group<C, true>(w, st, e, peak);
    }
    const int rest = (own & 7) * C; // elements of the track's last group, which is not whole: the peak alone
    if (rest) {
#pragma unroll
        for (int k = 0; k < C; k++) {
            if (8 * k >= rest) continue; // a piece without a sample of the track is not fetched
            const uint4 v = p[k];
            const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int h = 0; h < 8; h++) {
                const int s = (int)(i16)(w[h >> 1] >> (16 * (h & 1)));
                const int a = s < 0 ? -s : s;
                if (8 * k + h < rest) peak = a > peak ? a : peak;
            }
        }
    }
    float *const o = seg + (sp.seg_base + j) * (C + 1);
#pragma unroll
    for (int c = 0; c < C; c++) o[c] = e[c];
    o[C] = __int_as_float(peak);
}

// k_tracks_loudness_gate: one workgroup per track, over the track's places of the segment table.  Blocks, both gates and the means
// in double -- the table is small and the gate a comparison of sums, so the sums are kept far from their rounding --, every sum
// in a fixed order: lane t adds blocks t, t + 256, ... and the 256 partial sums fold as a tree in LDS.  The block power is formed
// the same way wherever it is needed (not stored: a long track has more blocks than LDS).  One 16-byte record per track.
constexpr int LOUD_GATE_LANES = 256;
__device__ __forceinline__ double loud_block(const float *__restrict__ e, int C, const LoudWeights &G, long long j) {
    double p = 0;
    for (int c = 0; c < C; c++) {
        const double a = (double)e[j * (C + 1) + c] + (double)e[(j + 1) * (C + 1) + c];
        const double b = (double)e[(j + 2) * (C + 1) + c] + (double)e[(j + 3) * (C + 1) + c];
        p += (double)G.g[c] * (a + b);
    }
    return p / (4.0 * LOUD_SEG);
}
// (sum, count) over the workgroup in a fixed order; every lane gets the result
__device__ __forceinline__ void loud_fold(double *sh_sum, int *sh_cnt, int tid, double &sum, int &cnt) {
    __syncthreads();
    sh_sum[tid] = sum, sh_cnt[tid] = cnt;
    __syncthreads();
    for (int h = LOUD_GATE_LANES / 2; h > 0; h >>= 1) {
        if (tid < h) sh_sum[tid] += sh_sum[tid + h], sh_cnt[tid] += sh_cnt[tid + h];
        __syncthreads();
    }
    sum = sh_sum[0], cnt = sh_cnt[0];
}
__global__ void __launch_bounds__(LOUD_GATE_LANES) k_tracks_loudness_gate(const LoudSpan *__restrict__ spans, const float *__restrict__ seg, int C,
                                                                           LoudWeights G, opusgpu_loudness *__restrict__ out) {
    __shared__ double sh_sum[LOUD_GATE_LANES];
    __shared__ int sh_cnt[LOUD_GATE_LANES];
    const int tid = (int)threadIdx.x;
    const LoudSpan sp = spans[blockIdx.x];
    const float *const e = seg + sp.seg_base * (C + 1);
    const long long segs = (sp.in_samples + LOUD_SEG - 1) / LOUD_SEG, whole = sp.in_samples / LOUD_SEG;
    const long long blocks = whole > 3 ? whole - 3 : 0;
    // the peak: every segment, the last one that is not whole included
    int peak = 0;
    for (long long j = tid; j < segs; j += LOUD_GATE_LANES) {
        const int a = __float_as_int(e[j * (C + 1) + C]);
        peak = a > peak ? a : peak;
    }
    __syncthreads();
    sh_cnt[tid] = peak;
    __syncthreads();
    for (int h = LOUD_GATE_LANES / 2; h > 0; h >>= 1) {
        if (tid < h) sh_cnt[tid] = sh_cnt[tid] > sh_cnt[tid + h] ? sh_cnt[tid] : sh_cnt[tid + h];
        __syncthreads();
    }
    peak = sh_cnt[0];
    // 1. the absolute gate: -0.691 + 10 log10 p > -70
    const double abs_gate = 1.1724653045822964e-7; // 10^((-70 + 0.691) / 10)
    double sum = 0;
    int cnt = 0;
    for (long long j = tid; j < blocks; j += LOUD_GATE_LANES) {
        const double p = loud_block(e, C, G, j);
        if (p > abs_gate) sum += p, cnt++;
    }
    loud_fold(sh_sum, sh_cnt, tid, sum, cnt);
    // 2. the relative gate: 10 LU below the mean of those
    const double rel_gate = cnt ? 0.1 * (sum / cnt) : 0;
    const int passed_abs = cnt;
    sum = 0, cnt = 0;
    for (long long j = tid; j < blocks && passed_abs; j += LOUD_GATE_LANES) {
        const double p = loud_block(e, C, G, j);
        if (p > abs_gate && p > rel_gate) sum += p, cnt++;
    }
    loud_fold(sh_sum, sh_cnt, tid, sum, cnt);
    if (tid == 0) {
        opusgpu_loudness r;
        r.lufs = cnt ? (float)(-0.691 + 10.0 * log10(sum / cnt)) : -__builtin_huge_valf();
        r.peak = (float)peak * (1.0f / 32768);
        r.blocks = (i32)blocks;
        r.gated = cnt;
        out[blockIdx.x] = r;
    }
}

// ---- host side ----------------------------------------------------------------------------------------
static const float og_loud_weights[8][8] = {{1},
                                            {1, 1},
                                            {1, 1, 1},
                                            {1, 1, 1.41f, 1.41f},
                                            {1, 1, 1, 1.41f, 1.41f},
                                            {1, 1, 1, 1.41f, 1.41f, 0},
                                            {1, 1, 1, 1.41f, 1.41f, 1, 0},
                                            {1, 1, 1, 1.41f, 1.41f, 1, 1, 0}};
static bool loud_weights_ok(const float *w, int n) {
    for (int c = 0; c < n; c++)
        if (!std::isfinite(w[c]) || w[c] < 0) return false;
    return true;
}

// The kernels over n tracks: checks the spans, builds the tile table, uploads, launches on `s`, waits and brings the records to
// `out`, which is written only when everything went well.
static int tracks_loudness_run(int device, hipStream_t s, int n_tracks, const opusgpu_loudness_span *spans, const void *d_in, int channels,
                               const float *weights, opusgpu_loudness *out, const TrackFail &hip_failed) {
    if (channels < 1 || channels > 8 || n_tracks < 0 || (n_tracks && (!spans || !out))) return OPUSGPU_BAD_ARG;
    if (weights && !loud_weights_ok(weights, channels)) return OPUSGPU_BAD_ARG;
    std::vector<LoudSpan> sp((size_t)n_tracks);
    std::vector<LoudTile> tiles;
    long long places = 0;
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_loudness_span &u = spans[t];
        if (u.in_offset < 0 || u.in_offset % 8 || u.in_samples < 0 || u.in_samples > (int64_t)LOUD_SEG * 0x7fffff00) return OPUSGPU_BAD_ARG;
        const long long segs = (u.in_samples + LOUD_SEG - 1) / LOUD_SEG;
        if ((segs + LOUD_TILE - 1) / LOUD_TILE + (long long)tiles.size() > 0x7fffffff) return OPUSGPU_BAD_ARG;
        sp[(size_t)t] = LoudSpan{u.in_offset, u.in_samples, places, 0};
        for (long long j = 0; j < segs; j += LOUD_TILE) tiles.push_back(LoudTile{t, (i32)j});
        places += segs;
    }
    const opusgpu_loudness silent = {-std::numeric_limits<float>::infinity(), 0.f, 0, 0};
    if (tiles.empty()) { // no sample anywhere: the records of tracks without a block
        for (int t = 0; t < n_tracks; t++) out[t] = silent;
        return OPUSGPU_OK;
    }
    if (!d_in || ((uintptr_t)d_in & 15)) return OPUSGPU_BAD_ARG;
    LoudWeights G{};
    for (int c = 0; c < channels; c++) G.g[c] = weights ? weights[c] : og_loud_weights[channels - 1][c];
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles, d_seg, d_rec;
    TRK_CHK(d_spans.upload(sp.data(), sp.size() * sizeof(LoudSpan)));
    TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(LoudTile)));
    TRK_CHK(d_seg.alloc((size_t)places * (channels + 1) * sizeof(float)));
    TRK_CHK(d_rec.alloc((size_t)n_tracks * sizeof(opusgpu_loudness)));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles.size()), dim3(LOUD_TILE), 0, s, (const LoudTile *)d_tiles.p, (const LoudSpan *)d_spans.p,
                           (const i16 *)d_in, (float *)d_seg.p);
    };
    switch (channels) {
        case 1: go(k_tracks_loudness_seg<1>); break;
        case 2: go(k_tracks_loudness_seg<2>); break;
        case 3: go(k_tracks_loudness_seg<3>); break;
        case 4: go(k_tracks_loudness_seg<4>); break;
        case 5: go(k_tracks_loudness_seg<5>); break;
        case 6: go(k_tracks_loudness_seg<6>); break;
        case 7: go(k_tracks_loudness_seg<7>); break;
        default: go(k_tracks_loudness_seg<8>); break;
    }
    TRK_CHK(hipGetLastError());
    hipLaunchKernelGGL(k_tracks_loudness_gate, dim3((unsigned)n_tracks), dim3(LOUD_GATE_LANES), 0, s, (const LoudSpan *)d_spans.p,
                       (const float *)d_seg.p, channels, G, (opusgpu_loudness *)d_rec.p);
    TRK_CHK(hipGetLastError());
    std::vector<opusgpu_loudness> rec((size_t)n_tracks);
    TRK_CHK(hipMemcpyAsync(rec.data(), d_rec.p, rec.size() * sizeof(opusgpu_loudness), hipMemcpyDeviceToHost, s));
    TRK_CHK(hipStreamSynchronize(s));
    std::copy(rec.begin(), rec.end(), out);
    return OPUSGPU_OK;
}

static double loud_gain(const opusgpu_loudness &r, double target_lufs, double peak_limit) {
    if (!(r.lufs > -std::numeric_limits<float>::infinity())) return 1.0;
    double g = std::pow(10.0, (target_lufs - (double)r.lufs) / 20.0);
    if (peak_limit > 0 && (double)r.peak * g > peak_limit) g = peak_limit / (double)r.peak;
    return g;
}

// What a request must keep (opusgpu_set_loudness): -> the state a context holds, `on` false for NULL or mode 0.
static int loud_set(LoudnessState &st, const opusgpu_loudness_req *req) {
    if (!req || req->mode == OPUSGPU_LOUDNESS_OFF) {
        st.req = opusgpu_loudness_req{};
        return OPUSGPU_OK;
    }
    if (req->mode != OPUSGPU_LOUDNESS_MEASURE && req->mode != OPUSGPU_LOUDNESS_NORMALIZE) return OPUSGPU_BAD_ARG;
    if (req->n_weights < 0 || req->n_weights > 8 || !loud_weights_ok(req->weights, req->n_weights)) return OPUSGPU_BAD_ARG;
    if (req->mode == OPUSGPU_LOUDNESS_NORMALIZE && (!std::isfinite(req->target_lufs) || !std::isfinite(req->peak_limit))) return OPUSGPU_BAD_ARG;
    st.req = *req;
    return OPUSGPU_OK;
}
static int loud_last(const LoudnessState &st, int n, opusgpu_loudness *records, double *gains) {
    if (n < 0) return OPUSGPU_BAD_ARG;
    const int have = (int)st.records.size();
    for (int i = 0; i < n && i < have; i++) {
        if (records) records[i] = st.records[(size_t)i];
        if (gains) gains[i] = st.gains[(size_t)i];
    }
    return have;
}

// A whole-file call with a request on, its S16 tracks decoded and their final lengths known: measures them where they lie and
// keeps records and gains (1 each when the request only measures) in the owner's state.  n_weights other than 0 must be the
// tracks' channel count.
static int files_loudness(const FilesOwner &own, const void *d_s16, const int64_t *final_lengths) {
    LoudnessState &st = *own.loud;
    const og_batch &b = own.b;
    const size_t n = (size_t)b.n_files;
    if (st.req.n_weights && st.req.n_weights != b.channels) return OPUSGPU_BAD_ARG;
    std::vector<opusgpu_loudness_span> spans(n);
    for (size_t i = 0; i < n; i++) spans[i] = opusgpu_loudness_span{b.info[i].track_offset, final_lengths[i]};
    std::vector<opusgpu_loudness> rec(n);
    if (int rc = tracks_loudness_run(own.device, own.stream, b.n_files, spans.data(), d_s16, b.channels, st.req.n_weights ? st.req.weights : nullptr,
                                     rec.data(), own.hip_failed))
        return rc;
    st.records = rec;
    st.gains.assign(n, 1.0);
    if (st.req.mode == OPUSGPU_LOUDNESS_NORMALIZE)
        for (size_t i = 0; i < n; i++) st.gains[i] = loud_gain(rec[i], st.req.target_lufs, st.req.peak_limit);
    return OPUSGPU_OK;
}
static bool loud_on(const FilesOwner &own) { return own.loud && own.loud->req.mode != OPUSGPU_LOUDNESS_OFF; }
static bool loud_normalizes(const FilesOwner &own) { return own.loud && own.loud->req.mode == OPUSGPU_LOUDNESS_NORMALIZE; }
// The scale a normalising call applies to track i: (float)((double)scale[i] * g).
static float loud_scale(const FilesOwner &own, const float *scale, size_t i) {
    return (float)((double)(scale ? scale[i] : 1.0f / 32768) * own.loud->gains[i]);
}

// opusgpu_files_decode and its multistream twin with a request on: int16 tracks in the caller's buffer, measured there after the
// last step.  run(lengths, status) is the decode.
template <class Run>
static int files_decode_measured(const FilesOwner &own, void *d_tracks, int64_t *track_lengths_out, int32_t *status_out, Run run) {
    if (!loud_on(own)) return run(track_lengths_out, status_out);
    if (loud_normalizes(own)) return OPUSGPU_BAD_ARG; // integer gain is not offered (TRACK FORMATS)
    const size_t n = (size_t)own.b.n_files;
    if (own.loud->req.n_weights && own.loud->req.n_weights != own.b.channels) return OPUSGPU_BAD_ARG;
    std::vector<int64_t> lengths(n, 0);
    std::vector<int32_t> status(2 * n, 0);
    if (int rc = run(lengths.data(), status.data())) return rc;
    if (int rc = files_loudness(own, d_tracks, lengths.data())) return rc;
    if (track_lengths_out) std::copy(lengths.begin(), lengths.end(), track_lengths_out);
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    return OPUSGPU_OK;
}

extern "C" {

int opusgpu_loudness_weights(int channels, float *weights) {
    if (channels < 1 || channels > 8 || !weights) return OPUSGPU_BAD_ARG;
    for (int c = 0; c < channels; c++) weights[c] = og_loud_weights[channels - 1][c];
    return OPUSGPU_OK;
}

double opusgpu_loudness_gain(const opusgpu_loudness *r, double target_lufs, double peak_limit) { return r ? loud_gain(*r, target_lufs, peak_limit) : 1.0; }

int opusgpu_tracks_loudness_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_loudness_span *spans, const void *d_in, int channels,
                                   const float *weights, opusgpu_loudness *out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_loudness_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in, channels, weights, out,
                               track_fail(ctx));
}

int opusgpu_set_loudness(opusgpu_ctx *ctx, const opusgpu_loudness_req *req) { return ctx ? loud_set(ctx->loud, req) : OPUSGPU_BAD_ARG; }

int opusgpu_last_loudness(const opusgpu_ctx *ctx, int n, opusgpu_loudness *records, double *gains) {
    return ctx ? loud_last(ctx->loud, n, records, gains) : OPUSGPU_BAD_ARG;
}

int opusgpu_ms_set_loudness(opusgpu_ms *ms, const opusgpu_loudness_req *req) { return ms ? loud_set(ms->loud, req) : OPUSGPU_BAD_ARG; }

int opusgpu_ms_last_loudness(const opusgpu_ms *ms, int n, opusgpu_loudness *records, double *gains) {
    return ms ? loud_last(ms->loud, n, records, gains) : OPUSGPU_BAD_ARG;
}

} // extern "C"
