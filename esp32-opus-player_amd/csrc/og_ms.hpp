// og_ms.hpp -- multistream decoding (include/opusgpu.h, MULTISTREAM): included at the end of og_api.hip, whose contexts (og_ctx.hpp) and
// decode_step_impl (og_step.hpp) it drives.
//
// An opusgpu_ms owns two ordinary contexts, its HALVES (og_ms_framing.hpp has which stream of which context decodes what): a
// 2-channel one for the coupled streams and a 1-channel one for the mono streams; either may be absent.  A step decodes every
// elementary frame through the contexts' own decode steps into PCM blocks the object owns, and k_ms_map turns those blocks into
// interleaved output channels (src/opus_decoder.cpp:826-914 does the same one packet at a time with opus_copy_channel_out_short).
#pragma once
#include "og_ms_framing.hpp"

// ---- kernels ----------------------------------------------------------------------------------------
// The device path's rows: row r = descs[r * streams .. + streams), one multistream frame.  One lane per row checks the row and
// writes the two contexts' step tables; a row that is refused gets descriptors of stream -1 (every kernel of a decode step
// reports those as OPUSGPU_BAD_ARG and touches nothing for them), so none of its elementary frames is decoded.
__global__ void __launch_bounds__(256) k_ms_split(const FrameDesc *__restrict__ descs, int n, int streams, int coupled, int n_dec,
                                                   int rfc, FrameDesc *__restrict__ dc, FrameDesc *__restrict__ dm) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= n) return;
    const int mono = streams - coupled;
    const FrameDesc *row = descs + (size_t)r * streams;
    const int d = row[0].stream;
    bool ok = d >= 0 && d < n_dec;
    const int dur = (row[0].flags >> 6) & 7;
    for (int s = 0; s < streams && ok; s++) {
        const int f = row[s].flags;
        ok = row[s].stream == d && (f & 3) != 3 && ((f >> 9) & 1) == rfc && !(f & (1 << 10)) && ((f >> 6) & 7) == dur &&
             (rfc ? !(f & OPUSGPU_DESC_NO_MODE) : dur == 0);
    }
    for (int s = 0; s < streams; s++) {
        FrameDesc o = row[s];
        if (!ok) o = FrameDesc{-1, 0, 0, row[s].flags & 63};
        if (s < coupled) {
            if (ok) o.stream = d * coupled + s;
            dc[(size_t)r * coupled + s] = o;
        } else {
            if (ok) o.stream = d * mono + (s - coupled);
            dm[(size_t)r * mono + (s - coupled)] = o;
        }
    }
}

// The host path's accumulation: frame j of a context's step lands in row[j] of the accumulator, `at[j]` samples in.
// Lengths and offsets are multiples of 120 samples (2.5 ms) and the strides multiples of 960: every copy is whole 16-byte pieces.
__global__ void __launch_bounds__(256) k_ms_gather(const int16_t *__restrict__ src, int src_stride, const int32_t *__restrict__ res,
                                                    const int32_t *__restrict__ place, int channels, int16_t *__restrict__ acc,
                                                    long long acc_stride, int acc_samples) {
    const int j = (int)blockIdx.x;
    const int ns = res[j];
    const int row = place[2 * j], at = place[2 * j + 1];
    if (ns <= 0 || at + ns > acc_samples || ns > src_stride / channels) return;
    const uint4 *s = reinterpret_cast<const uint4 *>(src + (size_t)j * src_stride);
    uint4 *o = reinterpret_cast<uint4 *>(acc + (size_t)row * acc_stride + (size_t)at * channels);
    const int pieces = ns * channels / 8;
    for (int q = (int)threadIdx.x; q < pieces; q += 256) o[q] = s[q];
}

// k_ms_map: the contexts' PCM -- stereo [rows * coupled][src_c] and mono [rows * mono][src_m] int16 -- to [rows][out_stride]
// interleaved output channels, one workgroup per row.  The row's result is the common sample count of its elementary frames or
// the first negative one in stream order; a failed row gets its code and no PCM.  The sources of a tile of TS samples come into
// LDS as 16-byte pieces (stereo streams as they are, L/R interleaved; mono streams after them), then every lane builds 16 bytes
// of consecutive output -- 8 samples of the interleaved row -- and stores them whole: a wave writes 1 KB of contiguous output per
// instruction.  lut[c] = LDS index of output channel c's first sample and its step (2 stereo, 1 mono), or -1: muted.
// CH > 0: the channel count is a constant of the instance (1..8); CH == 0: any count up to 255.
struct MsMapArgs {
    uint8_t mapping[256];
};
template <int CH>
__global__ void __launch_bounds__(256) k_ms_map(const int16_t *__restrict__ pc, int src_c, const int16_t *__restrict__ pm, int src_m,
                                                 const int32_t *__restrict__ rc, const int32_t *__restrict__ rm, int streams, int coupled,
                                                 int channels_rt, MsMapArgs map, int TS, int16_t *__restrict__ out, long long out_stride,
                                                 int32_t *__restrict__ result) {
    extern __shared__ __align__(16) int16_t lds[]; // [TS * (streams + coupled)] samples, then the channel table and the row's codes
    const int C = CH > 0 ? CH : channels_rt;
    const int mono = streams - coupled;
    const int row = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int decoded = streams + coupled;
    int *lut = reinterpret_cast<int *>(lds + (size_t)TS * decoded);
    int *codes = lut + C;
    for (int c = tid; c < C; c += 256) {
        const int m = map.mapping[c];
        lut[c] = m == 255 ? -1 : m < 2 * coupled ? ((m >> 1) * 2 * TS + (m & 1)) * 2 + 0 : (2 * coupled * TS + (m - 2 * coupled) * TS) * 2 + 1;
    }
    for (int s = tid; s < streams; s += 256)
        codes[s] = s < coupled ? rc[(size_t)row * coupled + s] : rm[(size_t)row * mono + (s - coupled)];
    __syncthreads();
    __shared__ int row_res;
    if (tid == 0) {
        int r = codes[0];
        for (int s = 0; s < streams && r >= 0; s++) {
            const int v = codes[s];
            if (v < 0)
                r = v;
            else if (v != r)
                r = OPUSGPU_INTERNAL_ERROR; // (elementary frames of one row always agree: the host and k_ms_split see to it)
        }
        if (r >= 0 && ((long long)r * C > out_stride || (coupled && r * 2 > src_c) || (mono && r > src_m))) r = OPUSGPU_INTERNAL_ERROR;
        result[row] = r;
        row_res = r;
    }
    __syncthreads();
    const int T = row_res;
    if (T <= 0) return;
    int16_t *orow = out + (size_t)row * out_stride;
    for (int t0 = 0; t0 < T; t0 += TS) {
        const int ts = T - t0 < TS ? T - t0 : TS; // a multiple of 8 (every duration is a multiple of 120 samples)
        // 1. sources of the tile -> LDS, 16 bytes per lane and load
        const int pc_pieces = ts / 4, pm_pieces = ts / 8; // per stereo / mono stream
        const int all = coupled * pc_pieces + mono * pm_pieces;
        for (int q = tid; q < all; q += 256) {
            uint4 v;
            int at;
            if (q < coupled * pc_pieces) {
                const int s = q / pc_pieces, w = q - s * pc_pieces;
                v = reinterpret_cast<const uint4 *>(pc + ((size_t)row * coupled + s) * src_c + (size_t)t0 * 2)[w];
                at = s * 2 * TS + w * 8;
            } else {
                const int q2 = q - coupled * pc_pieces;
                const int s = q2 / pm_pieces, w = q2 - s * pm_pieces;
                v = reinterpret_cast<const uint4 *>(pm + ((size_t)row * mono + s) * src_m + t0)[w];
                at = 2 * coupled * TS + s * TS + w * 8;
            }
            *reinterpret_cast<uint4 *>(lds + at) = v;
        }
        __syncthreads();
        // 2. LDS -> interleaved output, 8 samples (16 bytes) per lane and store
        const int out_pieces = ts * C / 8;
        uint4 *o = reinterpret_cast<uint4 *>(orow + (size_t)t0 * C);
        for (int q = tid; q < out_pieces; q += 256) {
            const int e0 = q * 8;
            int j = e0 / C, c = e0 - j * C;
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 8; k += 2) {
                int32_t v2[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int l = lut[c];
                    v2[h] = l < 0 ? 0 : (uint16_t)lds[(l >> 1) + j * (l & 1 ? 1 : 2)];
                    if (++c == C) {
                        c = 0;
                        j++;
                    }
                }
                w[k / 2] = (uint32_t)v2[0] | (uint32_t)v2[1] << 16;
            }
            o[q] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();
    }
}

// ---- host side ----------------------------------------------------------------------------------------
// One half of an opusgpu_ms (ogh::MsHalfLayout): its context and the buffers a step of it works in
struct MsHalf {
    opusgpu_ctx *ctx = nullptr;    // null: the layout has no such stream (streams == 0)
    int streams = 0, channels = 0; // elementary streams per decoder, channels of each
    bool own_stream = false;       // a device step of this half runs on its context's stream, next to the step's stream
    // a step's table, PCM and codes; the host path's accumulator
    void *d_desc = nullptr, *d_pcm = nullptr, *d_res = nullptr, *d_acc = nullptr;
    size_t cap_desc = 0, cap_pcm = 0, cap_res = 0, cap_acc = 0;
};
// what the mapping kernels read of a half: PCM rows [rows * streams][stride] int16 and the rows' results
struct MsSrc {
    const void *pcm;
    int stride;
    const void *res;
};

struct opusgpu_ms {
    int device = -1;
    opusgpu_ms_layout lay{};
    int n_dec = 0, mode = OPUSGPU_MODE_REFERENCE;
    MsHalf half[2]; // stereo (coupled) streams, mono streams
    hipStream_t stream = nullptr, last_stream = nullptr;
    hipEvent_t ev_split = nullptr, ev_mono = nullptr;
    // the host path: packet bytes, placements, output
    void *d_arena = nullptr, *d_place = nullptr, *d_out = nullptr, *d_res = nullptr;
    size_t cap_arena = 0, cap_place = 0, cap_out = 0, cap_res = 0;
    LoudnessState loud;
    FeatBatchState fbatch;
    WaveBatchState wave;
    WaveTrimState trim;
    StftBatchState sbatch;
    char err[256] = {0};
};

static int ms_fail(opusgpu_ms *ms, int code, const char *what, hipError_t e) {
    if (ms) snprintf(ms->err, sizeof(ms->err), "%s: %s", what, hipGetErrorString(e));
    return code;
}
#define MSCHK(ms, call)                                                       \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) return ms_fail(ms, OPUSGPU_ERR_HIP, #call, e_); \
    } while (0)

static int ms_grow(opusgpu_ms *ms, void **p, size_t *cap, size_t need) {
    if (*cap >= need) return OPUSGPU_OK;
    if (*p) MSCHK(ms, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    const size_t want = need + need / 4 + 256;
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) return ms_fail(ms, OPUSGPU_ALLOC_FAIL, "hipMalloc(multistream)", e);
    *cap = want;
    return OPUSGPU_OK;
}
// room for a step of m frames of a half: its table, PCM blocks of `fr` samples, codes
static int ms_half_room(opusgpu_ms *ms, MsHalf &h, size_t m, int fr) {
    int rc;
    if ((rc = ms_grow(ms, &h.d_desc, &h.cap_desc, sizeof(FrameDesc) * m))) return rc;
    if ((rc = ms_grow(ms, &h.d_pcm, &h.cap_pcm, m * fr * h.channels * 2))) return rc;
    return ms_grow(ms, &h.d_res, &h.cap_res, sizeof(int32_t) * m);
}
// the halves' step PCM (blocks of `fr` samples) and codes
static void ms_step_src(const opusgpu_ms *ms, int fr, MsSrc src[2]) {
    for (int h = 0; h < 2; h++) src[h] = MsSrc{ms->half[h].d_pcm, fr * ms->half[h].channels, ms->half[h].d_res};
}

// LDS tile (samples) of k_ms_map: whole 20 ms rows where 16 KB hold them, 8-sample multiples always
static int ms_tile(int streams, int coupled, int longest) {
    int ts = 16384 / (2 * (streams + coupled)) / 8 * 8;
    const int want = (longest + 7) / 8 * 8;
    return ts > want ? want : (ts < 8 ? 8 : ts);
}

static int ms_launch_map(opusgpu_ms *ms, hipStream_t s, int n, const MsSrc src[2], int longest, void *out, long long out_stride,
                         void *result) {
    const opusgpu_ms_layout &L = ms->lay;
    MsMapArgs a;
    memset(a.mapping, 255, sizeof a.mapping);
    memcpy(a.mapping, L.mapping, (size_t)L.channels);
    const int ts = ms_tile(L.streams, L.coupled, longest);
    const size_t lds = (size_t)ts * (L.streams + L.coupled) * 2 + (size_t)(L.channels + L.streams) * 4;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(n), dim3(256), lds, s, (const int16_t *)src[0].pcm, src[0].stride, (const int16_t *)src[1].pcm,
                           src[1].stride, (const int32_t *)src[0].res, (const int32_t *)src[1].res, L.streams, L.coupled, L.channels, a, ts,
                           (int16_t *)out, out_stride, (int32_t *)result);
    };
    switch (L.channels) {
        case 1: go(k_ms_map<1>); break;
        case 2: go(k_ms_map<2>); break;
        case 3: go(k_ms_map<3>); break;
        case 4: go(k_ms_map<4>); break;
        case 5: go(k_ms_map<5>); break;
        case 6: go(k_ms_map<6>); break;
        case 7: go(k_ms_map<7>); break;
        case 8: go(k_ms_map<8>); break;
        default: go(k_ms_map<0>); break;
    }
    MSCHK(ms, hipGetLastError());
    return OPUSGPU_OK;
}

extern "C" {

int opusgpu_ms_packet_to_frames(const opusgpu_ms_layout *layout, const uint8_t *packet, int32_t len, int32_t decoder, int mode,
                                opusgpu_frame_desc *descs, int32_t *counts) {
    if (!ogh::ms_layout_ok(layout) || !packet || !descs || !counts || len < 0 || (mode != OPUSGPU_MODE_REFERENCE && mode != OPUSGPU_MODE_RFC))
        return OPUSGPU_BAD_ARG;
    return ogh::ms_packet_to_frames(*layout, packet, len, decoder, mode, descs, counts);
}

int opusgpu_ms_create(int device, const opusgpu_ms_layout *layout, int n_decoders, opusgpu_ms **out) {
    if (!out) return OPUSGPU_BAD_ARG;
    *out = nullptr;
    if (!ogh::ms_layout_ok(layout) || n_decoders <= 0 || (long long)n_decoders * layout->streams > 0x7fffffff) return OPUSGPU_BAD_ARG;
    opusgpu_ms *ms = new (std::nothrow) opusgpu_ms();
    if (!ms) return OPUSGPU_ALLOC_FAIL;
    ms->device = device;
    ms->lay = *layout;
    for (int c = layout->channels; c < 256; c++) ms->lay.mapping[c] = 255;
    ms->n_dec = n_decoders;
    ms->half[1].own_stream = true;
    int rc = OPUSGPU_OK;
    for (int h = 0; h < 2 && !rc; h++) {
        const ogh::MsHalfLayout hl = ogh::ms_half(*layout, h);
        ms->half[h].streams = hl.streams, ms->half[h].channels = hl.channels;
        if (hl.streams && !(rc = opusgpu_ctx_create(device, &ms->half[h].ctx)))
            rc = opusgpu_streams_alloc(ms->half[h].ctx, n_decoders * hl.streams, hl.channels);
    }
    if (!rc && (hipStreamCreateWithFlags(&ms->stream, hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&ms->ev_split, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ms->ev_mono, hipEventDisableTiming) != hipSuccess))
        rc = OPUSGPU_ERR_HIP;
    if (rc) {
        opusgpu_ms_destroy(ms);
        return rc;
    }
    ms->last_stream = ms->stream;
    *out = ms;
    return OPUSGPU_OK;
}

void opusgpu_ms_destroy(opusgpu_ms *ms) {
    if (!ms) return;
    (void)hipSetDevice(ms->device);
    if (ms->stream) (void)hipStreamSynchronize(ms->stream);
    if (ms->last_stream && ms->last_stream != ms->stream) (void)hipStreamSynchronize(ms->last_stream);
    for (MsHalf &h : ms->half) opusgpu_ctx_destroy(h.ctx);
    for (MsHalf &h : ms->half)
        for (void *p : {h.d_desc, h.d_pcm, h.d_res, h.d_acc}) (void)hipFree(p);
    for (void *p : {ms->d_arena, ms->d_place, ms->d_out, ms->d_res}) (void)hipFree(p);
    if (ms->ev_split) (void)hipEventDestroy(ms->ev_split);
    if (ms->ev_mono) (void)hipEventDestroy(ms->ev_mono);
    if (ms->stream) (void)hipStreamDestroy(ms->stream);
    delete ms;
}

const char *opusgpu_ms_last_error(const opusgpu_ms *ms) {
    if (!ms) return "no multistream decoder";
    if (ms->err[0]) return ms->err;
    for (const MsHalf &h : ms->half)
        if (h.ctx && h.ctx->err[0]) return h.ctx->err;
    return "";
}

int opusgpu_ms_set_mode(opusgpu_ms *ms, int mode) {
    if (!ms || (mode != OPUSGPU_MODE_REFERENCE && mode != OPUSGPU_MODE_RFC)) return OPUSGPU_BAD_ARG;
    for (MsHalf &h : ms->half)
        if (h.ctx) opusgpu_set_mode(h.ctx, mode);
    ms->mode = mode;
    return OPUSGPU_OK;
}

int opusgpu_ms_reset(opusgpu_ms *ms, int first, int count, int full) {
    if (!ms || first < 0 || count < 0 || (long long)first + count > ms->n_dec) return OPUSGPU_BAD_ARG;
    if (count == 0) return OPUSGPU_OK;
    MSCHK(ms, hipSetDevice(ms->device));
    MSCHK(ms, hipStreamSynchronize(ms->last_stream)); // (an ms step still in flight works on these decoders' state)
    for (MsHalf &h : ms->half)
        if (h.ctx)
            if (int rc = opusgpu_streams_reset(h.ctx, first * h.streams, count * h.streams, full)) return rc;
    return OPUSGPU_OK;
}

// One device step of n rows (include/opusgpu.h).  Stereo half on the step's stream, mono half on the mono context's stream next to
// it (queued first), the mapping behind both on the step's stream.  map == false: the step ends behind both halves, with the elementary
// PCM and results in the halves' d_pcm / d_res for whoever is queued on `s` next (og_ms_tracks.hpp); d_pcm and d_result are not used.
static int ms_step_impl(opusgpu_ms *ms, int n, const void *d_descs, const void *d_arena, void *d_pcm, void *d_result, hipStream_t s,
                        bool map) {
    const opusgpu_ms_layout &L = ms->lay;
    const bool rfc = ms->mode == OPUSGPU_MODE_RFC;
    const int fr = rfc ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES;
    int rc;
    for (MsHalf &h : ms->half)
        if (h.streams && (rc = ms_half_room(ms, h, (size_t)n * h.streams, fr))) return rc;
    hipLaunchKernelGGL(k_ms_split, dim3((n + 255) / 256), dim3(256), 0, s, (const FrameDesc *)d_descs, n, L.streams, L.coupled, ms->n_dec,
                       rfc ? 1 : 0, (FrameDesc *)ms->half[0].d_desc, (FrameDesc *)ms->half[1].d_desc);
    MSCHK(ms, hipGetLastError());
    for (int i = 1; i >= 0; i--) {
        MsHalf &h = ms->half[i];
        if (!h.streams) continue;
        if (h.own_stream) {
            MSCHK(ms, hipEventRecord(ms->ev_split, s));
            MSCHK(ms, hipStreamWaitEvent(h.ctx->stream, ms->ev_split, 0));
        }
        if ((rc = decode_step_impl(h.ctx, n * h.streams, h.d_desc, d_arena, h.d_pcm, h.d_res, h.own_stream ? nullptr : s, true))) return rc;
    }
    for (MsHalf &h : ms->half)
        if (h.streams && h.own_stream) {
            MSCHK(ms, hipEventRecord(ms->ev_mono, h.ctx->stream));
            MSCHK(ms, hipStreamWaitEvent(s, ms->ev_mono, 0));
        }
    if (!map) return OPUSGPU_OK;
    MsSrc src[2];
    ms_step_src(ms, fr, src);
    return ms_launch_map(ms, s, n, src, fr, d_pcm, (long long)fr * L.channels, d_result);
}

// ms steps run in order: a change of stream drains the last one
static int ms_enter(opusgpu_ms *ms, hipStream_t s) {
    MSCHK(ms, hipSetDevice(ms->device));
    if (s != ms->last_stream) MSCHK(ms, hipStreamSynchronize(ms->last_stream));
    ms->last_stream = s;
    ms->err[0] = 0;
    return OPUSGPU_OK;
}

int opusgpu_ms_decode_step_device(opusgpu_ms *ms, int n, const void *d_descs, const void *d_arena, void *d_pcm, void *d_result,
                                  void *hip_stream) {
    if (!ms || n < 0) return OPUSGPU_BAD_ARG;
    if (n == 0) return OPUSGPU_OK;
    if (!d_descs || !d_arena || !d_pcm || !d_result || ((uintptr_t)d_arena & 15) || ((uintptr_t)d_pcm & 15)) return OPUSGPU_BAD_ARG;
    if ((long long)n * ms->lay.streams > 0x7fffffff) return OPUSGPU_BAD_ARG;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ms->stream;
    if (int rc = ms_enter(ms, s)) return rc;
    return ms_step_impl(ms, n, d_descs, d_arena, d_pcm, d_result, s, true);
}

int opusgpu_ms_synchronize(opusgpu_ms *ms) {
    if (!ms) return OPUSGPU_BAD_ARG;
    MSCHK(ms, hipSetDevice(ms->device));
    MSCHK(ms, hipStreamSynchronize(ms->last_stream));
    MSCHK(ms, hipStreamSynchronize(ms->stream));
    for (MsHalf &h : ms->half)
        if (h.ctx && h.own_stream) MSCHK(ms, hipStreamSynchronize(h.ctx->stream));
    return OPUSGPU_OK;
}

} // extern "C"

// One half's share of a step of the host path: the table and the placements up, the context's decode step, the gather into the
// half's accumulator, the codes back into `got` -- and the stream drained: the next table depends on these codes, and d_place is reused.
static int ms_host_half_step(opusgpu_ms *ms, MsHalf &h, const ogh::MsStepTable &t, int fr, int acc_samples, hipStream_t s,
                             std::vector<int32_t> &got) {
    const size_t m = t.tab.size();
    int rc;
    if ((rc = ms_half_room(ms, h, m, fr))) return rc;
    if ((rc = ms_grow(ms, &ms->d_place, &ms->cap_place, sizeof(int32_t) * 2 * m))) return rc;
    MSCHK(ms, hipMemcpyAsync(h.d_desc, t.tab.data(), sizeof(FrameDesc) * m, hipMemcpyHostToDevice, s));
    MSCHK(ms, hipMemcpyAsync(ms->d_place, t.place.data(), sizeof(int32_t) * 2 * m, hipMemcpyHostToDevice, s));
    if ((rc = decode_step_impl(h.ctx, (int)m, h.d_desc, ms->d_arena, h.d_pcm, h.d_res, s, false))) return rc;
    hipLaunchKernelGGL(k_ms_gather, dim3((unsigned)m), dim3(256), 0, s, (const int16_t *)h.d_pcm, fr * h.channels, (const int32_t *)h.d_res,
                       (const int32_t *)ms->d_place, h.channels, (int16_t *)h.d_acc, (long long)acc_samples * h.channels, acc_samples);
    MSCHK(ms, hipGetLastError());
    got.resize(m);
    MSCHK(ms, hipMemcpyAsync(got.data(), h.d_res, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
    MSCHK(ms, hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// The host path.  Every multistream packet is framed on the host (ogh::ms_plan_call); elementary frame k of every elementary
// stream of every packet goes into step k of its half (each half runs its own step table), the step's PCM is gathered into
// per-elementary-stream accumulators (k_ms_gather), and one k_ms_map per call turns those into the caller's layout.
extern "C" int opusgpu_ms_decode_packets(opusgpu_ms *ms, int n, const int32_t *decoder_ids, const uint8_t *const *packets,
                                         const int32_t *lens, int16_t *pcm, int frame_capacity, int32_t *result) {
    if (!ms || n < 0) return OPUSGPU_BAD_ARG;
    if (n == 0) return OPUSGPU_OK;
    if (!decoder_ids || !packets || !lens || !pcm || !result || frame_capacity <= 0 || frame_capacity > 48) return OPUSGPU_BAD_ARG;
    hipStream_t s = ms->stream;
    int rc;
    if ((rc = ms_enter(ms, s))) return rc;
    const opusgpu_ms_layout &L = ms->lay;
    const int fr = ms->mode == OPUSGPU_MODE_RFC ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES;
    const int acc_samples = frame_capacity * OPUSGPU_FRAME_SAMPLES; // per row of an accumulator and of the output
    // plan: every refusal, every frame, the arena's layout
    memset(result, 0, sizeof(int32_t) * (size_t)n);
    ogh::MsMemory mem[2] = {};
    for (int h = 0; h < 2; h++)
        if (opusgpu_ctx *c = ms->half[h].ctx) mem[h] = ogh::MsMemory{c->last_count.data(), c->last_flags.data(), c->n_streams};
    ogh::MsCallPlan plan;
    if ((rc = ogh::ms_plan_call(L, ms->n_dec, ms->mode, frame_capacity, n, decoder_ids, packets, lens, mem, plan))) return rc;
    // packet bytes up, accumulators
    const std::vector<uint8_t> arena = ogh::ms_fill_arena(plan, packets);
    if ((rc = ms_grow(ms, &ms->d_arena, &ms->cap_arena, arena.size()))) return rc;
    MSCHK(ms, hipMemcpyAsync(ms->d_arena, arena.data(), arena.size(), hipMemcpyHostToDevice, s));
    for (MsHalf &h : ms->half)
        if (h.streams && (rc = ms_grow(ms, &h.d_acc, &h.cap_acc, (size_t)n * h.streams * acc_samples * h.channels * 2))) return rc;
    // steps: frame k of every elementary stream that has one and has not failed
    ogh::MsStepTable tab[2];
    std::vector<int32_t> got;
    for (int k = 0; ogh::ms_step_tables(L, plan, k, tab); k++)
        for (int h = 0; h < 2; h++) {
            if (tab[h].tab.empty()) continue;
            if ((rc = ms_host_half_step(ms, ms->half[h], tab[h], fr, acc_samples, s, got))) return rc;
            ogh::ms_fold_step(plan, tab[h], got.data());
        }
    // one mapping over the accumulators, then the rows that succeeded to the caller
    std::vector<int32_t> er[2];
    MsSrc src[2];
    for (int h = 0; h < 2; h++) {
        MsHalf &x = ms->half[h];
        er[h] = ogh::ms_half_results(L, plan, h);
        if (x.streams && (rc = ms_grow(ms, &x.d_res, &x.cap_res, sizeof(int32_t) * er[h].size()))) return rc;
        if (x.streams) MSCHK(ms, hipMemcpyAsync(x.d_res, er[h].data(), sizeof(int32_t) * er[h].size(), hipMemcpyHostToDevice, s));
        src[h] = MsSrc{x.d_acc, acc_samples * x.channels, x.d_res};
    }
    const size_t out_row = (size_t)acc_samples * L.channels;
    if ((rc = ms_grow(ms, &ms->d_out, &ms->cap_out, (size_t)n * out_row * 2))) return rc;
    if ((rc = ms_grow(ms, &ms->d_res, &ms->cap_res, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ms_launch_map(ms, s, n, src, acc_samples, ms->d_out, (long long)out_row, ms->d_res))) return rc;
    std::vector<int16_t> host_out((size_t)n * out_row);
    MSCHK(ms, hipMemcpyAsync(result, ms->d_res, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    MSCHK(ms, hipMemcpyAsync(host_out.data(), ms->d_out, host_out.size() * 2, hipMemcpyDeviceToHost, s));
    MSCHK(ms, hipStreamSynchronize(s));
    for (int i = 0; i < n; i++)
        if (result[i] > 0) memcpy(pcm + (size_t)i * out_row, host_out.data() + (size_t)i * out_row, (size_t)result[i] * L.channels * 2);
    return OPUSGPU_OK;
}
