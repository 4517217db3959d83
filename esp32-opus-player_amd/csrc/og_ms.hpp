// og_ms.hpp -- multistream decoding (include/opusgpu.h, MULTISTREAM): included at the end of og_api.hip, whose contexts (og_ctx.hpp) and
// decode_step_impl (og_step.hpp) it drives.
//
// An opusgpu_ms owns two ordinary contexts: a 2-channel one with n_decoders * coupled streams and a 1-channel one with
// n_decoders * (streams - coupled) streams (either may be absent).  Decoder d's coupled stream s is stream d * coupled + s of the
// stereo context, its mono stream s (s >= coupled) stream d * (streams - coupled) + (s - coupled) of the mono context.  A step
// decodes every elementary frame through the contexts' own decode steps into PCM blocks the object owns, and k_ms_map turns
// those blocks into interleaved output channels (src/opus_decoder.cpp:826-914 does the same one packet at a time with
// opus_copy_channel_out_short).
#pragma once

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
struct opusgpu_ms {
    int device = -1;
    opusgpu_ms_layout lay{};
    int n_dec = 0, mono = 0, mode = OPUSGPU_MODE_REFERENCE;
    opusgpu_ctx *cc = nullptr, *cm = nullptr; // stereo (coupled) and mono contexts
    hipStream_t stream = nullptr, last_stream = nullptr;
    hipEvent_t ev_split = nullptr, ev_mono = nullptr;
    // the device step's tables and the contexts' PCM and codes
    void *d_dc = nullptr, *d_dm = nullptr, *d_pc = nullptr, *d_pm = nullptr, *d_rc = nullptr, *d_rm = nullptr;
    size_t cap_dc = 0, cap_dm = 0, cap_pc = 0, cap_pm = 0, cap_rc = 0, cap_rm = 0;
    // the host path: packet bytes, accumulators, placements, output
    void *d_arena = nullptr, *d_acc_c = nullptr, *d_acc_m = nullptr, *d_place = nullptr, *d_out = nullptr, *d_res = nullptr;
    size_t cap_arena = 0, cap_acc_c = 0, cap_acc_m = 0, cap_place = 0, cap_out = 0, cap_res = 0;
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

// opus_multistream_decoder_init's argument checks and validate_layout (src/opus_decoder.cpp:742-770, :688-697)
static bool ms_layout_ok(const opusgpu_ms_layout *l) {
    if (!l || l->channels > 255 || l->channels < 1 || l->coupled > l->streams || l->streams < 1 || l->coupled < 0 ||
        l->streams > 255 - l->coupled)
        return false;
    for (int c = 0; c < l->channels; c++)
        if (l->mapping[c] >= l->streams + l->coupled && l->mapping[c] != 255) return false;
    return true;
}

// LDS tile (samples) of k_ms_map: whole 20 ms rows where 16 KB hold them, 8-sample multiples always
static int ms_tile(int streams, int coupled, int longest) {
    int ts = 16384 / (2 * (streams + coupled)) / 8 * 8;
    const int want = (longest + 7) / 8 * 8;
    return ts > want ? want : (ts < 8 ? 8 : ts);
}

static int ms_launch_map(opusgpu_ms *ms, hipStream_t s, int n, const void *pc, int src_c, const void *pm, int src_m, const void *rc,
                         const void *rm, int longest, void *out, long long out_stride, void *result) {
    const opusgpu_ms_layout &L = ms->lay;
    MsMapArgs a;
    memset(a.mapping, 255, sizeof a.mapping);
    memcpy(a.mapping, L.mapping, (size_t)L.channels);
    const int ts = ms_tile(L.streams, L.coupled, longest);
    const size_t lds = (size_t)ts * (L.streams + L.coupled) * 2 + (size_t)(L.channels + L.streams) * 4;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(n), dim3(256), lds, s, (const int16_t *)pc, src_c, (const int16_t *)pm, src_m, (const int32_t *)rc,
                           (const int32_t *)rm, L.streams, L.coupled, L.channels, a, ts, (int16_t *)out, out_stride, (int32_t *)result);
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

// samples of one (elementary) packet as opus_packet_get_nb_samples counts them (src/opus_decoder.cpp:477-504)
static int ms_nb_samples(const uint8_t *p, int32_t len) {
    if (len < 1) return OPUSGPU_BAD_ARG;
    const int code = p[0] & 3;
    int count = code == 0 ? 1 : code != 3 ? 2 : -1;
    if (code == 3) {
        if (len < 2) return OPUSGPU_INVALID_PACKET;
        count = p[1] & 0x3F;
    }
    const int samples = count * ogh::toc_samples_per_frame(p[0], 48000);
    return samples * 25 > 48000 * 3 ? OPUSGPU_INVALID_PACKET : samples;
}

extern "C" {

int opusgpu_ms_packet_to_frames(const opusgpu_ms_layout *layout, const uint8_t *packet, int32_t len, int32_t decoder, int mode,
                                opusgpu_frame_desc *descs, int32_t *counts) {
    if (!ms_layout_ok(layout) || !packet || !descs || !counts || len < 0 || (mode != OPUSGPU_MODE_REFERENCE && mode != OPUSGPU_MODE_RFC))
        return OPUSGPU_BAD_ARG;
    const int S = layout->streams;
    // opus_multistream_decode_native (:855-865) and opus_multistream_packet_validate (:803-823)
    if (len == 0 || len < 2 * S - 1) return OPUSGPU_INVALID_PACKET;
    const uint8_t *data = packet;
    int samples = 0;
    for (int s = 0; s < S; s++) {
        if (len <= 0) return OPUSGPU_INVALID_PACKET;
        int16_t size[48];
        uint8_t toc;
        int off = 0;
        int32_t packet_offset = 0;
        const int count = ogh::parse_packet(data, len, s != S - 1, &toc, size, &off, &packet_offset);
        if (count < 0) return count;
        const int tmp = ms_nb_samples(data, packet_offset);
        if (tmp < 0) return tmp;
        if (s != 0 && samples != tmp) return OPUSGPU_INVALID_PACKET;
        samples = tmp;
        const int32_t flags = mode == OPUSGPU_MODE_RFC ? ogh::toc_flags_rfc(toc) : ogh::toc_flags(toc);
        int32_t at = (int32_t)(data - packet) + off;
        for (int k = 0; k < count; k++) {
            descs[s * 48 + k] = opusgpu_frame_desc{decoder, at, size[k], flags};
            at += size[k];
        }
        counts[s] = count;
        data += packet_offset;
        len -= packet_offset;
    }
    // Reference mode decodes every frame as 960 samples (Q6): streams of equal durations but different frame counts would give
    // different sample counts, and the reference's loop would overrun its buffer.  Refused here.
    if (mode == OPUSGPU_MODE_REFERENCE)
        for (int s = 1; s < S; s++)
            if (counts[s] != counts[0]) return OPUSGPU_INVALID_PACKET;
    return samples;
}

int opusgpu_ms_create(int device, const opusgpu_ms_layout *layout, int n_decoders, opusgpu_ms **out) {
    if (!out) return OPUSGPU_BAD_ARG;
    *out = nullptr;
    if (!ms_layout_ok(layout) || n_decoders <= 0 || (long long)n_decoders * layout->streams > 0x7fffffff) return OPUSGPU_BAD_ARG;
    opusgpu_ms *ms = new (std::nothrow) opusgpu_ms();
    if (!ms) return OPUSGPU_ALLOC_FAIL;
    ms->device = device;
    ms->lay = *layout;
    for (int c = layout->channels; c < 256; c++) ms->lay.mapping[c] = 255;
    ms->n_dec = n_decoders;
    ms->mono = layout->streams - layout->coupled;
    int rc = OPUSGPU_OK;
    if (layout->coupled && !(rc = opusgpu_ctx_create(device, &ms->cc))) rc = opusgpu_streams_alloc(ms->cc, n_decoders * layout->coupled, 2);
    if (!rc && ms->mono && !(rc = opusgpu_ctx_create(device, &ms->cm))) rc = opusgpu_streams_alloc(ms->cm, n_decoders * ms->mono, 1);
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
    opusgpu_ctx_destroy(ms->cc);
    opusgpu_ctx_destroy(ms->cm);
    for (void *p : {ms->d_dc, ms->d_dm, ms->d_pc, ms->d_pm, ms->d_rc, ms->d_rm, ms->d_arena, ms->d_acc_c, ms->d_acc_m, ms->d_place,
                    ms->d_out, ms->d_res})
        (void)hipFree(p);
    if (ms->ev_split) (void)hipEventDestroy(ms->ev_split);
    if (ms->ev_mono) (void)hipEventDestroy(ms->ev_mono);
    if (ms->stream) (void)hipStreamDestroy(ms->stream);
    delete ms;
}

const char *opusgpu_ms_last_error(const opusgpu_ms *ms) {
    if (!ms) return "no multistream decoder";
    if (ms->err[0]) return ms->err;
    if (ms->cc && ms->cc->err[0]) return ms->cc->err;
    if (ms->cm && ms->cm->err[0]) return ms->cm->err;
    return "";
}

int opusgpu_ms_set_mode(opusgpu_ms *ms, int mode) {
    if (!ms || (mode != OPUSGPU_MODE_REFERENCE && mode != OPUSGPU_MODE_RFC)) return OPUSGPU_BAD_ARG;
    if (ms->cc) opusgpu_set_mode(ms->cc, mode);
    if (ms->cm) opusgpu_set_mode(ms->cm, mode);
    ms->mode = mode;
    return OPUSGPU_OK;
}

int opusgpu_ms_reset(opusgpu_ms *ms, int first, int count, int full) {
    if (!ms || first < 0 || count < 0 || (long long)first + count > ms->n_dec) return OPUSGPU_BAD_ARG;
    if (count == 0) return OPUSGPU_OK;
    MSCHK(ms, hipSetDevice(ms->device));
    MSCHK(ms, hipStreamSynchronize(ms->last_stream)); // (an ms step still in flight works on these decoders' state)
    const int C2 = ms->lay.coupled;
    if (ms->cc)
        if (int rc = opusgpu_streams_reset(ms->cc, first * C2, count * C2, full)) return rc;
    if (ms->cm)
        if (int rc = opusgpu_streams_reset(ms->cm, first * ms->mono, count * ms->mono, full)) return rc;
    return OPUSGPU_OK;
}

// One device step of n rows (include/opusgpu.h).  Stereo half on the step's stream, mono half on the mono context's stream next to
// it, the mapping behind both on the step's stream.  map == false: the step ends behind both halves, with the elementary PCM and
// results in d_pc / d_pm / d_rc / d_rm for whoever is queued on `s` next (og_ms_tracks.hpp); d_pcm and d_result are not used.
static int ms_step_impl(opusgpu_ms *ms, int n, const void *d_descs, const void *d_arena, void *d_pcm, void *d_result, hipStream_t s,
                        bool map) {
    const opusgpu_ms_layout &L = ms->lay;
    const int C2 = L.coupled, M = ms->mono;
    const bool rfc = ms->mode == OPUSGPU_MODE_RFC;
    const int fr = rfc ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES;
    int rc;
    if (C2) {
        if ((rc = ms_grow(ms, &ms->d_dc, &ms->cap_dc, sizeof(FrameDesc) * (size_t)n * C2))) return rc;
        if ((rc = ms_grow(ms, &ms->d_pc, &ms->cap_pc, (size_t)n * C2 * fr * 2 * 2))) return rc;
        if ((rc = ms_grow(ms, &ms->d_rc, &ms->cap_rc, sizeof(int32_t) * (size_t)n * C2))) return rc;
    }
    if (M) {
        if ((rc = ms_grow(ms, &ms->d_dm, &ms->cap_dm, sizeof(FrameDesc) * (size_t)n * M))) return rc;
        if ((rc = ms_grow(ms, &ms->d_pm, &ms->cap_pm, (size_t)n * M * fr * 2))) return rc;
        if ((rc = ms_grow(ms, &ms->d_rm, &ms->cap_rm, sizeof(int32_t) * (size_t)n * M))) return rc;
    }
    hipLaunchKernelGGL(k_ms_split, dim3((n + 255) / 256), dim3(256), 0, s, (const FrameDesc *)d_descs, n, L.streams, C2, ms->n_dec,
                       rfc ? 1 : 0, (FrameDesc *)ms->d_dc, (FrameDesc *)ms->d_dm);
    MSCHK(ms, hipGetLastError());
    if (M) {
        MSCHK(ms, hipEventRecord(ms->ev_split, s));
        MSCHK(ms, hipStreamWaitEvent(ms->cm->stream, ms->ev_split, 0));
        if ((rc = decode_step_impl(ms->cm, n * M, ms->d_dm, d_arena, ms->d_pm, ms->d_rm, nullptr, true))) return rc;
    }
    if (C2 && (rc = decode_step_impl(ms->cc, n * C2, ms->d_dc, d_arena, ms->d_pc, ms->d_rc, s, true))) return rc;
    if (M) {
        MSCHK(ms, hipEventRecord(ms->ev_mono, ms->cm->stream));
        MSCHK(ms, hipStreamWaitEvent(s, ms->ev_mono, 0));
    }
    if (!map) return OPUSGPU_OK;
    return ms_launch_map(ms, s, n, ms->d_pc, fr * 2, ms->d_pm, fr, ms->d_rc, ms->d_rm, fr, d_pcm, (long long)fr * L.channels, d_result);
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
    if (ms->cm) MSCHK(ms, hipStreamSynchronize(ms->cm->stream));
    return OPUSGPU_OK;
}

// The host path.  Every multistream packet is framed on the host; elementary frame k of every elementary stream of every packet
// goes into step k of its context (the stereo and the mono context each run their own step table), the step's PCM is gathered
// into per-elementary-stream accumulators (k_ms_gather), and one k_ms_map per call turns those into the caller's layout.
int opusgpu_ms_decode_packets(opusgpu_ms *ms, int n, const int32_t *decoder_ids, const uint8_t *const *packets, const int32_t *lens,
                              int16_t *pcm, int frame_capacity, int32_t *result) {
    if (!ms || n < 0) return OPUSGPU_BAD_ARG;
    if (n == 0) return OPUSGPU_OK;
    if (!decoder_ids || !packets || !lens || !pcm || !result || frame_capacity <= 0 || frame_capacity > 48) return OPUSGPU_BAD_ARG;
    hipStream_t s = ms->stream;
    if (int rc = ms_enter(ms, s)) return rc;
    const opusgpu_ms_layout &L = ms->lay;
    const int S = L.streams, C2 = L.coupled, M = ms->mono, CH = L.channels;
    const bool rfc = ms->mode == OPUSGPU_MODE_RFC;
    // frame_size as opus_multistream_decode_native limits it (:840: at most 120 ms)
    const int frame_size = OG_MIN(frame_capacity * OPUSGPU_FRAME_SAMPLES, 5760);
    const int acc_samples = frame_capacity * OPUSGPU_FRAME_SAMPLES;
    auto ctx_of = [&](int st) { return st < C2 ? ms->cc : ms->cm; };
    auto sub_index = [&](int d, int st) { return st < C2 ? d * C2 + st : d * M + (st - C2); };
    // 1. framing: elementary frames of every packet, flat, with (packet, stream) -> first frame / count
    std::vector<opusgpu_frame_desc> frames;
    std::vector<int32_t> first((size_t)n * S + 1, 0), cnt((size_t)n * S, 0);
    std::vector<size_t> base(n + 1, 0);
    std::vector<int32_t> eres((size_t)n * S, 0); // per elementary stream: samples so far or its first negative code
    std::vector<opusgpu_frame_desc> tmp((size_t)S * 48);
    std::vector<int32_t> tcnt(S);
    frames.reserve((size_t)n * S);
    for (int i = 0; i < n; i++) {
        result[i] = 0;
        const int d = decoder_ids[i];
        const bool empty = !packets[i] || lens[i] == 0;
        base[i + 1] = base[i] + (empty || lens[i] < 0 ? 0 : (size_t)lens[i]);
        int code = 0;
        if (d < 0 || d >= ms->n_dec || lens[i] < 0)
            code = OPUSGPU_BAD_ARG;
        else if (empty) {
            for (int st = 0; st < S; st++) { // every elementary stream, as do_plc does (:851-874): the empty-packet branch, frame_size /
                                             // 960 passes (include/opusgpu.h EMPTY PACKETS); RFC mode: a lost packet, concealed
                opusgpu_ctx *c = ctx_of(st);
                const int e = sub_index(d, st);
                const ogh::PacketPlan p = ogh::plan_packet(nullptr, 0, e, c->n_streams, ms->mode, false, st < C2 ? 2 : 1,
                                                           rfc ? frame_capacity : frame_size / OPUSGPU_FRAME_SAMPLES, c->last_count[e], c->last_flags[e], nullptr);
                if (p.code) code = p.code;
                tcnt[st] = ogh::plan_descs(p, nullptr, 0, e, ms->mode, 0, nullptr, &tmp[st * 48]);
            }
        } else {
            const int samples = opusgpu_ms_packet_to_frames(&L, packets[i], lens[i], d, ms->mode, tmp.data(), tcnt.data());
            if (samples < 0)
                code = samples;
            else if (samples > frame_size)
                code = OPUSGPU_BUFFER_TOO_SMALL; // (:845-847)
            else if (!rfc && (tcnt[0] > frame_capacity || (S > 1 && ogh::toc_samples_per_frame(packets[i][0], 48000) > OPUSGPU_FRAME_SAMPLES)))
                // every frame decodes as 960 samples (Q6): more frames than the room (as opusgpu_decode_packets); and the
                // reference's second stream is checked against the first one's 960-per-frame count (:880, frame_size = ret),
                // which frames of 40 / 60 ms fail -- decided here, before anything is decoded
                code = OPUSGPU_BUFFER_TOO_SMALL;
            else
                for (int st = 0; st < S; st++) { // the TOC an empty packet of this stream decodes as (:327-331)
                    opusgpu_ctx *c = ctx_of(st);
                    const int e = sub_index(d, st);
                    ogh::remember_packet(ogh::decoded_plan(tcnt[st], tmp[st * 48].flags), &c->last_count[e], &c->last_flags[e]);
                    for (int k = 0; k < tcnt[st]; k++) {
                        tmp[st * 48 + k].stream = e;
                        tmp[st * 48 + k].offset += (int32_t)base[i];
                    }
                }
        }
        for (int st = 0; st < S; st++) {
            const size_t e = (size_t)i * S + st;
            first[e] = (int32_t)frames.size();
            if (code) {
                eres[e] = code;
                continue;
            }
            cnt[e] = tcnt[st];
            for (int k = 0; k < tcnt[st]; k++) frames.push_back(tmp[st * 48 + k]);
        }
        first[(size_t)n * S] = (int32_t)frames.size();
    }
    if (base[n] > 0x7fffffffu) return OPUSGPU_BAD_ARG; // descriptor offsets are 32-bit: split the call
    int rc;
    // 2. packet bytes, accumulators
    std::vector<uint8_t> arena(base[n] + 16, 0);
    for (int i = 0; i < n; i++)
        if (base[i + 1] > base[i]) memcpy(arena.data() + base[i], packets[i], base[i + 1] - base[i]);
    if ((rc = ms_grow(ms, &ms->d_arena, &ms->cap_arena, arena.size()))) return rc;
    MSCHK(ms, hipMemcpyAsync(ms->d_arena, arena.data(), arena.size(), hipMemcpyHostToDevice, s));
    const size_t acc_c = (size_t)acc_samples * 2, acc_m = (size_t)acc_samples; // int16 per elementary row
    if (C2 && (rc = ms_grow(ms, &ms->d_acc_c, &ms->cap_acc_c, (size_t)n * C2 * acc_c * 2))) return rc;
    if (M && (rc = ms_grow(ms, &ms->d_acc_m, &ms->cap_acc_m, (size_t)n * M * acc_m * 2))) return rc;
    const int fr = rfc ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES;
    // 3. steps: frame k of every elementary stream that has one and has not failed
    std::vector<int32_t> placed((size_t)n * S, 0);
    std::vector<opusgpu_frame_desc> tab[2];
    std::vector<int32_t> place[2], owner[2], got;
    for (int k = 0;; k++) {
        for (int h = 0; h < 2; h++) {
            tab[h].clear();
            place[h].clear();
            owner[h].clear();
        }
        for (int i = 0; i < n; i++)
            for (int st = 0; st < S; st++) {
                const size_t e = (size_t)i * S + st;
                if (cnt[e] <= k || eres[e] < 0) continue;
                const int h = st < C2 ? 0 : 1;
                tab[h].push_back(frames[first[e] + k]);
                place[h].push_back(h == 0 ? i * C2 + st : i * M + (st - C2));
                place[h].push_back(placed[e]);
                owner[h].push_back((int32_t)e);
            }
        if (tab[0].empty() && tab[1].empty()) break;
        for (int h = 0; h < 2; h++) {
            const int m = (int)tab[h].size();
            if (!m) continue;
            opusgpu_ctx *c = h == 0 ? ms->cc : ms->cm;
            const int ch = h == 0 ? 2 : 1;
            void **dd = h == 0 ? &ms->d_dc : &ms->d_dm, **dp = h == 0 ? &ms->d_pc : &ms->d_pm, **dr = h == 0 ? &ms->d_rc : &ms->d_rm;
            size_t *cd = h == 0 ? &ms->cap_dc : &ms->cap_dm, *cp = h == 0 ? &ms->cap_pc : &ms->cap_pm, *cr = h == 0 ? &ms->cap_rc : &ms->cap_rm;
            if ((rc = ms_grow(ms, dd, cd, sizeof(FrameDesc) * (size_t)m))) return rc;
            if ((rc = ms_grow(ms, dp, cp, (size_t)m * fr * ch * 2))) return rc;
            if ((rc = ms_grow(ms, dr, cr, sizeof(int32_t) * (size_t)m))) return rc;
            if ((rc = ms_grow(ms, &ms->d_place, &ms->cap_place, sizeof(int32_t) * 2 * (size_t)m))) return rc;
            MSCHK(ms, hipMemcpyAsync(*dd, tab[h].data(), sizeof(FrameDesc) * (size_t)m, hipMemcpyHostToDevice, s));
            MSCHK(ms, hipMemcpyAsync(ms->d_place, place[h].data(), sizeof(int32_t) * 2 * (size_t)m, hipMemcpyHostToDevice, s));
            if ((rc = decode_step_impl(c, m, *dd, ms->d_arena, *dp, *dr, s, false))) return rc;
            hipLaunchKernelGGL(k_ms_gather, dim3(m), dim3(256), 0, s, (const int16_t *)*dp, fr * ch, (const int32_t *)*dr,
                               (const int32_t *)ms->d_place, ch, (int16_t *)(h == 0 ? ms->d_acc_c : ms->d_acc_m),
                               (long long)(h == 0 ? acc_c : acc_m), acc_samples);
            MSCHK(ms, hipGetLastError());
            got.resize(m);
            MSCHK(ms, hipMemcpyAsync(got.data(), *dr, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
            MSCHK(ms, hipStreamSynchronize(s)); // (the next step's table depends on these codes, and d_place is reused)
            for (int j = 0; j < m; j++) {
                const size_t e = (size_t)owner[h][j];
                if (got[j] < 0)
                    eres[e] = got[j]; // a failing frame ends its stream's packet, as opus_decode_native stops (:336-339)
                else {
                    eres[e] += got[j];
                    placed[e] += got[j];
                }
            }
        }
    }
    // 4. one mapping over the accumulators, then the rows that succeeded to the caller
    std::vector<int32_t> er_c((size_t)n * C2), er_m((size_t)n * M);
    for (int i = 0; i < n; i++)
        for (int st = 0; st < S; st++) {
            const int32_t v = eres[(size_t)i * S + st];
            if (st < C2)
                er_c[(size_t)i * C2 + st] = v;
            else
                er_m[(size_t)i * M + (st - C2)] = v;
        }
    if (C2) {
        if ((rc = ms_grow(ms, &ms->d_rc, &ms->cap_rc, sizeof(int32_t) * er_c.size()))) return rc;
        MSCHK(ms, hipMemcpyAsync(ms->d_rc, er_c.data(), sizeof(int32_t) * er_c.size(), hipMemcpyHostToDevice, s));
    }
    if (M) {
        if ((rc = ms_grow(ms, &ms->d_rm, &ms->cap_rm, sizeof(int32_t) * er_m.size()))) return rc;
        MSCHK(ms, hipMemcpyAsync(ms->d_rm, er_m.data(), sizeof(int32_t) * er_m.size(), hipMemcpyHostToDevice, s));
    }
    const size_t out_row = (size_t)acc_samples * CH;
    if ((rc = ms_grow(ms, &ms->d_out, &ms->cap_out, (size_t)n * out_row * 2))) return rc;
    if ((rc = ms_grow(ms, &ms->d_res, &ms->cap_res, sizeof(int32_t) * (size_t)n))) return rc;
    if ((rc = ms_launch_map(ms, s, n, ms->d_acc_c, (int)acc_c, ms->d_acc_m, (int)acc_m, ms->d_rc, ms->d_rm, acc_samples, ms->d_out,
                            (long long)out_row, ms->d_res)))
        return rc;
    std::vector<int16_t> host_out((size_t)n * out_row);
    MSCHK(ms, hipMemcpyAsync(result, ms->d_res, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    MSCHK(ms, hipMemcpyAsync(host_out.data(), ms->d_out, host_out.size() * 2, hipMemcpyDeviceToHost, s));
    MSCHK(ms, hipStreamSynchronize(s));
    for (int i = 0; i < n; i++)
        if (result[i] > 0) memcpy(pcm + (size_t)i * out_row, host_out.data() + (size_t)i * out_row, (size_t)result[i] * CH * 2);
    return OPUSGPU_OK;
}

} // extern "C"
