// og_wave_trim.hpp -- leading and trailing silence cut off the int16 tracks of a wave batch (include/opusgpu.h, WAVE TRIM): exact
// integer frame energies of the packed int16 tracks that a resampling kernel wrote, a threshold under their maximum or an absolute
// one, and per track the span of samples between the first and the last active frame.  Included by og_api.hip behind
// og_wave_batch.hpp; files_resampled_to (og_tracks_resample.hpp) calls wave_trim_run between its kernel and wave_batch_run when
// the owner holds a request, and hands wave_batch_run the trimmed spans.  DESIGN.md section 13o.
#pragma once

// ---- kernels ------------------------------------------------------------------------------------------
// A streaming stage over 2-byte samples: the tracks are read once, in aligned 16-byte pieces; plain vector loads and stores and
// integer atomics only, so the order of arrival changes no bit.
//   k_wave_trim_energy  a workgroup per (track, tile of frames).  Frames begin and end on multiples of G = gcd(hop, fl / 2) samples,
//                       a multiple of 8: a GRANULE of G samples is whole pieces for any C.  First the energies of the tile's
//                       granules, per channel, as u64 cells in LDS: a lane takes an octet (8 samples, C pieces), squares them per
//                       channel, the lanes of a granule that are neighbours in the wave add up by a butterfly, one LDS atomic a
//                       group.  Then a lane per frame sums the frame's fl / G granules per channel, takes the maximum over the
//                       channels and stores M[f]; the wave's maximum goes to the track's record by one 64-bit atomicMax.
//   k_wave_trim_fold    a wave per track: the threshold, then first / last / active by wave reductions over the frames; writes
//                       the record and, if asked, the flag bytes, every byte once.
// Resources (tests/test_wave_trim.py reads them from the code objects): no scratch memory in either kernel.  k_wave_trim_energy
// has no static LDS and sizes its LDS at the launch: 8 bytes a cell, at most WTRIM_LDS_CELLS cells (64 KB; 35 cells at fl 2048, hop
// 512, one channel).  Up to 8 pieces a lane are in flight (C = 8), and every instantiation stays within 64 vector registers, 8 waves
// per SIMD.  k_wave_trim_fold uses no LDS.
constexpr int WTRIM_TILE = 16384;     // elements (samples x channels) the frames of one workgroup of k_wave_trim_energy advance over
constexpr int WTRIM_LDS_CELLS = 8192; // the most (granule, channel) cells of a tile: fl / G <= 1024 granules of 8 channels fit one frame
struct WtrimTile {
    i32 track, first; // the tile's first frame
};
struct WtrimStat { // opusgpu_wave_trim_stat as the kernels see it
    long long start, count, full;
    unsigned long long emax, thr;
    i32 frames, first, last, active;
    i32 reserved[2];
};
struct WtrimArgs {
    double ratio;
    unsigned long long threshold;
    long long margin;
    int hop, octets, hop_g, half_g; // octets a granule; granules a hop and half a frame
    int group;                      // lanes of a butterfly: the largest power of two <= 64 that divides `octets`
    int tile_frames, mode;
};
static_assert(sizeof(opusgpu_wave_trim_req) == 64 && sizeof(opusgpu_wave_trim_stat) == 64, "wave trim records");
static_assert(sizeof(WtrimStat) == sizeof(opusgpu_wave_trim_stat), "wave trim records");

// The track's record starts as zeros (a memset on the stream in front of this kernel).  frame_base[t]: the track's first cell of M.
template <int C>
__global__ void __launch_bounds__(256) k_wave_trim_energy(const WtrimTile *__restrict__ tiles, const WbatSpan *__restrict__ spans,
                                                          const long long *__restrict__ frame_base, const i16 *__restrict__ in, WtrimArgs A,
                                                          u64 *__restrict__ M, WtrimStat *__restrict__ stat) {
    extern __shared__ __align__(16) unsigned long long wtrim_cells[]; // [granules of the tile][C]
    const int tid = (int)threadIdx.x;
    const WtrimTile tile = tiles[blockIdx.x];
    const WbatSpan sp = spans[tile.track];
    const long long L = sp.samples;
    const int F = 1 + (int)(L / A.hop);
    const int nf = F - tile.first < A.tile_frames ? F - tile.first : A.tile_frames; // the tile's frames, >= 1
    const int NG = (nf - 1) * A.hop_g + 2 * A.half_g;                                // its granules: NG * C <= WTRIM_LDS_CELLS
    for (int i = tid; i < NG * C; i += 256) wtrim_cells[i] = 0;
    __syncthreads();
    const long long o0 = ((long long)tile.first * A.hop_g - A.half_g) * A.octets; // the tile's first octet of the track: < 0 in front of it
    const long long Lo = (L + 7) >> 3;                                            // the track's octets that hold a real sample
    const int NO = NG * A.octets;
    const i16 *src = in + sp.in_offset * C; // 16-byte aligned: in_offset is a multiple of 8
    for (int base = 0; base < NO; base += 256) {
        const int i = base + tid;
        const long long o = o0 + i;
        const bool real = i < NO && o >= 0 && o < Lo;
        u64 acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 0;
        if (real) {
            const long long e0 = o * 8 * C, N = L * C; // the octet's first element, the track's elements
            const int left = (int)(L - o * 8 < 8 ? L - o * 8 : 8); // its real samples, >= 1
            u32 w[4 * C];
#pragma unroll
            for (int k = 0; k < C; k++) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (e0 + 8 * k < N) v = *reinterpret_cast<const uint4 *>(src + e0 + 8 * k); // the piece holds a real element
                w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
            }
#pragma unroll
            for (int c = 0; c < C; c++) {
#pragma unroll
                for (int s = 0; s < 8; s += 2) { // element j = s * C + c is half j & 1 of word j >> 1
                    const int ja = s * C + c, jb = ja + C;
                    const i32 a = s < left ? (i32)(i16)(w[ja >> 1] >> (16 * (ja & 1))) : 0;
                    const i32 b = s + 1 < left ? (i32)(i16)(w[jb >> 1] >> (16 * (jb & 1))) : 0;
                    // a pair of -32768 squares to 2^31: an unsigned word holds it (k_wave_stats)
                    acc[c] += (u64)((u32)(a * a) + (u32)(b * b));
                }
            }
        }
        // `group` divides 256 and the octets of a granule, and the tile begins on a granule: aligned groups of lanes share a cell
        for (int d = 1; d < A.group; d <<= 1) {
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] += __shfl_xor(acc[c], d, 64);
        }
        if (real && (tid & (A.group - 1)) == 0) {
            unsigned long long *cell = wtrim_cells + (i / A.octets) * C;
#pragma unroll
            for (int c = 0; c < C; c++) atomicAdd(cell + c, (unsigned long long)acc[c]);
        }
    }
    __syncthreads();
    u64 top = 0;
    for (int j = tid; j < nf; j += 256) {
        u64 e[C];
#pragma unroll
        for (int c = 0; c < C; c++) e[c] = 0;
        const unsigned long long *cell = wtrim_cells + j * A.hop_g * C;
        for (int k = 0; k < 2 * A.half_g; k++) {
#pragma unroll
            for (int c = 0; c < C; c++) e[c] += cell[k * C + c];
        }
        u64 m = e[0];
#pragma unroll
        for (int c = 1; c < C; c++) m = m > e[c] ? m : e[c];
        M[frame_base[tile.track] + tile.first + j] = m;
        top = top > m ? top : m;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const u64 o = __shfl_xor(top, d, 64);
        top = top > o ? top : o;
    }
    if ((tid & 63) == 0 && top) atomicMax(&stat[tile.track].emax, (unsigned long long)top);
}

__global__ void __launch_bounds__(64) k_wave_trim_fold(const WbatSpan *__restrict__ spans, const long long *__restrict__ frame_base,
                                                       const u64 *__restrict__ M, WtrimArgs A, WtrimStat *__restrict__ stat,
                                                       unsigned char *__restrict__ flags) {
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    const long long L = spans[t].samples, at = frame_base[t];
    const int F = 1 + (int)(L / A.hop);
    const u64 emax = stat[t].emax;
    // (double)emax is exact (at most 2^43), the product is rounded once, the floor is exact and fits: ratio <= 1
    const u64 thr = A.mode == OPUSGPU_WAVE_TRIM_ABS ? A.threshold : (u64)floor(__dmul_rn((double)emax, A.ratio));
    i32 first = 0x7fffffff, last = -1, active = 0;
    for (int f = lane; f < F; f += 64) {
        const bool on = M[at + f] > thr;
        if (flags) flags[at + f] = on ? 1 : 0;
        if (on) {
            first = first < f ? first : f;
            last = f; // ascending
            active++;
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const i32 a = __shfl_xor(first, d, 64), b = __shfl_xor(last, d, 64);
        first = first < a ? first : a;
        last = last > b ? last : b;
        active += __shfl_xor(active, d, 64);
    }
    if (lane) return;
    WtrimStat r{};
    r.full = L, r.emax = emax, r.thr = thr, r.frames = F, r.first = -1, r.last = -1;
    if (active) {
        const long long a = (long long)first * A.hop - A.margin, b = ((long long)last + 1) * A.hop + A.margin;
        r.start = a > 0 ? a : 0;
        r.count = (b < L ? b : L) - r.start;
        r.first = first, r.last = last, r.active = active;
    }
    stat[t] = r;
}

// ---- host side ----------------------------------------------------------------------------------------
// What a request must be, wherever it comes from: -> nullptr, or what is wrong with it.
static const char *wave_trim_req_wrong(const opusgpu_wave_trim_req *r) {
    if (!r) return "wave trim: no request";
    if (r->frame_length < 16 || r->frame_length > 8192 || r->frame_length % 16) return "wave trim: frame_length must be a multiple of 16 in 16 - 8192";
    if (r->hop < 8 || r->hop > r->frame_length || r->hop % 8) return "wave trim: hop must be a multiple of 8 in 8 - frame_length";
    if (r->margin < 0 || r->margin % 8) return "wave trim: margin must be a multiple of 8 and >= 0";
    if (r->mode != OPUSGPU_WAVE_TRIM_REL && r->mode != OPUSGPU_WAVE_TRIM_ABS) return "wave trim: an unknown mode";
    if (!std::isfinite(r->ratio)) return "wave trim: a ratio that is not finite";
    if (r->mode == OPUSGPU_WAVE_TRIM_REL && !(r->ratio > 0 && r->ratio <= 1)) return "wave trim: ratio must be in (0, 1]";
    if (r->flags != 0 && r->flags != 1) return "wave trim: flags must be 0 or 1";
    for (int32_t w : r->reserved)
        if (w) return "wave trim: a reserved word that is not 0";
    return nullptr;
}
static int wtrim_gcd(int a, int b) { return b ? wtrim_gcd(b, a % b) : a; }

// The stage over n tracks: checks, the tile table, the uploads, the launches on `s`, one copy back and the wait; every device buffer
// of the call is freed on every way out.  recs: n records out.  flags_out: the flag bytes of all tracks, track by track, or null;
// read only where req->flags is on.  why(reason) is told what a refusal was.
static int wave_trim_run(int device, hipStream_t s, int n_tracks, const opusgpu_wave_span *spans, int C, const opusgpu_wave_trim_req *req,
                         const void *d_s16, opusgpu_wave_trim_stat *recs, uint8_t *flags_out, const TrackFail &hip_failed,
                         const std::function<void(const char *)> &why) {
    auto refuse = [&](const char *reason) {
        if (why) why(reason);
        return (int)OPUSGPU_BAD_ARG;
    };
    if (n_tracks < 0 || (n_tracks && !spans)) return refuse("wave trim: no spans");
    if (const char *bad = wave_trim_req_wrong(req)) return refuse(bad);
    if (C < 1 || C > 8) return refuse("wave trim: the channels must be 1 - 8");
    const int hop = req->hop, half = req->frame_length / 2, G = wtrim_gcd(hop, half);
    WtrimArgs A{req->ratio, req->threshold, req->margin, hop, G / 8, hop / G, half / G, 1, 1, req->mode};
    while (A.group < 64 && A.octets % (2 * A.group) == 0) A.group *= 2;
    // the frames of a tile: WTRIM_TILE elements of advance, and no more granules than the LDS cells hold (one frame's always fit)
    A.tile_frames = std::max(1, std::min(WTRIM_TILE / (hop * C), (WTRIM_LDS_CELLS / C - 2 * A.half_g) / A.hop_g + 1));
    std::vector<WtrimTile> tiles;
    std::vector<long long> base((size_t)n_tracks);
    int64_t frames = 0;
    bool any = false;
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_wave_span &u = spans[t];
        if (u.in_offset < 0 || u.in_offset % 8 || u.samples < 0 || u.in_offset > INT64_MAX / 64 || u.reserved)
            return refuse("wave trim: a span that breaks a rule");
        if (u.samples > 0x7fffffffLL / C) return refuse("wave trim: samples * channels is above 0x7fffffff");
        const int64_t F = 1 + u.samples / hop;
        const int64_t n_tiles = (F + A.tile_frames - 1) / A.tile_frames;
        if ((int64_t)tiles.size() + n_tiles > 0x7fffffff) return refuse("wave trim: too many tiles");
        for (int64_t g = 0; g < n_tiles; g++) tiles.push_back(WtrimTile{t, (i32)(g * A.tile_frames)});
        base[(size_t)t] = frames;
        frames += F;
        any |= u.samples > 0;
    }
    if (!n_tracks) return OPUSGPU_OK;
    if (!recs) return refuse("wave trim: no records to write");
    if (any && (!d_s16 || ((uintptr_t)d_s16 & 15))) return refuse("wave trim: a buffer that is NULL or not aligned");
    const bool flags = req->flags && flags_out;
    const size_t rec_bytes = (size_t)n_tracks * sizeof(WtrimStat), back_bytes = rec_bytes + (flags ? (size_t)frames : 0);
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles, d_base, d_M, d_back; // d_back: the records, then the flag bytes
    TRK_CHK(d_spans.upload(spans, (size_t)n_tracks * sizeof(WbatSpan)));
    TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(WtrimTile)));
    TRK_CHK(d_base.upload(base.data(), base.size() * sizeof(long long)));
    TRK_CHK(d_M.alloc((size_t)frames * sizeof(u64)));
    TRK_CHK(d_back.alloc(back_bytes));
    TRK_CHK(hipMemsetAsync(d_back.p, 0, rec_bytes, s));
    const size_t lds = (size_t)((A.tile_frames - 1) * A.hop_g + 2 * A.half_g) * C * sizeof(u64);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles.size()), dim3(256), lds, s, (const WtrimTile *)d_tiles.p, (const WbatSpan *)d_spans.p,
                           (const long long *)d_base.p, (const i16 *)d_s16, A, (u64 *)d_M.p, (WtrimStat *)d_back.p);
    };
    switch (C) {
        case 1: go(k_wave_trim_energy<1>); break;
        case 2: go(k_wave_trim_energy<2>); break;
        case 3: go(k_wave_trim_energy<3>); break;
        case 4: go(k_wave_trim_energy<4>); break;
        case 5: go(k_wave_trim_energy<5>); break;
        case 6: go(k_wave_trim_energy<6>); break;
        case 7: go(k_wave_trim_energy<7>); break;
        default: go(k_wave_trim_energy<8>); break;
    }
    TRK_CHK(hipGetLastError());
    hipLaunchKernelGGL(k_wave_trim_fold, dim3((unsigned)n_tracks), dim3(64), 0, s, (const WbatSpan *)d_spans.p, (const long long *)d_base.p,
                       (const u64 *)d_M.p, A, (WtrimStat *)d_back.p, flags ? (unsigned char *)d_back.p + rec_bytes : nullptr);
    TRK_CHK(hipGetLastError());
    std::vector<uint8_t> back(back_bytes);
    TRK_CHK(hipMemcpyAsync(back.data(), d_back.p, back_bytes, hipMemcpyDeviceToHost, s));
    TRK_CHK(hipStreamSynchronize(s));
    memcpy(recs, back.data(), rec_bytes);
    if (flags) memcpy(flags_out, back.data() + rec_bytes, (size_t)frames);
    return OPUSGPU_OK;
}

// What a request must keep (opusgpu_set_wave_trim): -> the state a context holds, off for NULL or `enabled` 0.  A request is only
// turned on beside a wave-batch request.
static int wave_trim_set(WaveTrimState &st, const WaveBatchState &wave, const opusgpu_wave_trim_req *req, char *err, size_t err_size) {
    if (!req || !req->enabled) {
        st.req = opusgpu_wave_trim_req{};
        return OPUSGPU_OK;
    }
    const char *bad = wave_trim_req_wrong(req);
    if (!bad && !wave.req.enabled) bad = OG_TRIM_NEEDS_BATCH;
    if (bad) {
        snprintf(err, err_size, "%s", bad);
        return OPUSGPU_BAD_ARG;
    }
    st.req = *req;
    return OPUSGPU_OK;
}
static int wave_trim_last(const WaveTrimState &st, int n, opusgpu_wave_trim_stat *recs) {
    if (n < 0) return OPUSGPU_BAD_ARG;
    const int have = (int)st.records.size();
    for (int i = 0; i < n && i < have && recs; i++) recs[i] = st.records[(size_t)i];
    return have;
}
static int64_t wave_trim_last_flags(const WaveTrimState &st, int64_t n_bytes, uint8_t *flags) {
    if (n_bytes < 0) return OPUSGPU_BAD_ARG;
    const int64_t have = (int64_t)st.flags.size();
    if (flags && have) memcpy(flags, st.flags.data(), (size_t)std::min(n_bytes, have));
    return have;
}

// files_resampled_to's step between its kernel and wave_batch_run: the stage over the spans the wave batch would get, which come
// back as {offset + start, count, scale}; the owner keeps the records and the flags.
static int wave_trim_spans(const FilesOwner &own, WaveTrimState &st, std::vector<opusgpu_wave_span> &tracks, int C, const void *d_s16) {
    const int n = (int)tracks.size();
    std::vector<opusgpu_wave_trim_stat> recs((size_t)n);
    int64_t frames = 0;
    for (const opusgpu_wave_span &u : tracks) frames += 1 + u.samples / st.req.hop;
    std::vector<uint8_t> flags(st.req.flags ? (size_t)frames : 0);
    if (int rc = wave_trim_run(own.device, own.stream, n, tracks.data(), C, &st.req, d_s16, recs.data(), flags.data(), own.hip_failed, own.refused))
        return rc;
    for (int t = 0; t < n; t++) { // start is a multiple of 8: wave_batch_run's alignment rule holds
        tracks[(size_t)t].in_offset += recs[(size_t)t].start;
        tracks[(size_t)t].samples = recs[(size_t)t].count;
    }
    st.records.swap(recs);
    st.flags.swap(flags);
    return OPUSGPU_OK;
}

extern "C" {

int opusgpu_set_wave_trim(opusgpu_ctx *ctx, const opusgpu_wave_trim_req *req) {
    return ctx ? wave_trim_set(ctx->trim, ctx->wave, req, ctx->err, sizeof(ctx->err)) : OPUSGPU_BAD_ARG;
}

int opusgpu_ms_set_wave_trim(opusgpu_ms *ms, const opusgpu_wave_trim_req *req) {
    return ms ? wave_trim_set(ms->trim, ms->wave, req, ms->err, sizeof(ms->err)) : OPUSGPU_BAD_ARG;
}

int opusgpu_last_wave_trim(const opusgpu_ctx *ctx, int n, opusgpu_wave_trim_stat *records) {
    return ctx ? wave_trim_last(ctx->trim, n, records) : OPUSGPU_BAD_ARG;
}

int opusgpu_ms_last_wave_trim(const opusgpu_ms *ms, int n, opusgpu_wave_trim_stat *records) {
    return ms ? wave_trim_last(ms->trim, n, records) : OPUSGPU_BAD_ARG;
}

int64_t opusgpu_last_wave_trim_flags(const opusgpu_ctx *ctx, int64_t n_bytes, uint8_t *flags) {
    return ctx ? wave_trim_last_flags(ctx->trim, n_bytes, flags) : OPUSGPU_BAD_ARG;
}

int64_t opusgpu_ms_last_wave_trim_flags(const opusgpu_ms *ms, int64_t n_bytes, uint8_t *flags) {
    return ms ? wave_trim_last_flags(ms->trim, n_bytes, flags) : OPUSGPU_BAD_ARG;
}

int opusgpu_tracks_wave_trim_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_wave_span *spans, int channels,
                                    const opusgpu_wave_trim_req *req, const void *d_s16, opusgpu_wave_trim_stat *stats_out,
                                    uint8_t *flags_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return wave_trim_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, channels, req, d_s16, stats_out,
                         flags_out, track_fail(ctx), [ctx](const char *why) { snprintf(ctx->err, sizeof(ctx->err), "%s", why); });
}

} // extern "C"
