// og_ms_tracks.hpp -- whole multistream files (include/opusgpu.h, WHOLE FILES / MULTISTREAM): the kernel that maps channels and
// assembles tracks in one pass, and what the driver of a planned batch (og_files_run.hpp) needs of an opusgpu_ms.  Included at the
// end of og_api.hip behind og_ms.hpp (opusgpu_ms, ms_step_impl), og_tracks.hpp (TrackSeg, TrackState), og_tracks_resample.hpp,
// og_tracks_resample_ratio.hpp, og_feat.hpp, og_tracks_mel.hpp, og_tracks_stft.hpp, og_tracks_melspec.hpp and og_tracks_fbank.hpp.
#pragma once

// ---- kernel -------------------------------------------------------------------------------------------
// k_ms_tracks_assemble: k_ms_map and k_tracks_assemble in one, one workgroup per segment.  An ms step that ends in k_ms_map writes
// [rows][row_samples * channels] interleaved PCM which k_tracks_assemble would read back only to copy most of it once more; here
// the samples go from the two contexts' PCM -- stereo [rows * coupled][row_samples * 2], mono [rows * mono][row_samples] -- to
// their place in the track directly.
// The work is split by DESTINATION, as in k_tracks_assemble: lane q owns the q-th aligned 16-byte piece of the track buffer that
// the segment touches -- 8 consecutive int16 of the interleaved track -- composes it and stores it whole; only the segment's first
// and last piece, where it covers them in part, go out as 16-bit stores.  The sources come into LDS first, as in k_ms_map: of every
// elementary stream the mapping uses, the aligned 16-byte pieces that hold a sample the tile needs (stereo streams as they are, L/R
// interleaved; mono streams after them); the tile's first LDS sample is the source sample `A`, src_first rounded down to 8, so
// that every stream's pieces are aligned in HBM and in LDS alike.  A tile is PT destination pieces and the (at most TS) source
// samples they take; a 20 ms row of 8 channels is one tile, a 2,880-sample row of 8 channels three.
// lut[c] = LDS index of output channel c's sample A, times 2, plus 1 for a mono source (step 1 instead of 2); -1: muted.
struct MsTrackArgs {
    int n_stereo, n_mono; // the elementary streams that are staged: those the mapping uses, stereo ones first
    unsigned long long row_of; // byte j: which of its decoder's coupled (j < n_stereo) or mono streams staged stream j is -- packed, so
                               // that a lane gets at it with a shift: a table lookup would be a load in front of every PCM load
    int lut[8];           // output channel c: -1 muted, else (decoded channels staged before its stream) << 2 | right << 1 | mono
};
template <int CH>
__global__ void __launch_bounds__(256) k_ms_tracks_assemble(const TrackSeg *__restrict__ segs, const i16 *__restrict__ pc,
                                                             const i16 *__restrict__ pm, int row_samples, const i32 *__restrict__ rc,
                                                             const i32 *__restrict__ rm, int streams, int coupled, MsTrackArgs a, int TS,
                                                             i16 *__restrict__ tracks, TrackState *__restrict__ state) {
    extern __shared__ __align__(16) i16 lds[]; // [TS * staged decoded channels] samples, then the channel table
    const TrackSeg sg = segs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    const int mono = streams - coupled;
    // the row's result as k_ms_map forms it: the first negative elementary result in stream order, else the common count
    i32 res = 0;
    for (int s = 0; s < streams; s++) {
        const i32 v = s < coupled ? rc[(size_t)sg.slot * coupled + s] : rm[(size_t)sg.slot * mono + (s - coupled)];
        if (s == 0 || v < 0) res = v;
        if (v < 0) break;
        if (v != res) {
            res = OPUSGPU_INTERNAL_ERROR;
            break;
        }
    }
    if (res < 0) { // a failed row: nothing is written, the track ends at its packet (k_tracks_assemble's protocol)
        if (tid == 0) {
            const i32 old = atomicMin(&state[sg.track].first_bad, sg.packet_seq);
            if (sg.packet_seq < old) state[sg.track].code = res;
        }
        return;
    }
    if (sg.packet_seq >= state[sg.track].first_bad) return;
    if (sg.count <= 0 || sg.src_first < 0 || sg.src_first + sg.count > row_samples) return;
    const int D = 2 * a.n_stereo + a.n_mono;
    int *lut = reinterpret_cast<int *>(lds + (size_t)TS * D);
    if (tid < CH) {
        const int m = a.lut[tid];
        lut[tid] = m < 0 ? -1 : (((m >> 2) * TS + ((m >> 1) & 1)) << 1) | (m & 1);
    }
    // the segment in the track buffer, in int16 elements: pieces of 8
    const long long E0 = sg.dst_first * CH;
    const int EN = sg.count * CH;
    const long long c0 = E0 >> 3;
    const int lead = (int)(E0 - (c0 << 3)); // elements of the first piece that lie in front of the segment
    const int pieces = (lead + EN + 7) >> 3;
    const int PT = (TS - 8) * CH / 8; // pieces per tile: they take at most TS - 8 source samples, and up to 7 lie between A and the first
    const int cnt1 = sg.count - 1;
    for (int p0 = 0; p0 < pieces; p0 += PT) {
        const int p1 = p0 + PT < pieces ? p0 + PT : pieces;
        // the samples of the segment that pieces [p0, p1) hold
        const int j_lo = (p0 * 8 > lead ? p0 * 8 - lead : 0) / CH;
        const int j_end = (p1 * 8 - lead - 1) / CH;
        const int j_hi = j_end < cnt1 ? j_end : cnt1;
        const int lo = sg.src_first + j_lo;
        const int A = lo & ~7;
        const int n = sg.src_first + j_hi + 1 - A; // source samples [A, A + n), n <= TS
        // 1. sources of the tile -> LDS, 16 bytes per lane and load; no piece without a sample of [lo, A + n) is fetched
        const int pc_pieces = (n + 3) >> 2, pm_pieces = (n + 7) >> 3; // per stereo / mono stream
        const int pc_skip = (lo - A) >> 2;
        const int all = a.n_stereo * pc_pieces + a.n_mono * pm_pieces;
        for (int q = tid; q < all; q += 256) {
            uint4 v;
            int at;
            if (q < a.n_stereo * pc_pieces) {
                const int j = q / pc_pieces, w = q - j * pc_pieces;
                if (w < pc_skip) continue;
                v = reinterpret_cast<const uint4 *>(pc + ((size_t)sg.slot * coupled + ((a.row_of >> (8 * j)) & 255)) * row_samples * 2 + (size_t)A * 2)[w];
                at = j * 2 * TS + w * 8;
            } else {
                const int q2 = q - a.n_stereo * pc_pieces;
                const int j = q2 / pm_pieces, w = q2 - j * pm_pieces;
                v = reinterpret_cast<const uint4 *>(pm + ((size_t)sg.slot * mono + ((a.row_of >> (8 * (a.n_stereo + j))) & 255)) * row_samples + A)[w];
                at = (2 * a.n_stereo + j) * TS + w * 8;
            }
            *reinterpret_cast<uint4 *>(lds + at) = v;
        }
        __syncthreads();
        // 2. LDS -> the track, 8 interleaved int16 (16 bytes) per lane and store
        const int off = sg.src_first - A;
        for (int q = p0 + tid; q < p1; q += 256) {
            const int r0 = q * 8 - lead;           // the piece's first element, counted from the segment's (-7 .. -1: in front of it)
            int j = (r0 + 8 * CH) / CH - 8;        // its sample (floor) and channel
            int c = r0 - j * CH;
            int t = off + (j < 0 ? 0 : j > cnt1 ? cnt1 : j); // elements outside the segment read a sample of it: they are not stored
            u32 w[4];
#pragma unroll
            for (int k = 0; k < 8; k += 2) {
                u32 v2[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int l = lut[c];
                    v2[h] = l < 0 ? 0 : (uint16_t)lds[(l >> 1) + t * (l & 1 ? 1 : 2)];
                    if (++c == CH) {
                        c = 0;
                        j++;
                        t = off + (j < 0 ? 0 : j > cnt1 ? cnt1 : j);
                    }
                }
                w[k / 2] = v2[0] | v2[1] << 16;
            }
            i16 *d = tracks + ((c0 + q) << 3);
            if (r0 >= 0 && r0 + 8 <= EN) {
                *reinterpret_cast<uint4 *>(d) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int h = 0; h < 8; h++)
                    if (r0 + h >= 0 && r0 + h < EN) d[h] = (i16)(w[h >> 1] >> (16 * (h & 1)));
            }
        }
        __syncthreads();
    }
}

// k_ms_tracks_assemble_f32<CH, PLANAR>: the same pass into float tracks (og_tracks.hpp: TrackPlace, track_f32), every sample
// (float)s * scale[track] with s what k_ms_tracks_assemble stores.  The elementary rows are staged in LDS exactly as above; a
// destination piece is 16 bytes again, now 4 floats, so a tile is PT pieces of 4 elements.
// Interleaved: lane q owns the q-th aligned piece of the track buffer that the segment touches and composes its 4 floats through
// the channel table.  Planar: every output channel's plane is a straight scaled copy of one staged channel (zeros for a muted
// one); the pieces are aligned groups of 4 samples of the track -- the same cut for all planes, which begin on 256-byte
// boundaries -- and a tile's work items run plane after plane, piece after piece, so that a wave stores 1 KB of one plane.  In both
// forms no piece straddles two tiles, and the first and last piece, where covered in part, go out as 32-bit stores.
template <int CH, bool PLANAR>
__global__ void __launch_bounds__(256) k_ms_tracks_assemble_f32(const TrackSeg *__restrict__ segs, const i16 *__restrict__ pc,
                                                                 const i16 *__restrict__ pm, int row_samples, const i32 *__restrict__ rc,
                                                                 const i32 *__restrict__ rm, int streams, int coupled, MsTrackArgs a, int TS,
                                                                 const TrackPlace *__restrict__ place, float *__restrict__ tracks,
                                                                 TrackState *__restrict__ state) {
    extern __shared__ __align__(16) i16 lds[]; // [TS * staged decoded channels] samples, then the channel table
    const TrackSeg sg = segs[blockIdx.x];
    const int tid = (int)threadIdx.x;
    const int mono = streams - coupled;
    // the row's result as k_ms_map forms it: the first negative elementary result in stream order, else the common count
    i32 res = 0;
    for (int s = 0; s < streams; s++) {
        const i32 v = s < coupled ? rc[(size_t)sg.slot * coupled + s] : rm[(size_t)sg.slot * mono + (s - coupled)];
        if (s == 0 || v < 0) res = v;
        if (v < 0) break;
        if (v != res) {
            res = OPUSGPU_INTERNAL_ERROR;
            break;
        }
    }
    if (!track_seg_kept(sg, res, tid, row_samples, state)) return;
    const TrackPlace pl = place[sg.track];
    const float k = pl.scale;
    const int D = 2 * a.n_stereo + a.n_mono;
    int *lut = reinterpret_cast<int *>(lds + (size_t)TS * D);
    if (tid < CH) {
        const int m = a.lut[tid];
        lut[tid] = m < 0 ? -1 : (((m >> 2) * TS + ((m >> 1) & 1)) << 1) | (m & 1);
    }
    // the segment in elements of the piece sequence -- interleaved: of the track buffer, CH per sample; planar: of one plane of
    // its track, one per sample -- pieces of 4
    constexpr int U = PLANAR ? 1 : CH;
    const long long E0 = PLANAR ? sg.dst_first - pl.track_offset : sg.dst_first * CH;
    const int EN = sg.count * U;
    const long long c0 = E0 >> 2;
    const int lead = (int)(E0 - (c0 << 2)); // elements of the first piece that lie in front of the segment
    const int pieces = (lead + EN + 3) >> 2;
    const int PT = (TS - 8) * U / 4; // pieces per tile: they take at most TS - 8 source samples, and up to 7 lie between A and the first
    const int cnt1 = sg.count - 1;
    float *const out = PLANAR ? tracks + CH * pl.track_offset : tracks;
    for (int p0 = 0; p0 < pieces; p0 += PT) {
        const int p1 = p0 + PT < pieces ? p0 + PT : pieces;
        // the samples of the segment that pieces [p0, p1) hold
        const int j_lo = (p0 * 4 > lead ? p0 * 4 - lead : 0) / U;
        const int j_end = (p1 * 4 - lead - 1) / U;
        const int j_hi = j_end < cnt1 ? j_end : cnt1;
        const int lo = sg.src_first + j_lo;
        const int A = lo & ~7;
        const int n = sg.src_first + j_hi + 1 - A; // source samples [A, A + n), n <= TS
        // 1. sources of the tile -> LDS, 16 bytes per lane and load; no piece without a sample of [lo, A + n) is fetched
        const int pc_pieces = (n + 3) >> 2, pm_pieces = (n + 7) >> 3; // per stereo / mono stream
        const int pc_skip = (lo - A) >> 2;
        const int all = a.n_stereo * pc_pieces + a.n_mono * pm_pieces;
        for (int q = tid; q < all; q += 256) {
            uint4 v;
            int at;
            if (q < a.n_stereo * pc_pieces) {
                const int j = q / pc_pieces, w = q - j * pc_pieces;
                if (w < pc_skip) continue;
                v = reinterpret_cast<const uint4 *>(pc + ((size_t)sg.slot * coupled + ((a.row_of >> (8 * j)) & 255)) * row_samples * 2 + (size_t)A * 2)[w];
                at = j * 2 * TS + w * 8;
            } else {
                const int q2 = q - a.n_stereo * pc_pieces;
                const int j = q2 / pm_pieces, w = q2 - j * pm_pieces;
                v = reinterpret_cast<const uint4 *>(pm + ((size_t)sg.slot * mono + ((a.row_of >> (8 * (a.n_stereo + j))) & 255)) * row_samples + A)[w];
                at = (2 * a.n_stereo + j) * TS + w * 8;
            }
            *reinterpret_cast<uint4 *>(lds + at) = v;
        }
        __syncthreads();
        // 2. LDS -> the track, 4 floats (16 bytes) per lane and store
        const int off = sg.src_first - A;
        const int np = p1 - p0;
        for (int x = tid; x < (PLANAR ? np * CH : np); x += 256) {
            const int ch = PLANAR ? x / np : 0;          // planar: the item's plane
            const int q = p0 + (PLANAR ? x - ch * np : x);
            const int r0 = q * 4 - lead;                 // the piece's first element, counted from the segment's (-3 .. -1: in front of it)
            float f[4];
            if constexpr (PLANAR) {
                const int l = lut[ch];
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const int j = r0 + h < 0 ? 0 : r0 + h > cnt1 ? cnt1 : r0 + h; // elements outside the segment read a sample of it: they are not stored
                    f[h] = track_f32(l < 0 ? 0 : (uint16_t)lds[(l >> 1) + (off + j) * (l & 1 ? 1 : 2)], k);
                }
            } else {
                int j = (r0 + 4 * CH) / CH - 4;          // its sample (floor) and channel
                int c = r0 - j * CH;
                int t = off + (j < 0 ? 0 : j > cnt1 ? cnt1 : j);
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const int l = lut[c];
                    f[h] = track_f32(l < 0 ? 0 : (uint16_t)lds[(l >> 1) + t * (l & 1 ? 1 : 2)], k);
                    if (++c == CH) {
                        c = 0;
                        j++;
                        t = off + (j < 0 ? 0 : j > cnt1 ? cnt1 : j);
                    }
                }
            }
            float *d = out + (PLANAR ? ch * pl.plane_samples : 0) + ((c0 + q) << 2);
            if (r0 >= 0 && r0 + 4 <= EN) {
                track_store4(d, f);
            } else {
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (r0 + h >= 0 && r0 + h < EN) d[h] = f[h];
            }
        }
        __syncthreads();
    }
}

// ---- host side ----------------------------------------------------------------------------------------
// What a launch of either assembly kernel takes from the layout: the staged streams and the channel table, the LDS tile.
struct MsTrackPlan {
    MsTrackArgs a{};
    int ts = 0;
    size_t lds = 0;
};
static MsTrackPlan ms_track_plan(const opusgpu_ms_layout &L, int row_samples) {
    MsTrackPlan plan;
    MsTrackArgs &a = plan.a;
    // the streams the mapping uses, stereo ones first (stream order has them first), and where each lies in the staged tile
    int staged_at[256];
    bool used[256] = {};
    for (int c = 0; c < L.channels; c++)
        if (L.mapping[c] != 255) used[L.mapping[c] < 2 * L.coupled ? L.mapping[c] >> 1 : L.mapping[c] - L.coupled] = true;
    int n = 0;
    for (int st = 0; st < L.streams; st++) {
        if (!used[st]) continue;
        staged_at[st] = st < L.coupled ? 2 * n : 2 * a.n_stereo + (n - a.n_stereo);
        a.row_of |= (unsigned long long)(st < L.coupled ? st : st - L.coupled) << (8 * n++);
        (st < L.coupled ? a.n_stereo : a.n_mono)++;
    }
    for (int c = 0; c < 8; c++) {
        const int m = c < L.channels ? L.mapping[c] : 255;
        if (m == 255)
            a.lut[c] = -1;
        else if (m < 2 * L.coupled)
            a.lut[c] = staged_at[m >> 1] << 2 | (m & 1) << 1;
        else
            a.lut[c] = staged_at[m - L.coupled] << 2 | 1;
    }
    // LDS tile (samples): a whole row and its alignment slack where 16 KB hold them, 8-sample multiples always
    const int D = 2 * a.n_stereo + a.n_mono;
    int ts = 16384 / (2 * (D ? D : 1)) / 8 * 8;
    if (ts > row_samples + 16) ts = row_samples + 16;
    plan.ts = ts;
    plan.lds = (size_t)ts * D * 2 + (size_t)L.channels * 4;
    return plan;
}

static int ms_tracks_launch(opusgpu_ms *ms, hipStream_t s, int n_segs, const void *d_segs, const MsSrc src[2], int row_samples, void *d_tracks,
                            void *d_track_state) {
    const opusgpu_ms_layout &L = ms->lay;
    const MsTrackPlan plan = ms_track_plan(L, row_samples);
    const MsTrackArgs &a = plan.a;
    const int ts = plan.ts;
    const size_t lds = plan.lds;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)n_segs), dim3(256), lds, s, (const TrackSeg *)d_segs, (const i16 *)src[0].pcm,
                           (const i16 *)src[1].pcm, row_samples, (const i32 *)src[0].res, (const i32 *)src[1].res, L.streams, L.coupled, a, ts,
                           (i16 *)d_tracks, (TrackState *)d_track_state);
    };
    switch (L.channels) { // files carry 1 - 8 channels: no general instance
        case 1: go(k_ms_tracks_assemble<1>); break;
        case 2: go(k_ms_tracks_assemble<2>); break;
        case 3: go(k_ms_tracks_assemble<3>); break;
        case 4: go(k_ms_tracks_assemble<4>); break;
        case 5: go(k_ms_tracks_assemble<5>); break;
        case 6: go(k_ms_tracks_assemble<6>); break;
        case 7: go(k_ms_tracks_assemble<7>); break;
        case 8: go(k_ms_tracks_assemble<8>); break;
        default: return OPUSGPU_BAD_ARG;
    }
    MSCHK(ms, hipGetLastError());
    return OPUSGPU_OK;
}
static int ms_tracks_f32_launch(opusgpu_ms *ms, hipStream_t s, int n_segs, const void *d_segs, const MsSrc src[2], int row_samples, int format,
                                const void *d_place, void *d_tracks, void *d_track_state) {
    const opusgpu_ms_layout &L = ms->lay;
    const MsTrackPlan plan = ms_track_plan(L, row_samples);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)n_segs), dim3(256), plan.lds, s, (const TrackSeg *)d_segs, (const i16 *)src[0].pcm,
                           (const i16 *)src[1].pcm, row_samples, (const i32 *)src[0].res, (const i32 *)src[1].res, L.streams, L.coupled, plan.a,
                           plan.ts, (const TrackPlace *)d_place, (float *)d_tracks, (TrackState *)d_track_state);
    };
    const bool planar = format == OPUSGPU_TRACKS_F32_PLANAR;
#define OG_MS_F32(CH)                                                                                  \
    case CH:                                                                                           \
        planar ? go(k_ms_tracks_assemble_f32<CH, true>) : go(k_ms_tracks_assemble_f32<CH, false>);     \
        break;
    switch (L.channels) {
        OG_MS_F32(1) OG_MS_F32(2) OG_MS_F32(3) OG_MS_F32(4) OG_MS_F32(5) OG_MS_F32(6) OG_MS_F32(7) OG_MS_F32(8)
        default: return OPUSGPU_BAD_ARG;
    }
#undef OG_MS_F32
    MSCHK(ms, hipGetLastError());
    return OPUSGPU_OK;
}

// Device time of the step loop of the last opusgpu_ms_files_decode (events on the steps' stream around it; -1: none yet), so that
// tools/ms_files_rate.py can set the steps against opusgpu_ms_decode_step_device without the upload in front of them.
static float g_ms_files_steps_ms = -1.f;
struct MsStepTimer {
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    explicit MsStepTimer(hipStream_t stream) : s(stream) {
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess || hipEventRecord(a, s) != hipSuccess) a = nullptr;
    }
    void stop() {
        if (a && hipEventRecord(b, s) != hipSuccess) a = nullptr;
    }
    float elapsed_ms() const { // after the stream has been drained
        float ms = -1.f;
        return a && hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : -1.f;
    }
    ~MsStepTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

static TrackFail track_fail(opusgpu_ms *ms) {
    return [ms](int code, const char *what, hipError_t e) { return ms_fail(ms, code, what, e); };
}

// opusgpu_ms_files_decode and opusgpu_ms_files_decode_as: `places` is null for int16 tracks, else the batch's table for `format`
// (og_tracks.hpp: files_decode_run -- the driver does not depend on the format here either).
static int ms_files_decode_run(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int format, const std::vector<TrackPlace> *places,
                               void *d_tracks, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ms || !batch) return OPUSGPU_BAD_ARG;
    const opusgpu_ms_layout &lay = batch->layout;
    if (ms->n_dec < batch->n_files || ms->mode != batch->mode || ms->lay.channels > 8 || ms->lay.channels != lay.channels ||
        ms->lay.streams != lay.streams || ms->lay.coupled != lay.coupled || memcmp(ms->lay.mapping, lay.mapping, sizeof lay.mapping))
        return OPUSGPU_BAD_ARG;
    const int row = batch->mode == OPUSGPU_MODE_RFC ? OPUSGPU_RFC_FRAME_SAMPLES : OPUSGPU_FRAME_SAMPLES;
    hipStream_t s = ms->stream;
    if (!batch->segs.empty())
        if (int rc = ms_enter(ms, s)) return rc;
    RsDevBuf d_place; // the place table, for the length of this call
    if (places && !batch->segs.empty()) {
        MSCHK(ms, hipSetDevice(ms->device));
        MSCHK(ms, d_place.upload(places->data(), places->size() * sizeof(TrackPlace)));
    }
    std::unique_ptr<MsStepTimer> timer;
    FilesRunOps ops;
    ops.device = ms->device;
    ops.reset = [&](int n_files) { return opusgpu_ms_reset(ms, 0, n_files, 1); };
    // Each step ends behind its two halves instead of in k_ms_map, the fused assembly behind it on the same stream.  One set of
    // elementary PCM and result buffers (the halves' own) serves every step: step k + 1's stereo half is queued on `s` behind step
    // k's assembly, and its mono half, on the mono context's stream, waits for ev_split, which step k + 1 records on `s` -- behind
    // step k's assembly too.  Step 0 is the largest, so the buffers do not move after it.
    ops.step = [&](int, int n, const void *d_descs, const void *d_arena, int, void *const *) {
        return ms_step_impl(ms, n, d_descs, d_arena, nullptr, nullptr, s, false);
    };
    ops.assemble = [&](int, int n, const void *d_segs, void *const *, void *d_state) {
        MsSrc src[2];
        ms_step_src(ms, row, src);
        if (places) return ms_tracks_f32_launch(ms, s, n, d_segs, src, row, format, d_place.p, d_tracks, d_state);
        return ms_tracks_launch(ms, s, n, d_segs, src, row, d_tracks, d_state);
    };
    ops.drain = [&] { return opusgpu_ms_synchronize(ms); };
    ops.hip_failed = track_fail(ms);
    ops.loop_begin = [&] { timer.reset(new MsStepTimer(s)); };
    ops.loop_end = [&] { timer->stop(); };
    const int rc = files_run_tails(*batch, ops, s, format, d_tracks, track_lengths_out, status_out);
    if (!rc && timer) g_ms_files_steps_ms = timer->elapsed_ms();
    return rc;
}

// The owner of a whole-file call over a multistream batch (og_tracks.hpp: FilesOwner).
static FilesOwner files_owner(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch) {
    return FilesOwner{*batch, ms->device, ms->stream,
                      [=](void *d_s16, int64_t *lengths, int32_t *status) {
                          if (batch->track_stride) {
                              snprintf(ms->err, sizeof(ms->err), "%s", OG_STRIDE_REFUSED);
                              return (int)OPUSGPU_BAD_ARG;
                          }
                          return ms_files_decode_run(ms, batch, OPUSGPU_TRACKS_S16, nullptr, d_s16, lengths, status);
                      },
                      track_fail(ms), &ms->loud, false, &ms->fbatch,
                      [=](const char *why) { snprintf(ms->err, sizeof(ms->err), "%s", why); }, &ms->wave, &ms->sbatch, &ms->trim};
}

extern "C" {

float opusgpu_ms_files_last_steps_ms(void) { return g_ms_files_steps_ms; }

int opusgpu_ms_tracks_assemble_device_as(opusgpu_ms *ms, int n_segs, const void *d_segs, const void *d_pcm_coupled, const void *d_pcm_mono,
                                         int row_samples, const void *d_res_coupled, const void *d_res_mono, int format, const void *d_place,
                                         void *d_tracks, void *d_track_state, void *hip_stream) {
    const bool f32 = format == OPUSGPU_TRACKS_F32 || format == OPUSGPU_TRACKS_F32_PLANAR;
    if (!f32 && (format != OPUSGPU_TRACKS_S16 || d_place)) return OPUSGPU_BAD_ARG;
    if (!ms || n_segs < 0 || ms->lay.channels > 8) return OPUSGPU_BAD_ARG;
    if (n_segs == 0) return OPUSGPU_OK;
    if (!d_segs || !d_tracks || !d_track_state || row_samples <= 0 || row_samples % 8 || ((uintptr_t)d_tracks & 127) || ((uintptr_t)d_segs & 7))
        return OPUSGPU_BAD_ARG;
    if (f32 && (!d_place || ((uintptr_t)d_place & 7))) return OPUSGPU_BAD_ARG;
    const MsSrc src[2] = {{d_pcm_coupled, row_samples * 2, d_res_coupled}, {d_pcm_mono, row_samples, d_res_mono}};
    for (int h = 0; h < 2; h++)
        if (((uintptr_t)src[h].pcm & 15) || (ms->half[h].streams && (!src[h].pcm || !src[h].res))) return OPUSGPU_BAD_ARG;
    MSCHK(ms, hipSetDevice(ms->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ms->stream;
    if (f32) return ms_tracks_f32_launch(ms, s, n_segs, d_segs, src, row_samples, format, d_place, d_tracks, d_track_state);
    return ms_tracks_launch(ms, s, n_segs, d_segs, src, row_samples, d_tracks, d_track_state);
}

int opusgpu_ms_tracks_assemble_device(opusgpu_ms *ms, int n_segs, const void *d_segs, const void *d_pcm_coupled, const void *d_pcm_mono,
                                      int row_samples, const void *d_res_coupled, const void *d_res_mono, void *d_tracks,
                                      void *d_track_state, void *hip_stream) {
    return opusgpu_ms_tracks_assemble_device_as(ms, n_segs, d_segs, d_pcm_coupled, d_pcm_mono, row_samples, d_res_coupled, d_res_mono,
                                                OPUSGPU_TRACKS_S16, nullptr, d_tracks, d_track_state, hip_stream);
}

int opusgpu_ms_files_decode(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, void *d_tracks, int64_t *track_lengths_out,
                            int32_t *status_out) {
    if (!ms || !batch || ms->loud.req.mode == OPUSGPU_LOUDNESS_OFF)
        return ms_files_decode_run(ms, batch, OPUSGPU_TRACKS_S16, nullptr, d_tracks, track_lengths_out, status_out);
    return files_decode_measured(files_owner(ms, batch), d_tracks, track_lengths_out, status_out, [&](int64_t *lengths, int32_t *status) {
        return ms_files_decode_run(ms, batch, OPUSGPU_TRACKS_S16, nullptr, d_tracks, lengths, status);
    });
}

int opusgpu_ms_files_decode_as(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int format, const float *scale, void *d_tracks,
                               int64_t *track_lengths_out, int32_t *status_out) {
    if (!ms || !batch) return OPUSGPU_BAD_ARG;
    std::vector<TrackPlace> places;
    if (int rc = track_places(*batch, format, scale, places)) return rc;
    if (format == OPUSGPU_TRACKS_S16) return opusgpu_ms_files_decode(ms, batch, d_tracks, track_lengths_out, status_out);
    if (ms->loud.req.mode != OPUSGPU_LOUDNESS_OFF) {
        snprintf(ms->err, sizeof(ms->err), "%s", OG_LOUD_AS_REFUSED);
        return OPUSGPU_BAD_ARG;
    }
    return ms_files_decode_run(ms, batch, format, &places, d_tracks, track_lengths_out, status_out);
}

// opusgpu_files_decode_resampled behind opusgpu_ms_files_decode (og_tracks_resample.hpp): all channels, no downmix.
int opusgpu_ms_files_decode_resampled(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int format, const float *scale,
                                      void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                                      int32_t *status_out) {
    if (!ms || !batch) return OPUSGPU_BAD_ARG;
    return files_resampled_run(files_owner(ms, batch), rate, 0, nullptr, format, scale, d_out, out_offsets, out_lengths, track_lengths_out,
                               status_out);
}

// opusgpu_files_decode_mixed behind opusgpu_ms_files_decode: the surround tracks mixed down (or about) on their way to `rate`.
int opusgpu_ms_files_decode_mixed(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, const opusgpu_mix_matrix *mix, int format,
                                  const float *scale, void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                                  int32_t *status_out) {
    if (!ms || !batch || !mix) return OPUSGPU_BAD_ARG;
    return files_resampled_run(files_owner(ms, batch), rate, 0, mix, format, scale, d_out, out_offsets, out_lengths, track_lengths_out,
                               status_out);
}

// opusgpu_files_decode_ratio behind opusgpu_ms_files_decode (og_tracks_resample_ratio.hpp): the layout's channels, through *mix if
// there is one, at up / down of 48 kHz.
int opusgpu_ms_files_decode_ratio(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int up, int down, const opusgpu_mix_matrix *mix,
                                  int format, const float *scale, void *d_out, int64_t *out_offsets, int64_t *out_lengths,
                                  int64_t *track_lengths_out, int32_t *status_out) {
    if (!ms || !batch) return OPUSGPU_BAD_ARG;
    return files_ratio_run(files_owner(ms, batch), up, down, 0, mix, format, scale, d_out, out_offsets, out_lengths, track_lengths_out,
                           status_out);
}

// opusgpu_files_decode_mel behind opusgpu_ms_files_decode (og_tracks_mel.hpp): the layout's channels through a one-row *mix.
int opusgpu_ms_files_decode_mel(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, const opusgpu_mix_matrix *mix,
                                const opusgpu_mel_params *params, const float *scale, void *d_out, int64_t *feat_offsets, int64_t *frames_out,
                                int64_t *track_lengths_out, int32_t *status_out) {
    if (!ms || !batch || !mix) return OPUSGPU_BAD_ARG;
    return files_mel_run(files_owner(ms, batch), 0, mix, params, scale, d_out, feat_offsets, frames_out, track_lengths_out, status_out);
}

// opusgpu_files_decode_melspec behind opusgpu_ms_files_decode (og_tracks_melspec.hpp): the layout's channels through a one-row *mix.
int opusgpu_ms_files_decode_melspec(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int up, int down,
                                    const opusgpu_mix_matrix *mix, const opusgpu_spec_params *p, const float *scale, void *d_out,
                                    int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ms || !batch || !mix) return OPUSGPU_BAD_ARG;
    return files_melspec_run(files_owner(ms, batch), rate, up, down, 0, mix, p, scale, d_out, feat_offsets, frames_out, track_lengths_out,
                             status_out);
}

// opusgpu_files_decode_stft behind opusgpu_ms_files_decode (og_tracks_stft.hpp): the layout's channels through a one-row *mix.
int opusgpu_ms_files_decode_stft(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int up, int down,
                                 const opusgpu_mix_matrix *mix, const opusgpu_stft_params *p, const float *scale, void *d_out,
                                 int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ms || !batch || !mix) return OPUSGPU_BAD_ARG;
    return files_stft_run(files_owner(ms, batch), rate, up, down, 0, mix, p, scale, d_out, feat_offsets, frames_out, track_lengths_out,
                          status_out);
}

// opusgpu_files_decode_fbank behind opusgpu_ms_files_decode (og_tracks_fbank.hpp): the layout's channels through a one-row *mix.
int opusgpu_ms_files_decode_fbank(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int up, int down,
                                  const opusgpu_mix_matrix *mix, const opusgpu_fbank_params *p, const float *scale, void *d_out,
                                  int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ms || !batch || !mix) return OPUSGPU_BAD_ARG;
    return files_fbank_run(files_owner(ms, batch), rate, up, down, 0, mix, p, scale, d_out, feat_offsets, frames_out, track_lengths_out,
                           status_out);
}

} // extern "C"
