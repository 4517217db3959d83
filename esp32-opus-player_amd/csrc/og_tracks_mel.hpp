// og_tracks_mel.hpp -- log-mel features of the 16 kHz mono tracks (include/opusgpu.h, TRACK FEATURES): the tables, the kernel that
// turns packed int16 mono tracks into float32 feature tracks, its host side, and the whole-file call that ends in it.  Included at
// the end of og_api.hip behind og_feat.hpp, which holds what this kernel shares with the other feature kernels -- the span and tile
// records, the table builders and packers, the run function and the whole-file flow --, and in front of og_ms_tracks.hpp, which holds
// the multistream twin of the whole-file call.
#pragma once

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_mel<MB>: one workgroup per entry of a tile table built on the host, a tile being MEL_T = 128 consecutive frames of one
// track, 32 per wave.  MB is the number of 32-band blocks (3 for 80 bands, 4 for 128).
//   1. STAGE.  The tile's window -- 127 * 160 + 400 samples, the first of them sample 160 * first - 200 of the track -- comes into
//      LDS as int16.  Samples of the track itself come through aligned 16-byte loads, one piece per lane (the window begins at a
//      multiple of 8 samples of a track that begins at one: pieces of the buffer are pieces of the window; nothing is read behind
//      the piece that holds the track's last sample).  Then the places in front of the track and behind it are filled from LDS by
//      the reflection rule, 0 where the reflected index lies outside the track -- or in front of the window, which happens only to
//      frames at or behind the track's last, never stored.  EVERY place the products read has been written: a partial last tile
//      computes all 128 frames, on zeros and reflections, and stores the ones there are.
//      In LDS the window is cut by PHASE as in k_tracks_resample: place p of the window lies at [p % 160][p / 160], so tap i of frame
//      f is at [i % 160][i / 160 + f] and the 32 lanes of a half wave, which hold 32 consecutive frames, read consecutive samples.
//   2. DFT.  The window is folded: w[i] = w[400 - i], w[0] = 0, so with u_i = x_i + x_{400 - i}, v_i = x_i - x_{400 - i}
//          Re[k] = sum_{i = 1 .. 200} Wc'[i][k] u_i,   Im[k] = sum_{i = 1 .. 199} Ws[i][k] v_i,
//      Wc' = Wc but for row 200, which is halved (u_200 = 2 x_200; v_200 = 0 whatever the table holds).  x = (float)y * scale is made
//      where it is read, one multiply that is never contracted.  A wave owns 32 frames and walks the 7 blocks of 32 bins (224 >=
//      201; the table is 0 behind bin 200): v_mfma_f32_32x32x2_f32 with the BASIS as the A operand (row = bin, from global memory
//      in lane order: one 8-byte load per lane gives the cos and the sin value of a k-step) and the FRAMES as the B operand (column
//      = frame), 100 k-steps of two taps for Re and for Im.  The result has the lane's frame in all 16 registers and 16 bins of
//      the block in them.
//   3. SQUARE, MEL.  P = Re^2 + Im^2 in those registers IS the B operand of the next product, mel[j][f] += B[j][k] P[k][f], with no
//      lane movement: k-step r takes register r, whose bin is 8 (r >> 2) + 4 (lane >> 5) + (r & 3) of the block, and the filterbank
//      comes from global memory in exactly that order (mel_tables: fb).  Of the 7 x MB (bin block, band block) pairs only those in
//      which the filterbank has a non-zero entry are multiplied (a mask with the kernel's arguments: 9 of 21 and 11 of 28).
//   4. STORE.  log10f(max(mel, 1e-10f)), band block by band block through LDS (the samples' area, every wave a part of its own)
//      into the destination's order, and out as whole aligned 16-byte pieces; only a track's last piece of a band's row can be
//      partial and goes out as element stores.  Frames at or behind the track's F write nothing.
// No float atomics, no sum whose order depends on the launch: the same input gives the same bits.
// The stage is this kernel's own, not og_feat.hpp's feat_stage_window: pieces stay in one column of this fixed phase cut.
static_assert(sizeof(opusgpu_mel_params) == 32, "mel params layout");

constexpr int MEL_T = 128;                      // frames per tile
constexpr int MEL_Q = MEL_T + 2;                // places per phase: frame f reads places f .. f + 2
constexpr int MEL_W = (MEL_T - 1) * 160 + 400;  // samples of a tile's window
constexpr int MEL_NB = 7;                       // blocks of 32 bins
constexpr int MEL_KS = 100;                     // k-steps of two taps: taps 1 .. 200 of the folded window
static_assert(160 * MEL_Q * 2 >= 4 * 32 * MEL_STG * 4, "the store areas lie inside the samples' area");

__device__ __forceinline__ int mel_place(int p) { return (p % 160) * MEL_Q + p / 160; }

template <int MB>
__global__ void __launch_bounds__(256) k_tracks_mel(const MelTile *__restrict__ tiles, const MelSpan *__restrict__ spans,
                                                    const i16 *__restrict__ in, const float2 *__restrict__ basis,
                                                    const float *__restrict__ fb, u32 fb_mask, int n_mels, int frames_major,
                                                    float *__restrict__ out) {
    __shared__ __align__(16) i16 lds[160 * MEL_Q]; // [phase][place]; afterwards four store areas of [32][MEL_STG] floats
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MelTile tl = tiles[blockIdx.x];
    const MelSpan sp = spans[tl.track];
    const long long n = sp.in_samples;
    const long long left = n / 160 - tl.first;
    const int nf = left < MEL_T ? (int)left : MEL_T; // frames of this tile that exist
    if (nf <= 0) return;

    // 1. the window -> LDS
    const long long base = 160LL * tl.first - 200;                      // its first sample, counted from the track's; a multiple of 8
    const long long qa = base < 0 ? 0 : base;                           // the track's samples inside it: [qa, qb), qa a multiple of 8
    const long long qb = n < base + MEL_W ? n : base + MEL_W;
    {
        const i16 *const trk = in + sp.in_offset;
        for (long long k = (qa >> 3) + tid; 8 * k < qb; k += 256) {
            const uint4 v = *reinterpret_cast<const uint4 *>(trk + 8 * k);
            const u32 w32[4] = {v.x, v.y, v.z, v.w};
            const int at = mel_place((int)(8 * k - base)); // p % 160 is a multiple of 8: the piece stays in one column of places
#pragma unroll
            for (int h = 0; h < 8; h++)
                if (8 * k + h < qb) lds[at + h * MEL_Q] = (i16)(w32[h >> 1] >> (16 * (h & 1)));
        }
    }
    __syncthreads();
    {
        const int lo_n = base < 0 ? (int)-base : 0;                     // places in front of the track
        const int hi_0 = n - base < MEL_W ? (int)(n - base) : MEL_W;    // the first place behind it
        for (int x = tid; x < lo_n + (MEL_W - hi_0); x += 256) {
            const int p = x < lo_n ? x : hi_0 + (x - lo_n);
            const long long q = base + p;
            const long long r = q < 0 ? -q : 2 * (n - 1) - q;           // reflected once
            i16 s = 0;
            if (r >= qa && r < qb) s = lds[mel_place((int)(r - base))]; // places of the track: written above, not written here
            lds[mel_place(p)] = s;
        }
    }
    __syncthreads();

    // 2. and 3. 32 frames x 224 bins per wave, then the bands
    const int fl = lane & 31, kh = lane >> 5;
    const int f = wave * 32 + fl; // the lane's frame in the tile
    const float scale = sp.scale;
    og_f32x16 mel[MB];
#pragma unroll
    for (int mm = 0; mm < MB; mm++)
#pragma unroll
        for (int r = 0; r < 16; r++) mel[mm][r] = 0.f;
    for (int nb = 0; nb < MEL_NB; nb++) {
        og_f32x16 re, im;
#pragma unroll
        for (int r = 0; r < 16; r++) re[r] = 0.f, im[r] = 0.f;
        const float2 *const bp = basis + (size_t)nb * MEL_KS * 64 + lane;
#pragma unroll 4
        for (int ks = 0; ks < MEL_KS; ks++) {
            const int i = 1 + 2 * ks + kh; // the lane's tap
            const float xa = __fmul_rn((float)lds[mel_place(i) + f], scale);
            const float xb = __fmul_rn((float)lds[mel_place(400 - i) + f], scale);
            const float2 w = bp[ks * 64];
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, xa + xb, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, xa - xb, im, 0, 0, 0);
        }
        const og_f32x16 P = re * re + im * im;
#pragma unroll
        for (int mm = 0; mm < MB; mm++) {
            if ((fb_mask >> (nb * 4 + mm)) & 1) { // wave-uniform
                const float *const fp = fb + (size_t)((nb * MB + mm) * 16) * 64 + lane;
#pragma unroll
                for (int r = 0; r < 16; r++) mel[mm] = __builtin_amdgcn_mfma_f32_32x32x2f32(fp[r * 64], P[r], mel[mm], 0, 0, 0);
            }
        }
    }
    __syncthreads(); // every wave has read its last sample

    // 4. log10 and out, 32 bands at a time: register r of the lane is band 8 (r >> 2) + 4 kh + (r & 3) of the block, frame fl
    float *const stg = reinterpret_cast<float *>(lds) + wave * 32 * MEL_STG;
    const int wf = nf - wave * 32 < 32 ? nf - wave * 32 : 32; // frames of this wave that exist (may be <= 0)
    float *const dst = out + sp.out_offset;
    const long long f0 = (long long)tl.first + wave * 32;
#pragma unroll
    for (int mm = 0; mm < MB; mm++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int band = 8 * (r >> 2) + 4 * kh + (r & 3);
            const float v = log10f(fmaxf(mel[mm][r], 1e-10f));
            stg[frames_major ? fl * MEL_STG + band : band * MEL_STG + fl] = v;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; it++) { // 32 rows of 8 pieces
            const int row = (lane + 64 * it) >> 3, pc = lane & 7;
            const og_f32x4 v = *reinterpret_cast<const og_f32x4 *>(stg + row * MEL_STG + 4 * pc);
            if (frames_major) { // row: frame, piece: bands 32 mm + 4 pc .. + 3 (n_mels is a multiple of 16: whole and aligned)
                if (row < wf && 32 * mm + 4 * pc < n_mels)
                    *reinterpret_cast<og_f32x4 *>(dst + (f0 + row) * n_mels + 32 * mm + 4 * pc) = v;
            } else {            // row: band, piece: frames f0 + 4 pc .. + 3
                if (32 * mm + row < n_mels && 4 * pc < wf) {
                    float *const d = dst + (32 * mm + row) * sp.plane + f0 + 4 * pc;
                    if (4 * pc + 4 <= wf) {
                        *reinterpret_cast<og_f32x4 *>(d) = v;
                    } else {
#pragma unroll
                        for (int h = 0; h < 4; h++)
                            if (4 * pc + h < wf) d[h] = v[h];
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- tables -------------------------------------------------------------------------------------------
// Made once per process at first use, in double, rounded once (include/opusgpu.h, TRACK FEATURES, TABLES): the tables as the
// accessors hand them out, and the same numbers in the order the kernel's lanes load them.
struct MelTables {
    std::vector<float> wc, ws;   // [400][201]
    std::vector<float> bank[2];  // [n_mels][201], 80 and 128 bands
    std::vector<float> basis;    // [7][100][64 lanes][cos, sin]: tap 1 + 2 ks + (lane >> 5), bin 32 nb + (lane & 31); row 200 folded
    std::vector<float> fb[2];    // [7][MB][16][64 lanes]: band 32 mm + (lane & 31), bin 32 nb + 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
    u32 mask[2] = {0, 0};        // bit 4 nb + mm: that block of fb has a non-zero entry
};
static MelTables mel_tables_make() {
    MelTables t;
    mel_basis_make(OPUSGPU_MEL_NFFT, OPUSGPU_MEL_NFFT, t.wc, t.ws);
    const std::vector<int> all{0, 1, 2, 3, 4, 5, 6}; // the kernel walks every block
    static_assert(MEL_NB == 7 && MEL_KS == OPUSGPU_MEL_NFFT / 4, "k_tracks_mel's table");
    t.basis = feat_pack_basis(t.wc, t.ws, OPUSGPU_MEL_NFFT, all);
    for (int v = 0; v < 2; v++) {
        const int n_mels = v ? 128 : 80, MB = n_mels / 32 + (n_mels % 32 != 0);
        mel_bank_make(40.0, OPUSGPU_MEL_BINS, n_mels, false, true, OPUSGPU_MEL_FMIN, OPUSGPU_MEL_FMAX, t.bank[v]);
        t.fb[v] = feat_pack_fb(t.bank[v], OPUSGPU_MEL_BINS, n_mels, all, MB, [&](int nb, int mm) { t.mask[v] |= 1u << (4 * nb + mm); });
    }
    return t;
}
static const MelTables &mel_tables() {
    static const MelTables t = mel_tables_make();
    return t;
}

// ---- host side ----------------------------------------------------------------------------------------
static bool mel_params_ok(const opusgpu_mel_params *p) {
    if (!p || (p->n_mels != 80 && p->n_mels != 128)) return false;
    if (p->layout != OPUSGPU_MEL_BANDS_MAJOR && p->layout != OPUSGPU_MEL_FRAMES_MAJOR) return false;
    for (int32_t r : p->reserved)
        if (r) return false;
    return true;
}
static int64_t mel_plane(int64_t planned_48k) { return rs_round64((planned_48k + 2) / 3 / OPUSGPU_MEL_HOP); }

// k_tracks_mel over n tracks.  A track may have any int32 count of frames here and 0x7fffffff - T of them in tracks_melspec_run
// (og_tracks_melspec.hpp): the two bounds are kept as each call was published.  Neither kernel needs the stricter one -- both widen a
// tile's first frame to 64 bits before they add to it -- so it only keeps first + T an int32 for code that may want it so.
static int tracks_mel_run(int device, hipStream_t s, int n_tracks, const opusgpu_mel_span *spans, const void *d_in,
                          const opusgpu_mel_params *params, void *d_out, const TrackFail &hip_failed) {
    if (!mel_params_ok(params)) return OPUSGPU_BAD_ARG;
    const int v = params->n_mels == 128;
    const MelTables *tab = nullptr;
    return tracks_feature_run(
        device, s, n_tracks, spans, d_in, d_out, MEL_T, 0x7fffffff, [](int64_t n) { return n / OPUSGPU_MEL_HOP; },
        [&] {
            tab = &mel_tables();
            return FeatTables{&tab->basis, &tab->fb[v]};
        },
        [&](unsigned n_tiles, const MelTile *d_tiles, const MelSpan *d_spans, const float2 *d_basis, const float *d_fb) {
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(n_tiles), dim3(256), 0, s, d_tiles, d_spans, (const i16 *)d_in, d_basis, d_fb, tab->mask[v],
                                   (int)params->n_mels, params->layout == OPUSGPU_MEL_FRAMES_MAJOR ? 1 : 0, (float *)d_out);
            };
            if (v)
                go(k_tracks_mel<4>);
            else
                go(k_tracks_mel<3>);
        },
        hip_failed);
}

// opusgpu_files_decode_mel and its multistream twin (og_ms_tracks.hpp): files_feature_run (og_feat.hpp) at 16 kHz, through the rate branch.
static int files_mel_run(const FilesOwner &own, int mono, const opusgpu_mix_matrix *mix, const opusgpu_mel_params *params, const float *scale,
                         void *d_out, int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out) {
    FeatFlow flow;
    flow.sample_rate = mel_params_ok(params) ? OPUSGPU_MEL_SR : 0;
    flow.scratch_failed = "hipMalloc(mel scratch)";
    flow.plane = [](int64_t planned, int, int) { return mel_plane(planned); };
    flow.frames = [](int64_t len) { return len / OPUSGPU_MEL_HOP; };
    flow.layout = [=](int n, const int64_t *planned, int, int, int64_t *feat) { return opusgpu_mel_layout(n, planned, params, feat); };
    if (flow.sample_rate) flow.width = params->n_mels, flow.frames_major = params->layout == OPUSGPU_MEL_FRAMES_MAJOR;
    flow.run = [&](int n, const opusgpu_mel_span *spans, const void *d_in, void *d_feat) {
        return tracks_mel_run(own.device, own.stream, n, spans, d_in, params, d_feat, own.hip_failed);
    };
    return files_feature_run(own, OPUSGPU_MEL_SR, 0, 0, mono, mix, scale, d_out, feat_offsets, frames_out, track_lengths_out, status_out, flow);
}

extern "C" {

int opusgpu_mel_basis(const float **wc, const float **ws) {
    const MelTables &t = mel_tables();
    if (wc) *wc = t.wc.data();
    if (ws) *ws = t.ws.data();
    return OPUSGPU_MEL_NFFT * OPUSGPU_MEL_BINS;
}

int opusgpu_mel_filterbank(int n_mels, const float **b) {
    if (n_mels != 80 && n_mels != 128) return OPUSGPU_BAD_ARG;
    if (b) *b = mel_tables().bank[n_mels == 128].data();
    return n_mels * OPUSGPU_MEL_BINS;
}

int64_t opusgpu_mel_layout(int n, const int64_t *planned_48k_samples, const opusgpu_mel_params *params, int64_t *feat_offsets) {
    if (!mel_params_ok(params) || n < 0 || (n && !planned_48k_samples)) return OPUSGPU_BAD_ARG;
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        if (planned_48k_samples[i] < 0) return OPUSGPU_BAD_ARG;
        if (feat_offsets) feat_offsets[i] = at;
        at += params->n_mels * mel_plane(planned_48k_samples[i]);
    }
    return at;
}

int opusgpu_tracks_mel_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in16k_mono,
                              const opusgpu_mel_params *params, void *d_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_mel_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in16k_mono, params, d_out,
                          track_fail(ctx));
}

int opusgpu_files_decode_mel(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int mono, const opusgpu_mix_matrix *mix,
                             const opusgpu_mel_params *params, const float *scale, void *d_out, int64_t *feat_offsets, int64_t *frames_out,
                             int64_t *track_lengths_out, int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    return files_mel_run(files_owner(ctx, batch), mono, mix, params, scale, d_out, feat_offsets, frames_out, track_lengths_out, status_out);
}

} // extern "C"
