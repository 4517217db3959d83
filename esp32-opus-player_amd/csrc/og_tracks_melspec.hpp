// og_tracks_melspec.hpp -- mel spectrograms of the mono track at any rate, n_fft and hop (include/opusgpu.h, TRACK SPECTROGRAMS): the
// record's rules, the tables per parameter set, the dense kernel that turns packed int16 mono tracks into float32 feature tracks, its
// host side, the dispatch on the record's algorithm word and the whole-file call that ends in it.  Included at the end of og_api.hip
// behind og_feat.hpp, whose window stage, table builders and packers, record rules, span record, run function and whole-file
// flow it shares, and behind og_tracks_stft.hpp (fft_tables), and in front of og_ms_tracks.hpp, which holds the
// multistream twin of the whole-file call.  og_tracks_melfft.hpp, included below between the rules it reads and the dispatch that
// sends it every FFT record, holds the second algorithm of the record (k_tracks_melfft, OPUSGPU_SPEC_ALGO_FFT).
#pragma once

// ---- the record's rules -------------------------------------------------------------------------------
typedef std::tuple<int, int, int, int, int, int, float, float> SpecKey; // sample_rate, n_fft, win, n_mels, mel_scale, norm, fmin, fmax

static int spec_win(const opusgpu_spec_params &p) { return p.win_length ? p.win_length : p.n_fft; }
static SpecKey spec_key(const opusgpu_spec_params &p) {
    return SpecKey(p.sample_rate, p.n_fft, spec_win(p), p.n_mels, p.mel_scale, p.norm, p.fmin, p.fmax);
}

// The record's algorithm is reserved[1]: OPUSGPU_SPEC_ALGO_DENSE (k_tracks_melspec, below) or OPUSGPU_SPEC_ALGO_FFT (k_tracks_melfft,
// og_tracks_melfft.hpp, which holds everything the FFT records alone need: they build no Wc / Ws).
static bool spec_is_fft(const opusgpu_spec_params &p) { return p.reserved[1] == OPUSGPU_SPEC_ALGO_FFT; }

static bool spec_params_ok(const opusgpu_spec_params *p) {
    if (!p) return false;
    if (p->reserved[0] || (p->reserved[1] != OPUSGPU_SPEC_ALGO_DENSE && p->reserved[1] != OPUSGPU_SPEC_ALGO_FFT)) return false;
    if (!dft_shape_ok(p->n_fft, p->hop, p->win_length, spec_is_fft(*p))) return false;
    if (p->n_mels < 1 || p->n_mels > 128) return false;
    if (p->mel_scale != OPUSGPU_SPEC_SLANEY && p->mel_scale != OPUSGPU_SPEC_HTK) return false;
    if (p->norm != OPUSGPU_SPEC_NORM_SLANEY && p->norm != OPUSGPU_SPEC_NORM_NONE) return false;
    if (p->power != 1 && p->power != 2) return false;
    if (p->log != OPUSGPU_SPEC_LOG_NONE && p->log != OPUSGPU_SPEC_LOG10 && p->log != OPUSGPU_SPEC_LN) return false;
    if (p->frames != OPUSGPU_SPEC_FRAMES_TORCH && p->frames != OPUSGPU_SPEC_FRAMES_WHISPER) return false;
    if (p->layout != OPUSGPU_MEL_BANDS_MAJOR && p->layout != OPUSGPU_MEL_FRAMES_MAJOR) return false;
    if (p->sample_rate < 1 || p->sample_rate > 1048576) return false;
    if (!(p->fmin >= 0.f) || !(p->fmin < p->fmax) || !((double)p->fmax <= p->sample_rate / 2.0)) return false;
    if (!std::isfinite(p->floor) || p->floor < 0.f || (p->log != OPUSGPU_SPEC_LOG_NONE && !(p->floor > 0.f))) return false;
    return true;
}
static_assert(sizeof(opusgpu_spec_params) == 64, "spec params layout");

static int64_t spec_frames(const opusgpu_spec_params &p, int64_t n) {
    return feat_frames_centered(p.frames == OPUSGPU_SPEC_FRAMES_WHISPER, p.hop, n);
}

#include "og_tracks_melfft.hpp" // k_tracks_melfft, melfft_tables, melfft_tile, tracks_melfft_run

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_melspec: k_tracks_mel (og_tracks_mel.hpp, whose head comment says what the four steps are) with its constants as
// arguments.  One workgroup per entry of a tile table built on the host, a tile being T = 128, 64 or 32 consecutive frames of one
// track, 32 per wave: the workgroup has T / 32 waves.  What differs:
//   1. STAGE (og_feat.hpp: feat_stage_window).  The tile's window -- W = (T - 1) hop + n_fft samples, the first of them sample hop *
//      first - n_fft / 2 of the track -- lies in LDS cut by phase: place p is at row p % hop, column p / hop, the rows packed without
//      room between them, so a window of 32,768 samples takes 65,536 bytes whatever the hop.  The places in front of the track and
//      behind it are filled by the reflection rule from LDS -- or, where the reflected sample lies in front of the window (the last
//      frame of F = n / hop + 1 when hop divides n and that frame is its tile's first), from the track itself --, 0 outside the
//      track.  Only the places that the tile's WORKING waves read are filled.
//   2. DFT.  The fold of k_tracks_mel: taps 1 .. n_fft / 2 of u_i = x_i + x_{n_fft - i} and v_i = x_i - x_{n_fft - i} (w[0] = 0 and
//      w[i] = w[n_fft - i] for every window of the section), row n_fft / 2 halved for u and zero for v, n_fft / 4 k-steps of two
//      taps.  A lane walks its two taps' (row, column) by additions: there is no division in the loop.  Only the blocks of 32 bins
//      that a band weights are walked (the host's list: the tables hold those blocks alone), and a wave whose 32 frames all lie at or
//      behind the track's F walks none and stores nothing; it still reaches every barrier.
//   3. POWER, MEL.  S = Re^2 + Im^2 or its sqrtf, in the accumulators, is the B operand of the band product; four blocks of 32
//      bands, those without a weight in the bin block skipped (4 mask bits per kept bin block, with the kernel's arguments).
//   4. STORE.  max(mel, floor), its log10f or logf or neither, through LDS into the destination's order and out in aligned 16-byte
//      pieces where a piece is whole and aligned (frames-major rows of an n_mels that is no multiple of 4 are not: element stores).
//   Steps 3 and 4 are this kernel's own text and k_tracks_fbank's a copy of it: og_feat.hpp says why they are no shared functions.
// No float atomics, no sum whose order depends on the launch: the same input gives the same bits.
struct MsArgs {
    i32 n_fft, hop, n_mels;
    i32 n_blocks;                   // kept blocks of 32 bins
    i32 power, log, whisper_frames, frames_major;
    float floor;
    u8 mask[MS_MAXBLK + 3];         // bit mm of mask[b]: band block mm has a weight in kept bin block b
};

__global__ void __launch_bounds__(256) k_tracks_melspec(const MelTile *__restrict__ tiles, const MelSpan *__restrict__ spans,
                                                        const i16 *__restrict__ in, const float2 *__restrict__ basis,
                                                        const float *__restrict__ fb, MsArgs a, float *__restrict__ out) {
    extern __shared__ __align__(16) i16 lds[]; // the window by phase, W places (feat_window_lds_bytes); afterwards a store area of [32][MEL_STG] floats per wave
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int T = nthr >> 1, N = a.n_fft, H = a.hop;
    const MelTile tl = tiles[blockIdx.x];
    const MelSpan sp = spans[tl.track];
    const long long n = sp.in_samples;
    const long long F = a.whisper_frames ? n / H : n ? n / H + 1 : 0;
    const long long left = F - tl.first;
    const int nf = left < T ? (int)left : T; // frames of this tile that exist
    if (nf <= 0) return;
    const int waves_on = (nf + 31) >> 5;                       // waves that have a frame
    const int W = (T - 1) * H + N;                             // the tile's window, which fixes the places
    const int Wuse = (32 * waves_on - 1) * H + N;              // what the working waves read of it
    const FeatPhase ph(W, H);

    // 1. the window -> LDS: its first sample, counted from the track's, is hop * first - n_fft / 2
    feat_stage_window(lds, ph, in + sp.in_offset, n, (long long)H * tl.first - N / 2, Wuse, tid, nthr, FeatEdgeTorch());

    // 2. and 3. 32 frames per wave: the kept bin blocks, then the bands
    const int fl = lane & 31, kh = lane >> 5;
    const float scale = sp.scale;
    og_f32x16 mel[4];
#pragma unroll
    for (int mm = 0; mm < 4; mm++)
#pragma unroll
        for (int r = 0; r < 16; r++) mel[mm][r] = 0.f;
    if (wave < waves_on && a.n_blocks > 0) { // (no kept block: no band has a weight, and mel stays 0)
        const int KS = N >> 2;
        const int m2 = 2 % H, d2 = 2 / H;
        const int ia0 = 1 + kh - 2, ib0 = N - ia0;       // one step in front of the lane's first taps, 1 + kh and n_fft - 1 - kh
        const int f = wave * 32 + fl;                    // the lane's frame in the tile
        const int pa0 = ia0 < 0 ? H - 1 - ((-ia0 - 1) % H) : ia0 % H, ca0 = ia0 < 0 ? -1 - (-ia0 - 1) / H : ia0 / H;
        const int pb0 = ib0 % H, cb0 = ib0 / H;
        const int Qm = ph.Qm, Qr = ph.Qr;
        // the basis comes a k-step at a time, 512 bytes per wave, from L2 at best: requested two groups of 4 k-steps ahead of its
        // use (the table is one run over all kept blocks), or every k-step would wait out a load with nothing to hide it behind
        const int G = KS >> 2, GT = a.n_blocks * G;
        const float2 *const bp = basis + lane;
        float2 w0[4], w1[4], w2[4];
#pragma unroll
        for (int j = 0; j < 4; j++) w0[j] = bp[(size_t)j * 64], w1[j] = bp[(size_t)(4 * (GT > 1 ? 1 : 0) + j) * 64];
        int gg = 0;
        for (int b = 0; b < a.n_blocks; b++) {
            og_f32x16 re, im;
#pragma unroll
            for (int r = 0; r < 16; r++) re[r] = 0.f, im[r] = 0.f;
            int pa = pa0, ca = ca0 + f, pb = pb0, cb = cb0 + f;
            for (int g = 0; g < G; g++, gg++) {
                const int ahead = gg + 2 < GT ? gg + 2 : GT - 1;
#pragma unroll
                for (int j = 0; j < 4; j++) w2[j] = bp[(size_t)(4 * ahead + j) * 64];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    pa += m2, ca += d2;
                    if (pa >= H) pa -= H, ca++;
                    pb -= m2, cb -= d2;
                    if (pb < 0) pb += H, cb--;
                    const float xa = __fmul_rn((float)lds[pa * Qm + (pa < Qr ? pa : Qr) + ca], scale); // (ph.at(pa, ca), written out:
                    const float xb = __fmul_rn((float)lds[pb * Qm + (pb < Qr ? pb : Qr) + cb], scale); // the generated code stays what it was)
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[j].x, xa + xb, re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[j].y, xa - xb, im, 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < 4; j++) w0[j] = w1[j], w1[j] = w2[j];
            }
            og_f32x16 P = re * re + im * im;
            if (a.power == 1) {
#pragma unroll
                for (int r = 0; r < 16; r++) P[r] = sqrtf(P[r]);
            }
            const u32 mk = a.mask[b];
#pragma unroll
            for (int mm = 0; mm < 4; mm++) {
                if ((mk >> mm) & 1) { // wave-uniform
                    const float *const fp = fb + (size_t)((b * 4 + mm) * 16) * 64 + lane;
#pragma unroll
                    for (int r = 0; r < 16; r++) mel[mm] = __builtin_amdgcn_mfma_f32_32x32x2f32(fp[r * 64], P[r], mel[mm], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads(); // every wave has read its last sample

    // 4. floor, log and out, 32 bands at a time: register r of the lane is band 8 (r >> 2) + 4 kh + (r & 3) of the block, frame fl
    float *const stg = reinterpret_cast<float *>(lds) + wave * 32 * MEL_STG;
    const int wf = nf - wave * 32 < 32 ? nf - wave * 32 : 32; // frames of this wave that exist (may be <= 0)
    float *const dst = out + sp.out_offset;
    const long long f0 = (long long)tl.first + wave * 32;
    const int n_mels = a.n_mels, frames_major = a.frames_major;
    const bool whole4 = (n_mels & 3) == 0;
#pragma unroll
    for (int mm = 0; mm < 4; mm++) {
        if (32 * mm < n_mels) { // the same for every wave: the barriers inside are reached by all
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int band = 8 * (r >> 2) + 4 * kh + (r & 3);
                float v = fmaxf(mel[mm][r], a.floor);
                if (a.log == 1) v = log10f(v);
                if (a.log == 2) v = logf(v);
                stg[frames_major ? fl * MEL_STG + band : band * MEL_STG + fl] = v;
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 4; it++) { // 32 rows of 8 pieces
                const int row = (lane + 64 * it) >> 3, pc = lane & 7;
                const og_f32x4 v = *reinterpret_cast<const og_f32x4 *>(stg + row * MEL_STG + 4 * pc);
                if (frames_major) { // row: frame, piece: bands 32 mm + 4 pc .. + 3
                    const int j0 = 32 * mm + 4 * pc;
                    if (row < wf && j0 < n_mels) {
                        float *const d = dst + (f0 + row) * n_mels + j0;
                        if (whole4) {
                            *reinterpret_cast<og_f32x4 *>(d) = v;
                        } else {
#pragma unroll
                            for (int h = 0; h < 4; h++)
                                if (j0 + h < n_mels) d[h] = v[h];
                        }
                    }
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
}

// ---- tables -------------------------------------------------------------------------------------------
// TRACK SPECTROGRAMS, TABLES: made in double at first use, rounded once, kept per distinct set of the fields that reach them for the
// life of the process: the tables as the accessors hand them out, and the same numbers in the order the kernel's lanes load them.
struct SpecTables {
    int n_fft = 0, bins = 0, n_mels = 0;
    std::vector<float> wc, ws;      // [n_fft][bins]
    std::vector<float> bank;        // [n_mels][bins]
    std::vector<int> blocks;        // the blocks of 32 bins in which the bank has a non-zero entry
    std::vector<float> basis;       // [kept block][n_fft / 4][64 lanes][cos, sin]: tap 1 + 2 ks + (lane >> 5), bin 32 nb + (lane & 31)
    std::vector<float> fb;          // [kept block][4][16][64 lanes]: band 32 mm + (lane & 31), bin 32 nb + 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
    u8 mask[MS_MAXBLK + 3] = {};
};

static std::unique_ptr<SpecTables> spec_tables_make(const opusgpu_spec_params &p) {
    std::unique_ptr<SpecTables> t(new SpecTables);
    const int N = p.n_fft, bins = N / 2 + 1, n_mels = p.n_mels;
    t->n_fft = N, t->bins = bins, t->n_mels = n_mels;
    mel_basis_make(N, spec_win(p), t->wc, t->ws);
    mel_bank_make((double)p.sample_rate / N, bins, n_mels, p.mel_scale == OPUSGPU_SPEC_HTK, p.norm == OPUSGPU_SPEC_NORM_SLANEY, p.fmin, p.fmax,
                  t->bank);
    t->blocks = feat_kept_blocks(t->bank, bins, n_mels);
    t->basis = feat_pack_basis(t->wc, t->ws, N, t->blocks);
    t->fb = feat_pack_fb(t->bank, bins, n_mels, t->blocks, 4, [&](int b, int mm) { t->mask[b] |= (u8)(1u << mm); });
    return t;
}

// The tables of a dense parameter set that spec_params_ok has passed; safe from any number of threads.
static const SpecTables &spec_tables(const opusgpu_spec_params &p) {
    return feat_cached<SpecKey, SpecTables>(spec_key(p), [&] { return spec_tables_make(p); });
}

// ---- host side ----------------------------------------------------------------------------------------
// The tile in frames: of a dense record feat_dense_tile's, of an FFT record melfft_tile's.
static int spec_tile(const opusgpu_spec_params &p) { return spec_is_fft(p) ? melfft_tile(p) : feat_dense_tile(p.hop, p.n_fft); }

// k_tracks_melspec, or for an FFT record k_tracks_melfft, over n tracks (og_feat.hpp: tracks_feature_run; og_tracks_mel.hpp says why
// the frames' bound differs from tracks_mel_run's).
static int tracks_melspec_run(int device, hipStream_t s, int n_tracks, const opusgpu_mel_span *spans, const void *d_in,
                              const opusgpu_spec_params *params, void *d_out, const TrackFail &hip_failed) {
    if (!spec_params_ok(params)) return OPUSGPU_BAD_ARG;
    if (spec_is_fft(*params)) return tracks_melfft_run(device, s, n_tracks, spans, d_in, params, d_out, hip_failed);
    const int T = spec_tile(*params);
    const SpecTables *tab = nullptr;
    return tracks_feature_run(
        device, s, n_tracks, spans, d_in, d_out, T, 0x7fffffff - T, [&](int64_t n) { return spec_frames(*params, n); },
        [&] {
            tab = &spec_tables(*params);
            return FeatTables{&tab->basis, &tab->fb};
        },
        [&](unsigned n_tiles, const MelTile *d_tiles, const MelSpan *d_spans, const float2 *d_basis, const float *d_fb) {
            MsArgs a{};
            a.n_fft = params->n_fft, a.hop = params->hop, a.n_mels = params->n_mels, a.n_blocks = (i32)tab->blocks.size();
            a.power = params->power, a.log = params->log, a.whisper_frames = params->frames == OPUSGPU_SPEC_FRAMES_WHISPER;
            a.frames_major = params->layout == OPUSGPU_MEL_FRAMES_MAJOR, a.floor = params->floor;
            std::copy(std::begin(tab->mask), std::end(tab->mask), a.mask);
            hipLaunchKernelGGL(k_tracks_melspec, dim3(n_tiles), dim3(2 * T), feat_window_lds_bytes(params->hop, params->n_fft, T, true), s,
                               d_tiles, d_spans, (const i16 *)d_in, d_basis, d_fb, a, (float *)d_out);
        },
        hip_failed);
}

// opusgpu_files_decode_melspec and its multistream twin (og_ms_tracks.hpp): files_feature_run at the record's rate.
static int files_melspec_run(const FilesOwner &own, int rate, int up, int down, int mono, const opusgpu_mix_matrix *mix,
                             const opusgpu_spec_params *params, const float *scale, void *d_out, int64_t *feat_offsets, int64_t *frames_out,
                             int64_t *track_lengths_out, int32_t *status_out) {
    const bool ok = spec_params_ok(params);
    const FeatFlow flow = feat_record_flow(
        ok, ok ? (int)params->sample_rate : 0, ok ? params->n_mels : 0, ok && params->layout == OPUSGPU_MEL_FRAMES_MAJOR,
        "hipMalloc(spectrogram scratch)", [=](int64_t len) { return spec_frames(*params, len); },
        [=](int n, const int64_t *planned, int u, int d, int64_t *feat) { return opusgpu_spec_layout(n, planned, u, d, params, feat); },
        [&own, params](int n, const opusgpu_mel_span *spans, const void *d_in, void *d_feat) {
            return tracks_melspec_run(own.device, own.stream, n, spans, d_in, params, d_feat, own.hip_failed);
        });
    return files_feature_run(own, rate, up, down, mono, mix, scale, d_out, feat_offsets, frames_out, track_lengths_out, status_out, flow);
}

extern "C" {

int opusgpu_spec_basis(const opusgpu_spec_params *p, const float **wc, const float **ws) {
    if (!spec_params_ok(p) || spec_is_fft(*p)) return OPUSGPU_BAD_ARG; // (an FFT record multiplies no Wc / Ws and builds none)
    const SpecTables &t = spec_tables(*p);
    if (wc) *wc = t.wc.data();
    if (ws) *ws = t.ws.data();
    return t.n_fft * t.bins;
}

int opusgpu_spec_filterbank(const opusgpu_spec_params *p, const float **b) {
    if (!spec_params_ok(p)) return OPUSGPU_BAD_ARG;
    if (spec_is_fft(*p)) {
        const std::vector<float> &bank = melfft_tables(*p).bank;
        if (b) *b = bank.data();
        return (int)bank.size();
    }
    const SpecTables &t = spec_tables(*p);
    if (b) *b = t.bank.data();
    return t.n_mels * t.bins;
}

int opusgpu_spec_tile(const opusgpu_spec_params *p) { return spec_params_ok(p) ? spec_tile(*p) : OPUSGPU_BAD_ARG; }

int64_t opusgpu_spec_layout(int n, const int64_t *planned_48k_samples, int up, int down, const opusgpu_spec_params *p, int64_t *feat_offsets) {
    if (!spec_params_ok(p)) return OPUSGPU_BAD_ARG;
    return feat_grid_layout(n, planned_48k_samples, up, down, p->n_mels, [=](int64_t len) { return spec_frames(*p, len); }, feat_offsets);
}

int opusgpu_tracks_melspec_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in_mono,
                                  const opusgpu_spec_params *p, void *d_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_melspec_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in_mono, p, d_out,
                              track_fail(ctx));
}

int opusgpu_files_decode_melspec(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int up, int down, int mono,
                                 const opusgpu_mix_matrix *mix, const opusgpu_spec_params *p, const float *scale, void *d_out,
                                 int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    return files_melspec_run(files_owner(ctx, batch), rate, up, down, mono, mix, p, scale, d_out, feat_offsets, frames_out, track_lengths_out,
                             status_out);
}

} // extern "C"
