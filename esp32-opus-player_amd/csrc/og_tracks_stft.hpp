// og_tracks_stft.hpp -- linear and complex STFT spectrograms of the mono track at any rate, n_fft and hop (include/opusgpu.h, TRACK
// STFT): the record's rules, the table per (n_fft, win_length), the dense kernel that turns packed int16 mono tracks into float32
// spectrogram tracks, its host side, the dispatch on the record's algorithm word and the whole-file call that ends in it.  Included
// at the end of og_api.hip behind og_feat.hpp, whose window stage, basis builder and packer, tile rule, span record, run function
// and whole-file flow it shares, and in front of og_ms_tracks.hpp, which holds the multistream twin of the whole-file call.
// og_tracks_fft.hpp, included below between the rules it reads and the dispatch that sends it every FFT record, holds the second
// algorithm of the record (k_tracks_fft, OPUSGPU_STFT_ALGO_FFT).
#pragma once

// ---- the record's rules -------------------------------------------------------------------------------
static int stft_win(const opusgpu_stft_params &p) { return p.win_length ? p.win_length : p.n_fft; }

// The record's algorithm is reserved[1]: OPUSGPU_STFT_ALGO_DENSE (k_tracks_stft, below) or OPUSGPU_STFT_ALGO_FFT (k_tracks_fft,
// og_tracks_fft.hpp, which holds everything the FFT records alone need).
static bool stft_is_fft(const opusgpu_stft_params &p) { return p.reserved[1] == OPUSGPU_STFT_ALGO_FFT; }

static bool stft_params_ok(const opusgpu_stft_params *p) {
    if (!p) return false;
    if (p->sample_rate < 1 || p->sample_rate > 1048576) return false;
    if (p->reserved[1] != OPUSGPU_STFT_ALGO_DENSE && p->reserved[1] != OPUSGPU_STFT_ALGO_FFT) return false;
    if (!dft_shape_ok(p->n_fft, p->hop, p->win_length, stft_is_fft(*p))) return false;
    if (p->power != OPUSGPU_STFT_COMPLEX && p->power != 1 && p->power != 2) return false;
    if (p->log != OPUSGPU_SPEC_LOG_NONE && p->log != OPUSGPU_SPEC_LOG10 && p->log != OPUSGPU_SPEC_LN) return false;
    if (p->power == OPUSGPU_STFT_COMPLEX && p->log != OPUSGPU_SPEC_LOG_NONE) return false;
    if (p->frames != OPUSGPU_SPEC_FRAMES_TORCH && p->frames != OPUSGPU_SPEC_FRAMES_WHISPER) return false;
    if (p->layout != OPUSGPU_MEL_BANDS_MAJOR && p->layout != OPUSGPU_MEL_FRAMES_MAJOR) return false;
    if (!std::isfinite(p->floor) || p->floor < 0.f || (p->log != OPUSGPU_SPEC_LOG_NONE && !(p->floor > 0.f))) return false;
    for (int i = 0; i < 7; i++)
        if (i != 1 && p->reserved[i]) return false;
    return true;
}
static_assert(sizeof(opusgpu_stft_params) == 64, "stft params layout");

static int64_t stft_frames(const opusgpu_stft_params &p, int64_t n) {
    return feat_frames_centered(p.frames == OPUSGPU_SPEC_FRAMES_WHISPER, p.hop, n);
}
static int stft_width(const opusgpu_stft_params &p) { return (p.n_fft / 2 + 1) * (p.power == OPUSGPU_STFT_COMPLEX ? 2 : 1); }

#include "og_tracks_fft.hpp" // k_tracks_fft, fft_tables, fft_tile, tracks_fft_run

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_stft<FM>: steps 1 and 2 of k_tracks_melspec (og_tracks_melspec.hpp, whose head comment says what they are; the stage is
// og_feat.hpp's, the DFT loop a copy with this kernel's operands) over EVERY block of 32 bins, and a second half of its own.  One
// workgroup of 256 threads per tile of 128, 64 or 32 frames; all four waves stage the window, then share out the tile's groups of
// 32 frames that exist and, where those are fewer than four, the bin blocks (below): a dense DFT has blocks to spare.
//   3. FINISH, STORE.  The accumulators of a bin block are finished (Re^2 + Im^2, its sqrtf, the floor, a log; or left as the pair)
//      and stored straight from the registers after every block, while the window is still live in LDS: there is no store area, so
//      the launch asks for the window alone and the tile rule is k_tracks_melspec's (feat_dense_tile).  What makes that coalesce is the
//      ORDER OF THE MFMA'S OPERANDS, which is the template argument.  Both operands are held the same way -- lane l has tap l >> 5 of
//      bin or frame l & 31 -- so swapping them transposes the result at no cost:
//        FM false (bins-major): A = basis, B = frames.  Register r of lane l is bin 8 (r >> 2) + 4 (l >> 5) + (r & 3) of the block,
//        frame l & 31: lanes 0 .. 31 store 32 consecutive frames of one bin row, one aligned 128-byte line (planes are multiples of
//        64 frames, tiles of 32), 256 bytes for pairs.
//        FM true (frames-major): A = frames, B = basis.  Register r of lane l is frame 8 (r >> 2) + 4 (l >> 5) + (r & 3) of the
//        wave, bin l & 31 of the block: lanes 0 .. 31 store 32 consecutive bins of one frame's row, 128 or 256 contiguous bytes (the
//        rows of 32 m + 1 bins are not aligned, which contiguous 4- and 8-byte stores do not need).
//      The last block holds the Nyquist bin alone (bins = 32 m + 1; the packed table is 0 behind it) and stores that one row.
//   Im carries torch.stft's sign: the table's sine is +w sin(a), so the second product takes x_{n_fft - i} - x_i, not x_i - x_{n_fft
//   - i}; with that operand an all-zero track leaves +0 in both accumulators whatever the scale's sign (-0 - -0 = +0 - +0 = +0).
// Waves without a frame group or a block walk nothing and store nothing; they have reached both barriers of step 1 by then, and
// there is none after.  Which wave computes a cell does not change its sum: the bits are those of any other sharing.
// No float atomics, no sum whose order depends on the launch: the same input gives the same bits.
struct StftArgs {
    i32 n_fft, hop, bins, tile;     // tile: frames of a tile, 128, 64 or 32; the workgroup has 256 threads whatever it is
    i32 n_blocks;                   // blocks of 32 bins: n_fft / 64 + 1
    i32 power, log, whisper_frames; // power 0: pairs
    float floor;
};

template <bool FM>
__global__ void __launch_bounds__(256) k_tracks_stft(const MelTile *__restrict__ tiles, const MelSpan *__restrict__ spans,
                                                     const i16 *__restrict__ in, const float2 *__restrict__ basis, StftArgs a,
                                                     float *__restrict__ out) {
    extern __shared__ __align__(16) i16 lds[]; // the window by phase, W places (feat_window_lds_bytes)
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.tile, N = a.n_fft, H = a.hop;
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
    // The workgroup's four waves share out the tile's groups of 32 frames that exist AND the bin blocks: with 1, 2 or 3 - 4 groups
    // a wave takes every 4th, every 2nd or every block of its group.  A tile of 32 frames, and the one tile of a short track, so
    // keep all four SIMDs at work on one window.  (The last barrier is behind every wave: one without work leaves here.)
    const int nfg = waves_on <= 1 ? 1 : waves_on == 2 ? 2 : 4, S = (nthr >> 6) / nfg;
    const int fg = wave & (nfg - 1), split = wave / nfg;   // the wave's frame group, and its first block
    const int nmine = (a.n_blocks - split + S - 1) / S;    // its blocks: split, split + S, ...
    if (fg >= waves_on || nmine <= 0) return;

    // 2. and 3. 32 frames per wave: its bin blocks, each finished and stored as it is done
    const int fl = lane & 31, kh = lane >> 5;
    const float scale = sp.scale;
    const int wf = nf - fg * 32 < 32 ? nf - fg * 32 : 32; // frames of this group that exist: 1 .. 32
    const long long f0 = (long long)tl.first + fg * 32;
    float *const dst = out + sp.out_offset;
    const long long plane = sp.plane;
    const int bins = a.bins, power = a.power, log = a.log;
    const float floor = a.floor;
    const int KS = N >> 2;
    const int m2 = 2 % H, d2 = 2 / H;
    const int ia0 = 1 + kh - 2, ib0 = N - ia0;       // one step in front of the lane's first taps, 1 + kh and n_fft - 1 - kh
    const int f = fg * 32 + fl;                      // the lane's frame in the tile
    const int pa0 = ia0 < 0 ? H - 1 - ((-ia0 - 1) % H) : ia0 % H, ca0 = ia0 < 0 ? -1 - (-ia0 - 1) / H : ia0 / H;
    const int pb0 = ib0 % H, cb0 = ib0 / H;
    // the basis two groups of 4 k-steps ahead of its use, as in k_tracks_melspec: group g of block b is entry b G + g of the table,
    // and (ab, ag) walks the wave's own blocks two groups ahead (G >= 4: n_fft >= 64), resting on its last group at the end
    const int G = KS >> 2, last_b = split + S * (nmine - 1);
    const float2 *const bp = basis + lane;
    float2 w0[4], w1[4], w2[4];
#pragma unroll
    for (int j = 0; j < 4; j++) w0[j] = bp[(size_t)(4 * (split * G) + j) * 64], w1[j] = bp[(size_t)(4 * (split * G + 1) + j) * 64];
    int ab = split, ag = 2;
    for (int b = split; b < a.n_blocks; b += S) {
        og_f32x16 re, im;
#pragma unroll
        for (int r = 0; r < 16; r++) re[r] = 0.f, im[r] = 0.f;
        int pa = pa0, ca = ca0 + f, pb = pb0, cb = cb0 + f;
        for (int g = 0; g < G; g++) {
            const int ahead = ab * G + ag;
            if (++ag == G) {
                ag = 0, ab += S;
                if (ab > last_b) ab = last_b, ag = G - 1;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) w2[j] = bp[(size_t)(4 * ahead + j) * 64];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                pa += m2, ca += d2;
                if (pa >= H) pa -= H, ca++;
                pb -= m2, cb -= d2;
                if (pb < 0) pb += H, cb--;
                const float xa = __fmul_rn((float)lds[ph.at(pa, ca)], scale);
                const float xb = __fmul_rn((float)lds[ph.at(pb, cb)], scale);
                if (FM) {
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(xa + xb, w0[j].x, re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(xb - xa, w0[j].y, im, 0, 0, 0);
                } else {
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[j].x, xa + xb, re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[j].y, xb - xa, im, 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) w0[j] = w1[j], w1[j] = w2[j];
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int sub = 8 * (r >> 2) + 4 * kh + (r & 3);   // the register's row of the 32 x 32 result
            const int k = 32 * b + (FM ? fl : sub), fr = FM ? sub : fl;
            if (k < bins && fr < wf) {
                const long long cell = FM ? (f0 + fr) * bins + k : k * plane + f0 + fr;
                if (power == 0) {
                    *reinterpret_cast<float2 *>(dst + 2 * cell) = make_float2(re[r], im[r]);
                } else {
                    float v = re[r] * re[r] + im[r] * im[r];
                    if (power == 1) v = sqrtf(v);
                    v = fmaxf(v, floor);
                    if (log == 1) v = log10f(v);
                    if (log == 2) v = logf(v);
                    dst[cell] = v;
                }
            }
        }
    }
}

// ---- table --------------------------------------------------------------------------------------------
// TRACK STFT, TABLES: made in double at first use, rounded once, kept per (n_fft, win_length) for the life of the process: Wc and Ws
// as the accessor hands them out (mel_basis_make, as for opusgpu_spec_basis), and the same numbers in the order the kernel's lanes
// load them, every block of 32 bins in turn.
struct StftTables {
    int n_fft = 0, bins = 0, n_blocks = 0;
    std::vector<float> wc, ws;      // [n_fft][bins]
    std::vector<float> basis;       // [block][n_fft / 4][64 lanes][cos, sin] (feat_pack_basis)
    std::vector<float> none;        // tracks_feature_run's second table: this kernel has no filterbank
};

// The tables of a parameter set that stft_params_ok has passed; safe from any number of threads.
static const StftTables &stft_tables(const opusgpu_stft_params &p) {
    return feat_cached<std::pair<int, int>, StftTables>({p.n_fft, stft_win(p)}, [&] {
        std::unique_ptr<StftTables> t(new StftTables);
        t->n_fft = p.n_fft, t->bins = p.n_fft / 2 + 1, t->n_blocks = (t->bins + 31) / 32;
        mel_basis_make(p.n_fft, stft_win(p), t->wc, t->ws);
        std::vector<int> all((size_t)t->n_blocks);
        for (int nb = 0; nb < t->n_blocks; nb++) all[(size_t)nb] = nb;
        t->basis = feat_pack_basis(t->wc, t->ws, p.n_fft, all);
        return t;
    });
}

// ---- host side ----------------------------------------------------------------------------------------
// The tile in frames: of a dense record feat_dense_tile's -- the launch's LDS is the window alone, since the kernel stores from its
// accumulators --, of an FFT record fft_tile's.
static int stft_tile(const opusgpu_stft_params &p) { return stft_is_fft(p) ? fft_tile(p) : feat_dense_tile(p.hop, p.n_fft); }

// k_tracks_stft, or for an FFT record k_tracks_fft, over n tracks (og_feat.hpp: tracks_feature_run; the frames' bound is
// tracks_melspec_run's).
static int tracks_stft_run(int device, hipStream_t s, int n_tracks, const opusgpu_mel_span *spans, const void *d_in,
                           const opusgpu_stft_params *params, void *d_out, const TrackFail &hip_failed) {
    if (!stft_params_ok(params)) return OPUSGPU_BAD_ARG;
    if (stft_is_fft(*params)) return tracks_fft_run(device, s, n_tracks, spans, d_in, params, d_out, hip_failed);
    const int T = stft_tile(*params);
    const StftTables *tab = nullptr;
    return tracks_feature_run(
        device, s, n_tracks, spans, d_in, d_out, T, 0x7fffffff - T, [&](int64_t n) { return stft_frames(*params, n); },
        [&] {
            tab = &stft_tables(*params);
            return FeatTables{&tab->basis, &tab->none};
        },
        [&](unsigned n_tiles, const MelTile *d_tiles, const MelSpan *d_spans, const float2 *d_basis, const float *) {
            StftArgs a{};
            a.n_fft = params->n_fft, a.hop = params->hop, a.bins = tab->bins, a.tile = T, a.n_blocks = tab->n_blocks;
            a.power = params->power, a.log = params->log, a.whisper_frames = params->frames == OPUSGPU_SPEC_FRAMES_WHISPER;
            a.floor = params->floor;
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(n_tiles), dim3(256), feat_window_lds_bytes(params->hop, params->n_fft, T, false), s, d_tiles,
                                   d_spans, (const i16 *)d_in, d_basis, a, (float *)d_out);
            };
            if (params->layout == OPUSGPU_MEL_FRAMES_MAJOR)
                go(k_tracks_stft<true>);
            else
                go(k_tracks_stft<false>);
        },
        hip_failed);
}

// STFT BATCHES (og_stft_batch.hpp, behind this header): the stage that turns a packed grid into the dense tensor, and the pad cells
// of the direct path.
static const char *stft_batch_shape_wrong(const opusgpu_stft_batch_req &r, int affine_bins, int bins, int c);
static int stft_batch_run(int device, hipStream_t s, int n_tracks, const opusgpu_stft_batch_span *spans, int bins, int c, int layout,
                          const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid, void *d_out,
                          const TrackFail &hip_failed, const std::function<void(const char *)> &why);
static int stft_pad_run(int device, hipStream_t s, int n_tracks, const int64_t *frames, int bins, int c, int layout,
                        const opusgpu_stft_batch_req &req, void *d_out, const TrackFail &hip_failed);

// opusgpu_files_decode_stft and its multistream twin (og_ms_tracks.hpp): files_feature_run at the record's rate.  FEATURE BATCHES
// hold widths of 1 - 128, which most of these are not: a request on the decoder is refused whole, before any device work.  STFT
// BATCHES: with the owner's request on, the result is the dense tensor -- by the direct path (norm NONE and a stride of a multiple of
// 64 frames: k_tracks_stft writes the tensor as its grid, k_stft_pad the cells behind every track's frames) or through a scratch grid.
static int files_stft_run(const FilesOwner &own, int rate, int up, int down, int mono, const opusgpu_mix_matrix *mix,
                          const opusgpu_stft_params *params, const float *scale, void *d_out, int64_t *feat_offsets, int64_t *frames_out,
                          int64_t *track_lengths_out, int32_t *status_out) {
    if (own.fbatch && own.fbatch->req.enabled) {
        if (own.refused) own.refused("feature batch: STFT spectrograms are not batched (widths of 1 - 128 only)");
        return OPUSGPU_BAD_ARG;
    }
    const bool ok = stft_params_ok(params);
    FeatFlow flow = feat_record_flow(
        ok, ok ? (int)params->sample_rate : 0, ok ? stft_width(*params) : 0, ok && params->layout == OPUSGPU_MEL_FRAMES_MAJOR,
        "hipMalloc(stft scratch)", [=](int64_t len) { return stft_frames(*params, len); },
        [=](int n, const int64_t *planned, int u, int d, int64_t *feat) { return opusgpu_stft_layout(n, planned, u, d, params, feat); },
        [&own, params](int n, const opusgpu_mel_span *spans, const void *d_in, void *d_feat) {
            return tracks_stft_run(own.device, own.stream, n, spans, d_in, params, d_feat, own.hip_failed);
        });
    const StftBatchState *sb = own.sbatch && own.sbatch->req.enabled && flow.sample_rate ? own.sbatch : nullptr;
    FeatDense dense;
    if (sb) {
        const int bins = params->n_fft / 2 + 1, c = params->power == OPUSGPU_STFT_COMPLEX ? 2 : 1, layout = params->layout;
        dense.stride = sb->req.stride_frames;
        dense.direct = sb->req.norm == OPUSGPU_FEAT_NORM_NONE && dense.stride % 64 == 0;
        dense.wrong = stft_batch_shape_wrong(sb->req, (int)sb->sub.size(), bins, c);
        dense.stride_short = "stft batch: stride_frames is below the frames of a track's planned length";
        dense.run = [&own, sb, bins, c, layout](int n, const opusgpu_feat_span *cells, const void *d_grid, void *d_dense) {
            if (!d_grid) {
                std::vector<int64_t> frames((size_t)n);
                for (int i = 0; i < n; i++) frames[(size_t)i] = cells[i].frames;
                return stft_pad_run(own.device, own.stream, n, frames.data(), bins, c, layout, sb->req, d_dense, own.hip_failed);
            }
            std::vector<opusgpu_stft_batch_span> spans((size_t)n);
            for (int i = 0; i < n; i++) spans[(size_t)i] = opusgpu_stft_batch_span{cells[i].grid_offset, cells[i].plane, cells[i].frames};
            return stft_batch_run(own.device, own.stream, n, spans.data(), bins, c, layout, &sb->req, sb->sub.data(), sb->mul.data(), d_grid,
                                  d_dense, own.hip_failed, own.refused);
        };
        flow.dense = &dense;
    }
    return files_feature_run(own, rate, up, down, mono, mix, scale, d_out, feat_offsets, frames_out, track_lengths_out, status_out, flow);
}

extern "C" {

int opusgpu_stft_basis(const opusgpu_stft_params *p, const float **wc, const float **ws) {
    if (!stft_params_ok(p) || p->n_fft > 2048) return OPUSGPU_BAD_ARG; // (above 2048 only the FFT runs, which multiplies no Wc / Ws)
    const StftTables &t = stft_tables(*p);
    if (wc) *wc = t.wc.data();
    if (ws) *ws = t.ws.data();
    return t.n_fft * t.bins;
}

int opusgpu_stft_tile(const opusgpu_stft_params *p) { return stft_params_ok(p) ? stft_tile(*p) : OPUSGPU_BAD_ARG; }

int64_t opusgpu_stft_layout(int n, const int64_t *planned_48k_samples, int up, int down, const opusgpu_stft_params *p, int64_t *feat_offsets) {
    if (!stft_params_ok(p)) return OPUSGPU_BAD_ARG;
    return feat_grid_layout(n, planned_48k_samples, up, down, stft_width(*p), [=](int64_t len) { return stft_frames(*p, len); }, feat_offsets);
}

int opusgpu_tracks_stft_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in_mono,
                               const opusgpu_stft_params *p, void *d_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_stft_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in_mono, p, d_out,
                           track_fail(ctx));
}

int opusgpu_files_decode_stft(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int up, int down, int mono,
                              const opusgpu_mix_matrix *mix, const opusgpu_stft_params *p, const float *scale, void *d_out,
                              int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    return files_stft_run(files_owner(ctx, batch), rate, up, down, mono, mix, p, scale, d_out, feat_offsets, frames_out, track_lengths_out,
                          status_out);
}

} // extern "C"
