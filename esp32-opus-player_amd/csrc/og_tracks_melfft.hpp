// og_tracks_melfft.hpp -- TRACK SPECTROGRAMS by FFT (include/opusgpu.h, TRACK SPECTROGRAMS, OPUSGPU_SPEC_ALGO_FFT): the tables of an
// FFT record -- the filterbank, its sparse form, and the window and twiddles that TRACK STFT's FFT records use --, the kernel that
// turns packed int16 mono tracks into float32 mel tracks for n_fft = 64 .. 8192, and its host side.  Included by
// og_tracks_melspec.hpp behind the record's rules, which this header reads, and in front of tracks_melspec_run, which sends every FFT
// record here; behind og_tracks_fft.hpp, whose load, passes and split it calls and whose table cache it shares.  The whole-file
// calls, the layout and FEATURE BATCHES are og_tracks_melspec.hpp's.
#pragma once

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_melfft: one workgroup of 256 threads per tile of T consecutive frames of one track (melfft_tile: a multiple of 32), over
// the MelTile / MelSpan tables of tracks_feature_run.  P = min(256, M / 4) threads hold one frame, M = n_fft / 2, so C = 256 / P
// frames are in flight (32 at n_fft 64, one from 2048 up), as in k_tracks_fft, and a tile takes ceil(frames / C) rounds of:
//   1. LOAD and 2. PASSES: fft_load and fft_passes of og_tracks_fft.hpp, from the same tables.
//   3. POWER.  The thread that holds k in [0, M / 2] makes X[k] and X[M - k] (fft_bin) -- both come from Z[k] and Z[M - k] alone, and
//      no other thread reads either -- and puts S = Re^2 + Im^2, or its sqrtf, where they stood: S[k] in the first half of place k
//      for k < M, S[M] in the second half of place 0.  No floor here.  A barrier.
//   4. BANK.  The work items are the (frame in flight, band) pairs, the band fastest; each goes to G consecutive lanes (a power of
//      two from the host, so that C n_mels G fills the 256 threads where it can), which stride the band's run of weights -- from
//      its first to its last non-zero entry of the filterbank, zeros inside included -- with one fmaf per entry, and are summed by
//      a butterfly over xor 1, 2, .. G / 2 of the lane: the order is a function of G and the band's record, so of the record and
//      the band alone.  max(mel, floor), its log10f or logf or neither, into the store area.
//   5. STORE, after every 32 frames of the tile and after its last: the store area holds 32 frames.  Bands-major: rows of 32 frames
//      (MEL_STG floats apart), out in aligned 16-byte pieces, element stores at the track's ragged end; a full row is one 128-byte
//      line, since planes are multiples of 64 and a tile's groups begin at multiples of 32 frames.  Frames-major: the group's cells
//      are one run of frames x n_mels floats that begins at a multiple of 128 bytes, whatever n_mels is: out in aligned 16-byte
//      pieces, element stores for the run's last 1 - 3 floats.
// LDS: the C buffers of k_tracks_fft (8,448 bytes up to n_fft 2048, 16,896 at 4096, 33,792 at 8192) and a store area of n_mels x
// MEL_STG floats (18,432 bytes at 128 bands): 52,224 bytes at most.  No float atomics, no sum whose order depends on the launch.
struct MelFftArgs {
    i32 n_fft, hop, n_mels, tile;
    i32 log2m;                      // log2 of M = n_fft / 2: 5 .. 12
    i32 log2g;                      // log2 of G, the lanes of a work item: 0 .. 6
    i32 power, log, whisper_frames, frames_major;
    float floor;
};

__global__ void __launch_bounds__(256) k_tracks_melfft(const MelTile *__restrict__ tiles, const MelSpan *__restrict__ spans,
                                                       const i16 *__restrict__ in, const float2 *__restrict__ twiddle_window,
                                                       const float *__restrict__ bands_weights, MelFftArgs a, float *__restrict__ out) {
    extern __shared__ __align__(16) float2 fft_lds[]; // C buffers of fft_place(M) places, then the store area (melfft_lds_bytes)
    const int tid = (int)threadIdx.x;
    const int N = a.n_fft, H = a.hop, L = a.log2m, M = 1 << L, T = a.tile;
    const int P = M / 4 < 256 ? M / 4 : 256, C = 256 / P, S = fft_place(M);
    const int cs = __ffs(C) - 1;            // C and P are powers of two
    const int slot = tid >> (8 - cs), t = tid & (P - 1);
    const MelTile tl = tiles[blockIdx.x];
    const MelSpan sp = spans[tl.track];
    const long long n = sp.in_samples;
    const long long F = a.whisper_frames ? n / H : n ? n / H + 1 : 0;
    const long long left = F - tl.first;
    const int nf = left < T ? (int)left : T; // frames of this tile that exist
    if (nf <= 0) return;
    const i16 *const trk = in + sp.in_offset;
    const float scale = sp.scale;
    float *const dst = out + sp.out_offset;
    const long long plane = sp.plane;
    const int n_mels = a.n_mels, power = a.power, log = a.log, frames_major = a.frames_major;
    const float floor = a.floor;
    const float2 *const twiddle = twiddle_window;                                        // [M] of the n_fft-point table
    const float *const window = reinterpret_cast<const float *>(twiddle_window + M);     // [n_fft]
    const int4 *const bands = reinterpret_cast<const int4 *>(bands_weights);             // [n_mels]: first bin, count, offset
    const float *const weights = bands_weights + 4 * n_mels;
    float2 *const buf = fft_lds + slot * S;
    float *const stg = reinterpret_cast<float *>(fft_lds + C * S);
    const int G = 1 << a.log2g, items = C * n_mels;

    for (int r0 = 0; r0 < nf; r0 += C) { // a round: frames r0 .. r0 + C - 1 of the tile, those that exist
        // 1. load, 2. passes (a slot without a frame runs them over what its buffer holds; nothing of it is used)
        if (r0 + slot < nf) fft_load(buf, trk, n, scale, window, (long long)H * (tl.first + r0 + slot) - N / 2, t, P, L);
        __syncthreads();
        fft_passes(buf, twiddle, t, P, L);
        // 3. power, in place
        if (r0 + slot < nf) {
            float *const sb = reinterpret_cast<float *>(buf);
            for (int k = t; k <= M / 2; k += P) {
                float re, im, re2, im2;
                fft_bin(buf, twiddle, M, k, re, im);
                fft_bin(buf, twiddle, M, M - k, re2, im2);
                float s1 = re * re + im * im, s2 = re2 * re2 + im2 * im2;
                if (power == 1) s1 = sqrtf(s1), s2 = sqrtf(s2);
                sb[2 * fft_place(k)] = s1;
                if (k == 0)
                    sb[1] = s2;                          // S[M]
                else if (k < M / 2)
                    sb[2 * fft_place(M - k)] = s2;
            }
        }
        __syncthreads();
        // 4. bank
        for (int i0 = 0; i0 < items; i0 += 256 >> a.log2g) { // (every lane of a wave reaches the shuffles)
            const int item = i0 + (tid >> a.log2g), g = tid & (G - 1);
            const int c = item / n_mels, band = item - c * n_mels;
            const bool on = item < items && r0 + c < nf;
            float acc = 0.f;
            if (on) {
                const int4 rec = bands[band];
                const float *const sb = reinterpret_cast<const float *>(fft_lds + c * S);
                const float *const w = weights + rec.z;
                for (int i = g; i < rec.y; i += G) {
                    const int k = rec.x + i;
                    acc = fmaf(w[i], sb[k < M ? 2 * fft_place(k) : 1], acc);
                }
            }
            for (int m = 1; m < G; m <<= 1) acc += __shfl_xor(acc, m, 64);
            if (on && g == 0) {
                float v = fmaxf(acc, floor);
                if (log == 1) v = log10f(v);
                if (log == 2) v = logf(v);
                const int fr = (r0 + c) & 31;
                stg[frames_major ? fr * n_mels + band : band * MEL_STG + fr] = v;
            }
        }
        __syncthreads(); // the next round loads over what this one read; the store area is whole
        // 5. store a group of 32 frames
        if (((r0 + C) & 31) == 0 || r0 + C >= nf) {
            const int g0 = r0 & ~31;
            const int wf = nf - g0 < 32 ? nf - g0 : 32;    // frames of the group that exist
            const long long f0 = (long long)tl.first + g0; // a multiple of 32
            if (frames_major) {
                const int cnt = wf * n_mels;
                float *const d = dst + f0 * n_mels;
                for (int x = 4 * tid; x < cnt; x += 1024) {
                    if (x + 4 <= cnt) {
                        *reinterpret_cast<og_f32x4 *>(d + x) = *reinterpret_cast<const og_f32x4 *>(stg + x);
                    } else {
                        for (int h = x; h < cnt; h++) d[h] = stg[h];
                    }
                }
            } else {
                for (int x = tid; x < 8 * n_mels; x += 256) { // rows of 8 pieces
                    const int row = x >> 3, pc = x & 7;
                    if (4 * pc < wf) {
                        const og_f32x4 v = *reinterpret_cast<const og_f32x4 *>(stg + row * MEL_STG + 4 * pc);
                        float *const d = dst + row * plane + f0 + 4 * pc;
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
            // (the next write of the store area lies behind the barriers of the next round's load and passes)
        }
    }
}

// ---- tables -------------------------------------------------------------------------------------------
// TRACK SPECTROGRAMS, the tables of an FFT record: B as opusgpu_spec_filterbank hands it out, by mel_bank_make as for a dense record,
// and the two buffers the kernel reads, kept per SpecKey for the life of the process.  No Wc, no Ws.
struct MelFftTables {
    std::vector<float> bank;            // [n_mels][bins]
    std::vector<float> twiddle_window;  // fft_tables' twiddle [n_fft / 2][cos, sin], then its window [n_fft]
    std::vector<float> bands_weights;   // [n_mels] x (first bin, count, offset, 0) as int32, then the runs' weights
};

// The tables of an FFT record that spec_params_ok has passed; safe from any number of threads.
static const MelFftTables &melfft_tables(const opusgpu_spec_params &p) {
    const FftTables &ft = fft_tables(p.n_fft, spec_win(p)); // (taken in front of this cache's lock, not under it)
    return feat_cached<SpecKey, MelFftTables>(spec_key(p), [&] {
        std::unique_ptr<MelFftTables> t(new MelFftTables);
        const int bins = p.n_fft / 2 + 1, n_mels = p.n_mels;
        mel_bank_make((double)p.sample_rate / p.n_fft, bins, n_mels, p.mel_scale == OPUSGPU_SPEC_HTK, p.norm == OPUSGPU_SPEC_NORM_SLANEY, p.fmin,
                      p.fmax, t->bank);
        t->twiddle_window = ft.twiddle;
        t->twiddle_window.insert(t->twiddle_window.end(), ft.window.begin(), ft.window.end());
        std::vector<int32_t> recs((size_t)4 * n_mels, 0);
        std::vector<float> runs;
        for (int j = 0; j < n_mels; j++) {
            const float *const row = &t->bank[(size_t)j * bins];
            int first = 0, last = -1; // the row's first and last non-zero entry
            for (int k = 0; k < bins; k++)
                if (row[k] != 0.f) {
                    if (last < 0) first = k;
                    last = k;
                }
            recs[4 * (size_t)j] = first, recs[4 * (size_t)j + 1] = last - first + 1 > 0 ? last - first + 1 : 0, recs[4 * (size_t)j + 2] = (int32_t)runs.size();
            if (last >= 0) runs.insert(runs.end(), row + first, row + last + 1);
        }
        t->bands_weights.resize(recs.size() + runs.size());
        std::memcpy(t->bands_weights.data(), recs.data(), recs.size() * sizeof(int32_t));
        std::copy(runs.begin(), runs.end(), t->bands_weights.begin() + (ptrdiff_t)recs.size());
        return t;
    });
}

// ---- host side ----------------------------------------------------------------------------------------
// The tile in frames: the larger of 32 and 8192 / n_fft, a multiple of the store area's 32 frames and of the frames in flight.
static int melfft_tile(const opusgpu_spec_params &p) { return 8192 / p.n_fft > 32 ? 8192 / p.n_fft : 32; }
static int melfft_in_flight(const opusgpu_spec_params &p) {
    const int M = p.n_fft / 2, P = M / 4 < 256 ? M / 4 : 256;
    return 256 / P;
}
static size_t melfft_lds_bytes(const opusgpu_spec_params &p) {
    const int M = p.n_fft / 2;
    return (size_t)melfft_in_flight(p) * (size_t)(M + (M >> 5)) * sizeof(float2) + (size_t)p.n_mels * MEL_STG * sizeof(float);
}

// k_tracks_melfft over n tracks (og_feat.hpp: tracks_feature_run; the frames' bound is tracks_melspec_run's).  The kernel's
// four tables travel as tracks_feature_run's two: twiddles and window in the one, band records and weights in the other.
static int tracks_melfft_run(int device, hipStream_t s, int n_tracks, const opusgpu_mel_span *spans, const void *d_in,
                             const opusgpu_spec_params *params, void *d_out, const TrackFail &hip_failed) {
    if (!spec_params_ok(params) || !spec_is_fft(*params)) return OPUSGPU_BAD_ARG;
    const int T = melfft_tile(*params);
    const MelFftTables *tab = nullptr;
    return tracks_feature_run(
        device, s, n_tracks, spans, d_in, d_out, T, 0x7fffffff - T, [&](int64_t n) { return spec_frames(*params, n); },
        [&] {
            tab = &melfft_tables(*params);
            return FeatTables{&tab->twiddle_window, &tab->bands_weights};
        },
        [&](unsigned n_tiles, const MelTile *d_tiles, const MelSpan *d_spans, const float2 *d_twiddle_window, const float *d_bands_weights) {
            MelFftArgs a{};
            a.n_fft = params->n_fft, a.hop = params->hop, a.n_mels = params->n_mels, a.tile = T;
            for (a.log2m = 0; (2 << a.log2m) < params->n_fft;) a.log2m++;
            const int items = melfft_in_flight(*params) * params->n_mels;
            for (a.log2g = 0; a.log2g < 6 && (items << (a.log2g + 1)) <= 256;) a.log2g++;
            a.power = params->power, a.log = params->log, a.whisper_frames = params->frames == OPUSGPU_SPEC_FRAMES_WHISPER;
            a.frames_major = params->layout == OPUSGPU_MEL_FRAMES_MAJOR, a.floor = params->floor;
            hipLaunchKernelGGL(k_tracks_melfft, dim3(n_tiles), dim3(256), melfft_lds_bytes(*params), s, d_tiles, d_spans, (const i16 *)d_in,
                               d_twiddle_window, d_bands_weights, a, (float *)d_out);
        },
        hip_failed);
}

extern "C" {

int opusgpu_spec_fft_tables(const opusgpu_spec_params *p, const float **window, const float **twiddle) {
    if (!spec_params_ok(p) || !spec_is_fft(*p)) return OPUSGPU_BAD_ARG;
    const FftTables &t = fft_tables(p->n_fft, spec_win(*p));
    if (window) *window = t.window.data();
    if (twiddle) *twiddle = t.twiddle.data();
    return t.n_fft;
}

} // extern "C"
