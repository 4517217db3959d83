// og_tracks_fft.hpp -- TRACK STFT by FFT (include/opusgpu.h, TRACK STFT, OPUSGPU_STFT_ALGO_FFT): the window and twiddle tables per
// (n_fft, win_length), the kernel that turns packed int16 mono tracks into float32 spectrogram tracks for n_fft = 64 .. 8192, and its
// host side.  Included by og_tracks_stft.hpp behind the record's rules, which this header reads, and in front of tracks_stft_run, which
// sends every FFT record here: the whole-file calls, the layout and STFT BATCHES are that header's.
#pragma once

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_fft<FM>: one workgroup of 256 threads per tile of T consecutive frames of one track (fft_tile), over the MelTile / MelSpan
// tables of tracks_feature_run.  A real frame of n_fft samples goes through a complex FFT of M = n_fft / 2 points:
//   z[j] = x[2j] w[2j] + i x[2j + 1] w[2j + 1],  Z = FFT_M(z),  X[k] = E[k] + e^{-2 pi i k / n_fft} O[k],  k in [0, M],
//   E[k] = (Z[k] + conj Z[M - k]) / 2,  O[k] = (Z[k] - conj Z[M - k]) / 2i,  Z[M] = Z[0].
// P = min(256, M / 4) threads hold one frame, so C = 256 / P frames are in flight at once (32 at n_fft 64, one from 2048 up) and a
// tile takes ceil(frames / C) rounds of:
//   1. LOAD.  Thread t of a frame's P makes z[j], j = t, t + P, ...: the samples straight from global memory (overlapping frames
//      hit L2) by the reflection rule of k_tracks_stft -- once, then zeros -- each (float)y * scale in one multiply, then the window;
//      z[j] goes to place bitrev(j) of the frame's LDS buffer.
//   2. PASSES, in place, decimation in time: one radix-2 pass if log2 M is odd, then passes that are two radix-2 stages fused
//      (half sizes h and 2h: places b, b + h, b + 2h, b + 3h; the second stage's twiddles are w and -i w), a barrier behind each.
//      The M-point twiddles are every second entry of the n_fft-point table, which the split pass reads whole.
//   3. SPLIT, FINISH, STORE.  X[k] from Z[k] and Z[M - k]; Re^2 + Im^2, its sqrtf, the floor, a log, or the pair; stored from the
//      registers.  FM true (frames-major): the P threads of a frame take its bins in turn, so a wave stores consecutive bins of one
//      row.  FM false (bins-major): the 256 threads take (bin, frame in flight) with the frame fastest, so a bin row gets runs of
//      C consecutive frames: 128 bytes at n_fft 64, single cells from 2048 up, where a tile's 16 frames of a row are 16 stores
//      of one workgroup that meet in L2 (DESIGN.md section 13p has what that costs).
// The pair's halves end in + 0.0f: a butterfly's sum of two -0 is -0, and an all-zero track under a negative scale must give +0.
// LDS: C buffers of M + M / 32 float2 (one place of padding per 32): 8,448 bytes up to n_fft 2048, 16,896 at 4096, 33,792 at 8192.
// No float atomics, no sum whose order depends on the launch: the same input gives the same bits.
struct FftArgs {
    i32 n_fft, hop, bins, tile;
    i32 log2m;                      // log2 of M = n_fft / 2: 5 .. 12
    i32 power, log, whisper_frames; // power 0: pairs
    float floor;
};

__device__ __forceinline__ int fft_place(int p) { return p + (p >> 5); }

// The steps that k_tracks_fft and k_tracks_melfft (og_tracks_melfft.hpp) share, for the P threads of one frame, t in [0, P).
// Sample q of a track of n samples, counted from the track's first: reflected once, then 0; (float)y * scale in one multiply.
__device__ __forceinline__ float fft_sample(const i16 *trk, long long n, float scale, long long q) {
    if (q < 0)
        q = -q;
    else if (q >= n)
        q = 2 * (n - 1) - q; // reflected once
    const i16 y = q >= 0 && q < n ? trk[q] : (i16)0;
    return __fmul_rn((float)y, scale);
}
// 1. LOAD: z[j] of the frame whose first sample is `base`, to place bitrev(j) of `buf`.
__device__ __forceinline__ void fft_load(float2 *buf, const i16 *trk, long long n, float scale, const float *window, long long base, int t,
                                         int P, int L) {
    const int M = 1 << L;
    for (int j = t; j < M; j += P) {
        const float x0 = __fmul_rn(fft_sample(trk, n, scale, base + 2 * j), window[2 * j]);
        const float x1 = __fmul_rn(fft_sample(trk, n, scale, base + 2 * j + 1), window[2 * j + 1]);
        buf[fft_place((int)(__brev((unsigned)j) >> (32 - L)))] = make_float2(x0, x1);
    }
}
// 2. PASSES over `buf`, in place, a barrier behind each: every thread of the workgroup calls this.
__device__ __forceinline__ void fft_passes(float2 *buf, const float2 *twiddle, int t, int P, int L) {
    const int M = 1 << L;
    int s = 0;
    if (L & 1) {
        for (int u = t; u < M / 2; u += P) {
            const float2 x0 = buf[fft_place(2 * u)], x1 = buf[fft_place(2 * u + 1)];
            buf[fft_place(2 * u)] = make_float2(x0.x + x1.x, x0.y + x1.y);
            buf[fft_place(2 * u + 1)] = make_float2(x0.x - x1.x, x0.y - x1.y);
        }
        s = 1;
        __syncthreads();
    }
    for (; s < L; s += 2) {
        const int h = 1 << s;
        for (int u = t; u < M / 4; u += P) {
            const int j = u & (h - 1), b = ((u >> s) << (s + 2)) + j;
            const float2 w2 = twiddle[j << (L - s)], w4 = twiddle[j << (L - s - 1)]; // e^{-i a} = (cos a, -sin a)
            const float2 x0 = buf[fft_place(b)], x1 = buf[fft_place(b + h)], x2 = buf[fft_place(b + 2 * h)], x3 = buf[fft_place(b + 3 * h)];
            const float2 t1 = make_float2(x1.x * w2.x + x1.y * w2.y, x1.y * w2.x - x1.x * w2.y);
            const float2 t3 = make_float2(x3.x * w2.x + x3.y * w2.y, x3.y * w2.x - x3.x * w2.y);
            const float2 a0 = make_float2(x0.x + t1.x, x0.y + t1.y), a1 = make_float2(x0.x - t1.x, x0.y - t1.y);
            const float2 a2 = make_float2(x2.x + t3.x, x2.y + t3.y), a3 = make_float2(x2.x - t3.x, x2.y - t3.y);
            const float2 u2 = make_float2(a2.x * w4.x + a2.y * w4.y, a2.y * w4.x - a2.x * w4.y);
            const float2 v3 = make_float2(a3.x * w4.x + a3.y * w4.y, a3.y * w4.x - a3.x * w4.y);
            const float2 u3 = make_float2(v3.y, -v3.x); // times -i
            buf[fft_place(b)] = make_float2(a0.x + u2.x, a0.y + u2.y);
            buf[fft_place(b + 2 * h)] = make_float2(a0.x - u2.x, a0.y - u2.y);
            buf[fft_place(b + h)] = make_float2(a1.x + u3.x, a1.y + u3.y);
            buf[fft_place(b + 3 * h)] = make_float2(a1.x - u3.x, a1.y - u3.y);
        }
        __syncthreads();
    }
}
// 3. SPLIT: X[k], k in [0, M], from Z[k] and Z[M - k] of the frame's buffer z.
__device__ __forceinline__ void fft_bin(const float2 *z, const float2 *twiddle, int M, int k, float &re, float &im) {
    const float2 zk = z[fft_place(k & (M - 1))], zm = z[fft_place((M - k) & (M - 1))];
    const float er = 0.5f * (zk.x + zm.x), ei = 0.5f * (zk.y - zm.y);  // E = (Z[k] + conj Z[M - k]) / 2
    const float dr = 0.5f * (zk.x - zm.x), di = 0.5f * (zk.y + zm.y);  // D = (Z[k] - conj Z[M - k]) / 2, O = -i D
    const float2 w = k < M ? twiddle[k] : make_float2(-1.f, 0.f);
    const float orr = di, oi = -dr;
    re = er + (orr * w.x + oi * w.y);
    im = ei + (oi * w.x - orr * w.y);
}

template <bool FM>
__global__ void __launch_bounds__(256) k_tracks_fft(const MelTile *__restrict__ tiles, const MelSpan *__restrict__ spans,
                                                    const i16 *__restrict__ in, const float2 *__restrict__ twiddle,
                                                    const float *__restrict__ window, FftArgs a, float *__restrict__ out) {
    extern __shared__ __align__(16) float2 fft_lds[]; // C buffers of fft_place(M) places (fft_lds_bytes)
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
    const int bins = a.bins, power = a.power, log = a.log;
    const float floor = a.floor;
    float2 *const buf = fft_lds + slot * S;

    auto finish_store = [&](long long f, int k, float re, float im) {
        const long long cell = FM ? f * bins + k : k * plane + f;
        if (power == 0) {
            *reinterpret_cast<float2 *>(dst + 2 * cell) = make_float2(re + 0.0f, im + 0.0f);
        } else {
            float v = re * re + im * im;
            if (power == 1) v = sqrtf(v);
            v = fmaxf(v, floor);
            if (log == 1) v = log10f(v);
            if (log == 2) v = logf(v);
            dst[cell] = v;
        }
    };

    for (int r0 = 0; r0 < nf; r0 += C) { // a round: frames r0 .. r0 + C - 1 of the tile, those that exist
        // 1. load
        if (r0 + slot < nf) fft_load(buf, trk, n, scale, window, (long long)H * (tl.first + r0 + slot) - N / 2, t, P, L);
        __syncthreads();
        // 2. passes (a slot without a frame runs them over what its buffer holds and stores nothing)
        fft_passes(buf, twiddle, t, P, L);
        // 3. split, finish, store
        if (FM) {
            if (r0 + slot < nf) {
                const long long f = (long long)tl.first + r0 + slot;
                for (int k = t; k <= M; k += P) {
                    float re, im;
                    fft_bin(buf, twiddle, M, k, re, im);
                    finish_store(f, k, re, im);
                }
            }
        } else {
            for (int x = tid; x < (M + 1) * C; x += 256) {
                const int c = x & (C - 1), k = x >> cs;
                if (r0 + c < nf) {
                    float re, im;
                    fft_bin(fft_lds + c * S, twiddle, M, k, re, im);
                    finish_store((long long)tl.first + r0 + c, k, re, im);
                }
            }
        }
        __syncthreads(); // the next round loads over what this one read
    }
}

// ---- tables -------------------------------------------------------------------------------------------
// TRACK STFT, FFT TABLES: made in double at first use, rounded once, kept per (n_fft, win_length) for the life of the process.
struct FftTables {
    int n_fft = 0;
    std::vector<float> window;  // [n_fft]: (float)w[i]
    std::vector<float> twiddle; // [n_fft / 2][cos, sin] of 2 pi j / n_fft
};

// The tables of an FFT record that stft_params_ok or spec_params_ok has passed, by its n_fft and window length (never 0 here); safe
// from any number of threads.  TRACK SPECTROGRAMS' FFT records take theirs from this cache too (og_tracks_melfft.hpp).
static const FftTables &fft_tables(int n_fft, int win) {
    return feat_cached<std::pair<int, int>, FftTables>({n_fft, win}, [&] {
        const double pi = 3.14159265358979323846;
        std::unique_ptr<FftTables> t(new FftTables);
        const int left = (n_fft - win) / 2;
        t->n_fft = n_fft;
        t->window.assign((size_t)n_fft, 0.f);
        for (int i = left; i < left + win; i++) t->window[(size_t)i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (i - left) / (double)win));
        t->twiddle.resize((size_t)n_fft);
        for (int j = 0; j < n_fft / 2; j++) {
            const double ang = 2.0 * pi * j / (double)n_fft;
            t->twiddle[2 * (size_t)j] = (float)std::cos(ang), t->twiddle[2 * (size_t)j + 1] = (float)std::sin(ang);
        }
        return t;
    });
}

// ---- host side ----------------------------------------------------------------------------------------
// The tile in frames: the larger of 16 and 8192 / n_fft -- four rounds of the frames in flight up to n_fft 256, 16 frames from 512 up.
static int fft_tile(const opusgpu_stft_params &p) { return 8192 / p.n_fft > 16 ? 8192 / p.n_fft : 16; }
static size_t fft_lds_bytes(const opusgpu_stft_params &p) {
    const int M = p.n_fft / 2, P = M / 4 < 256 ? M / 4 : 256;
    return (size_t)(256 / P) * (size_t)(M + (M >> 5)) * sizeof(float2);
}

// k_tracks_fft over n tracks (og_feat.hpp: tracks_feature_run; the frames' bound is tracks_stft_run's).  hop needs no bound
// beyond [1, n_fft]: the kernel keeps no window in LDS and forms hop * frame in 64 bits.
static int tracks_fft_run(int device, hipStream_t s, int n_tracks, const opusgpu_mel_span *spans, const void *d_in,
                          const opusgpu_stft_params *params, void *d_out, const TrackFail &hip_failed) {
    if (!stft_params_ok(params) || !stft_is_fft(*params)) return OPUSGPU_BAD_ARG;
    const int T = fft_tile(*params);
    const FftTables *tab = nullptr;
    return tracks_feature_run(
        device, s, n_tracks, spans, d_in, d_out, T, 0x7fffffff - T, [&](int64_t n) { return stft_frames(*params, n); },
        [&] {
            tab = &fft_tables(params->n_fft, stft_win(*params));
            return FeatTables{&tab->twiddle, &tab->window};
        },
        [&](unsigned n_tiles, const MelTile *d_tiles, const MelSpan *d_spans, const float2 *d_twiddle, const float *d_window) {
            FftArgs a{};
            a.n_fft = params->n_fft, a.hop = params->hop, a.bins = params->n_fft / 2 + 1, a.tile = T;
            for (a.log2m = 0; (2 << a.log2m) < params->n_fft;) a.log2m++;
            a.power = params->power, a.log = params->log, a.whisper_frames = params->frames == OPUSGPU_SPEC_FRAMES_WHISPER;
            a.floor = params->floor;
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(n_tiles), dim3(256), fft_lds_bytes(*params), s, d_tiles, d_spans, (const i16 *)d_in, d_twiddle,
                                   d_window, a, (float *)d_out);
            };
            if (params->layout == OPUSGPU_MEL_FRAMES_MAJOR)
                go(k_tracks_fft<true>);
            else
                go(k_tracks_fft<false>);
        },
        hip_failed);
}

extern "C" {

int opusgpu_stft_fft_tables(const opusgpu_stft_params *p, const float **window, const float **twiddle) {
    if (!stft_params_ok(p) || !stft_is_fft(*p)) return OPUSGPU_BAD_ARG;
    const FftTables &t = fft_tables(p->n_fft, stft_win(*p));
    if (window) *window = t.window.data();
    if (twiddle) *twiddle = t.twiddle.data();
    return t.n_fft;
}

} // extern "C"
