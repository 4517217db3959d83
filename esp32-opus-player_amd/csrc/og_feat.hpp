// og_feat.hpp -- what the feature kernels share (include/opusgpu.h: TRACK FEATURES, TRACK SPECTROGRAMS, TRACK STFT, TRACK KALDI
// FEATURES): the span and tile records, the table builders and packers, the window stage of the dense kernels, cut by phase, one set of
// host record rules, the run function of every feature kernel and the
// whole-file flow that ends in one.  Included at the end of og_api.hip behind og_tracks_resample_ratio.hpp (files_resampled_run,
// files_ratio_run; og_tracks.hpp: RsDevBuf, track_f32) and in front of the feature headers: og_tracks_mel.hpp, og_tracks_stft.hpp
// (which includes og_tracks_fft.hpp), og_tracks_melspec.hpp (which includes og_tracks_melfft.hpp) and og_tracks_fbank.hpp.
#pragma once
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

// ---- records ------------------------------------------------------------------------------------------
struct MelSpan {
    long long in_offset, in_samples, out_offset, plane;
    float scale;
    i32 reserved;
};
struct MelTile {
    i32 track, first; // the tile's first frame, a multiple of the kernel's tile
};
static_assert(sizeof(opusgpu_mel_span) == sizeof(MelSpan) && sizeof(MelSpan) == 40, "mel span layout");

constexpr int MEL_STG = 36;         // floats per row of a wave's 32 x 32 store area: rows 16-byte aligned, 4 banks apart
constexpr int MS_MAXW = 32768;      // samples of the largest window cut by phase: 65,536 bytes of LDS, which a launch asks for by its own window
constexpr int MS_MAXBLK = 33;       // blocks of 32 bins at n_fft 2048

typedef float og_f32x16 __attribute__((ext_vector_type(16)));

// ---- the window stage of the dense kernels ------------------------------------------------------------
// Shared by k_tracks_melspec, k_tracks_stft and k_tracks_fbank, inlined into each.  Deliberately NOT shared: the DFT inner loops
// (operand order, Im sign, block sharing and Kaldi's tap walk are each kernel's own), k_tracks_mel's fixed-phase stage and
// MB-templated store (og_tracks_mel.hpp), k_tracks_fft / k_tracks_melfft, which share their own steps (og_tracks_fft.hpp), and the
// POWER, MEL and STORE steps of k_tracks_melspec and k_tracks_fbank: as functions they changed k_tracks_melspec's generated code,
// which is held identical (DESIGN.md section 13r has every form that was tried and what each changed).
//
// The window of a tile, W places, cut by PHASE: place p is at row p % H, column p / H, the rows packed without room between them
// (the first W % H rows hold W / H + 1 places, the others W / H): row `ph` begins at ph * Qm + min(ph, Qr).
struct FeatPhase {
    int H, Qm, Qr;
    __device__ __forceinline__ FeatPhase(int W, int hop) : H(hop), Qm(W / hop), Qr(W % hop) {}
    __device__ __forceinline__ int at(int ph, int col) const { return ph * Qm + (ph < Qr ? ph : Qr) + col; }
    __device__ __forceinline__ int place(int p) const {
        const int ph = p % H;
        return ph * Qm + (ph < Qr ? ph : Qr) + p / H;
    }
};
// The edge rules: for sample q outside [0, n) of a track of n > 0 samples, whether a sample of the track stands there, and which.
struct FeatEdgeTorch { // torch.stft's reflect padding: reflected once, else 0
    __device__ __forceinline__ bool operator()(long long q, long long n, long long &r) const {
        r = q < 0 ? -q : 2 * (n - 1) - q;
        return r >= 0 && r < n;
    }
};
struct FeatEdgeKaldi { // Kaldi's reflection, repeated: period 2n, the upper half mirrored; with snip_edges zeros
    int snip;
    __device__ __forceinline__ bool operator()(long long q, long long n, long long &r) const {
        if (snip) return false;
        r = q % (2 * n);
        if (r < 0) r += 2 * n;
        if (r >= n) r = 2 * n - 1 - r;
        return true;
    }
};
// 1. STAGE.  The first Wuse places of the window whose first sample is sample `base` of the track (n samples at trk) -> lds, by
// every thread of the workgroup, both barriers inside.  Neither the hop nor `base` need be a multiple of 8: the track comes through
// aligned 16-byte loads of the BUFFER, one piece per lane, and every sample of a piece finds its own place.  Nothing is read behind
// the piece that holds the track's last sample.  The places in front of the track and behind it are then filled by the edge rule,
// from LDS where the source is among the staged places, else from the track itself.  The tile has a frame, so n > 0 and base < n
// (a frame's first sample lies in front of the track's end under every frame rule here): the first place behind the track is
// min(n - base, Wuse), and the track's samples among the places, [qa, qb), are not empty.
template <class Edge>
__device__ __forceinline__ void feat_stage_window(i16 *lds, const FeatPhase ph, const i16 *trk, long long n, long long base, int Wuse,
                                                  int tid, int nthr, Edge edge) {
    const long long qa = base < 0 ? 0 : base;                  // the track's samples inside what is used of it: [qa, qb)
    const long long qb = n < base + Wuse ? n : base + Wuse;
    for (long long k = (qa >> 3) + tid; 8 * k < qb; k += nthr) {
        const uint4 v = *reinterpret_cast<const uint4 *>(trk + 8 * k);
        const u32 w32[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int h = 0; h < 8; h++) {
            const long long q = 8 * k + h;
            if (q >= qa && q < qb) lds[ph.place((int)(q - base))] = (i16)(w32[h >> 1] >> (16 * (h & 1)));
        }
    }
    __syncthreads();
    {
        const int lo_n = base < 0 ? (int)-base : 0;                     // places in front of the track
        const int hi_0 = n - base < Wuse ? (int)(n - base) : Wuse;      // the first place behind it
        for (int x = tid; x < lo_n + (Wuse - hi_0); x += nthr) {
            const int p = x < lo_n ? x : hi_0 + (x - lo_n);
            long long r;
            i16 s = 0;
            if (edge(base + p, n, r)) s = r >= qa && r < qb ? lds[ph.place((int)(r - base))] : trk[r]; // places of the track: not written here
            lds[ph.place(p)] = s;
        }
    }
    __syncthreads();
}

// ---- table builders -----------------------------------------------------------------------------------
static double mel_point_hz(double m) { // Slaney's scale: linear below 1 kHz at 200 / 3 Hz per mel, logarithmic above
    return m < 15.0 ? 200.0 / 3.0 * m : 1000.0 * std::exp(std::log(6.4) / 27.0 * (m - 15.0));
}
static double mel_point_mel(double f) { return f < 1000.0 ? 3.0 * f / 200.0 : 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0); }
static double mel_htk_hz(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }
static double mel_htk_mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
// The two builders that TRACK FEATURES, TRACK SPECTROGRAMS and TRACK STFT share.
// Wc, Ws [n_fft][n_fft / 2 + 1]: a periodic Hann window of `win` taps, centred in the frame, times cos and sin of 2 pi i k / n_fft.
static void mel_basis_make(int n_fft, int win, std::vector<float> &wc, std::vector<float> &ws) {
    const double pi = 3.14159265358979323846;
    const int bins = n_fft / 2 + 1, left = (n_fft - win) / 2;
    wc.assign((size_t)n_fft * bins, 0.f), ws.assign((size_t)n_fft * bins, 0.f);
    for (int i = left; i < left + win; i++) {
        const double w = 0.5 - 0.5 * std::cos(2.0 * pi * (i - left) / (double)win);
        for (int k = 0; k < bins; k++) {
            const double a = 2.0 * pi * ((i * k) % n_fft) / (double)n_fft; // the angle reduced in integers
            wc[(size_t)i * bins + k] = (float)(w * std::cos(a));
            ws[(size_t)i * bins + k] = (float)(w * std::sin(a));
        }
    }
}
// B [n_mels][bins]: triangles over n_mels + 2 points evenly spaced in mel over [fmin, fmax], bin k at k * bin_hz.
static void mel_bank_make(double bin_hz, int bins, int n_mels, bool htk, bool slaney_norm, double fmin, double fmax, std::vector<float> &bank) {
    const double m0 = htk ? mel_htk_mel(fmin) : mel_point_mel(fmin), m1 = htk ? mel_htk_mel(fmax) : mel_point_mel(fmax);
    std::vector<double> pts(n_mels + 2);
    for (int j = 0; j < n_mels + 2; j++) {
        const double m = j == n_mels + 1 ? m1 : m0 + j * ((m1 - m0) / (n_mels + 1));
        pts[j] = htk ? mel_htk_hz(m) : mel_point_hz(m);
    }
    bank.assign((size_t)n_mels * bins, 0.f);
    for (int j = 0; j < n_mels; j++) {
        const double lo = pts[j], ce = pts[j + 1], hi = pts[j + 2];
        for (int k = 0; k < bins; k++) {
            const double fr = bin_hz * k, lower = (fr - lo) / (ce - lo), upper = (hi - fr) / (hi - ce);
            const double w = std::fmax(0.0, std::fmin(lower, upper));
            bank[(size_t)j * bins + k] = (float)(slaney_norm ? w * (2.0 / (hi - lo)) : w);
        }
    }
}
// The blocks of 32 bins in which a bank [n_mels][bins] has a non-zero entry: the blocks a kernel walks.
static std::vector<int> feat_kept_blocks(const std::vector<float> &bank, int bins, int n_mels) {
    std::vector<int> blocks;
    const int nblk = (bins + 31) / 32;
    for (int nb = 0; nb < nblk; nb++) {
        bool any = false;
        for (int j = 0; j < n_mels && !any; j++)
            for (int k = 32 * nb; k < 32 * nb + 32 && k < bins && !any; k++) any = bank[(size_t)j * bins + k] != 0.f;
        if (any) blocks.push_back(nb);
    }
    return blocks;
}
// The two packers that the dense kernels' tables go through: the numbers of Wc / Ws and of a bank in the order the lanes load them, for
// a list of blocks of 32 bins (entry b of the list is block b of the packed table).
// basis [block][n_fft / 4 k-steps][64 lanes][cos, sin]: tap 1 + 2 ks + (lane >> 5), bin 32 nb + (lane & 31); the middle tap folded
// (u = 2 x there: cos halved; v = 0: no sin), 0 behind the last bin.
static std::vector<float> feat_pack_basis(const std::vector<float> &wc, const std::vector<float> &ws, int n_fft,
                                          const std::vector<int> &blocks) {
    const int bins = n_fft / 2 + 1, KS = n_fft / 4;
    std::vector<float> basis(blocks.size() * KS * 64 * 2, 0.f);
    for (size_t b = 0; b < blocks.size(); b++)
        for (int ks = 0; ks < KS; ks++)
            for (int lane = 0; lane < 64; lane++) {
                const int i = 1 + 2 * ks + (lane >> 5), k = 32 * blocks[b] + (lane & 31);
                if (k >= bins) continue;
                float *const d = &basis[((b * KS + ks) * 64 + lane) * 2];
                d[0] = i == n_fft / 2 ? 0.5f * wc[(size_t)i * bins + k] : wc[(size_t)i * bins + k];
                d[1] = i == n_fft / 2 ? 0.f : ws[(size_t)i * bins + k];
            }
    return basis;
}
// fb [block][MB band blocks][16][64 lanes]: band 32 mm + (lane & 31), bin 32 nb + 8 (r >> 2) + 4 (lane >> 5) + (r & 3), 0 behind
// the last band and bin; weighted(b, mm) is told of every (block, band block) that holds a non-zero entry: the caller's mask bits.
template <class Weighted>
static std::vector<float> feat_pack_fb(const std::vector<float> &bank, int bins, int n_mels, const std::vector<int> &blocks, int MB,
                                       Weighted weighted) {
    std::vector<float> fb(blocks.size() * MB * 16 * 64, 0.f);
    for (size_t b = 0; b < blocks.size(); b++)
        for (int mm = 0; mm < MB; mm++)
            for (int r = 0; r < 16; r++)
                for (int lane = 0; lane < 64; lane++) {
                    const int j = 32 * mm + (lane & 31), k = 32 * blocks[b] + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                    if (j >= n_mels || k >= bins) continue;
                    const float w = bank[(size_t)j * bins + k];
                    fb[((b * MB + mm) * 16 + r) * 64 + lane] = w;
                    if (w != 0.f) weighted((int)b, mm);
                }
    return fb;
}
// Tables made at first use and kept per key for the life of the process: the T of `key`, made by make() where there is none yet;
// safe from any number of threads.  One cache per (Key, T).  make() runs under the cache's lock: it takes no lock that a caller of
// another cache holds while calling this one.
template <class Key, class T>
static const T &feat_cached(const Key &key, const std::function<std::unique_ptr<T>()> &make) {
    static std::mutex mu;
    static std::map<Key, std::unique_ptr<T>> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it == cache.end()) it = cache.emplace(key, make()).first;
    return *it->second;
}

// ---- host record rules --------------------------------------------------------------------------------
// F of the records whose frames are centred on multiples of the hop: torch's n / hop + 1 (none of an empty track), Whisper's n / hop.
static int64_t feat_frames_centered(bool whisper, int hop, int64_t n) { return whisper ? n / hop : n ? n / hop + 1 : 0; }
// The tile of a dense kernel in frames: the largest of 128, 64, 32 whose window, (T - 1) hop + len samples, fits the kernel's LDS
// (32 does: the records' rules).
static int feat_dense_tile(int64_t hop, int64_t len) {
    for (int T = 128; T > 32; T >>= 1)
        if ((T - 1) * hop + len <= MS_MAXW) return T;
    return 32;
}
// A dense launch's LDS: the tile's window as int16, and with a store area no less than the waves' store areas; at most 65,536 bytes
// (feat_dense_tile).
static size_t feat_window_lds_bytes(int hop, int len, int T, bool with_store_area) {
    const size_t window = ((size_t)(T - 1) * hop + len) * 2, store = with_store_area ? (size_t)(T / 32) * 32 * MEL_STG * 4 : 0;
    return ((window > store ? window : store) + 15) / 16 * 16;
}
// n_fft, hop and win_length (0: n_fft) of a TRACK SPECTROGRAMS or TRACK STFT record, by its algorithm.
static bool dft_shape_ok(int n_fft, int hop, int win_length, bool algo_is_fft) {
    if (algo_is_fft) {
        if (n_fft < 64 || n_fft > 8192 || (n_fft & (n_fft - 1))) return false;
        if (hop < 1 || hop > n_fft) return false;
    } else {
        if (n_fft < 64 || n_fft > 2048 || n_fft % 16) return false;
        if (hop < 1 || hop > n_fft || 31 * hop + n_fft > MS_MAXW) return false;
    }
    return !win_length || (win_length >= 16 && win_length <= n_fft && win_length % 2 == 0);
}
// The grid of a record's features of tracks at up / down of 48 kHz: a track's plane is its planned length's frames, rounded up to 64,
// and it takes `width` planes; -> total floats, offsets[i] (if not null) track i's first.  frames(len) is F of a track of len samples.
template <class Frames>
static int64_t feat_plane(Frames frames, int64_t planned_48k, int up, int down) {
    return rs_round64(frames((planned_48k * up + down - 1) / down));
}
template <class Frames>
static int64_t feat_grid_layout(int n, const int64_t *planned_48k, int up, int down, int width, Frames frames, int64_t *offsets) {
    if (!(up >= 1 && up <= down && down <= 48000) || n < 0 || (n && !planned_48k)) return OPUSGPU_BAD_ARG;
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        if (planned_48k[i] < 0 || planned_48k[i] > INT64_MAX / 65536) return OPUSGPU_BAD_ARG;
        if (offsets) offsets[i] = at;
        at += width * feat_plane(frames, planned_48k[i], up, down);
    }
    return at;
}

// ---- host side ----------------------------------------------------------------------------------------
// Any feature kernel over n tracks: checks the spans, builds the tile table of T frames a tile, uploads it with the spans and the
// two packed tables, launches on `s` and waits; every device buffer of the call is freed on every way out.  frames(in_samples) is
// the kernel's frame count, max_frames the most a track may have; tables() is called once there is work and returns the packed
// basis and filterbank, launch(n_tiles, d_tiles, d_spans, d_basis, d_fb) then queues the kernel.
struct FeatTables {
    const std::vector<float> *basis, *fb;
};
template <class Frames, class Tables, class Launch>
static int tracks_feature_run(int device, hipStream_t s, int n_tracks, const opusgpu_mel_span *spans, const void *d_in, void *d_out, int T,
                              int64_t max_frames, Frames frames, Tables tables, Launch launch, const TrackFail &hip_failed) {
    if (n_tracks < 0 || (n_tracks && !spans)) return OPUSGPU_BAD_ARG;
    std::vector<MelTile> tiles;
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_mel_span &sp = spans[t];
        if (sp.in_offset < 0 || sp.in_offset % 8 || sp.in_samples < 0 || sp.out_offset < 0 || sp.out_offset % 64 || sp.reserved)
            return OPUSGPU_BAD_ARG;
        const int64_t F = frames(sp.in_samples);
        if (sp.plane < F || sp.plane % 64 || !std::isfinite(sp.scale)) return OPUSGPU_BAD_ARG;
        if (F > max_frames || (F + T - 1) / T + (int64_t)tiles.size() > 0x7fffffff) return OPUSGPU_BAD_ARG;
        for (int64_t f = 0; f < F; f += T) tiles.push_back(MelTile{t, (i32)f});
    }
    if (tiles.empty()) return OPUSGPU_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 127)) return OPUSGPU_BAD_ARG;
    const FeatTables tab = tables();
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles, d_basis, d_fb;
    TRK_CHK(d_spans.upload(spans, (size_t)n_tracks * sizeof(MelSpan)));
    TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(MelTile)));
    TRK_CHK(d_basis.upload(tab.basis->data(), tab.basis->size() * sizeof(float)));
    TRK_CHK(d_fb.upload(tab.fb->data(), tab.fb->size() * sizeof(float)));
    launch((unsigned)tiles.size(), (const MelTile *)d_tiles.p, (const MelSpan *)d_spans.p, (const float2 *)d_basis.p, (const float *)d_fb.p);
    TRK_CHK(hipGetLastError());
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// What differs between the whole-file calls that end in a feature kernel.
struct FeatFlow {
    int sample_rate;                                        // the argument check: the rate the params name, 0: they are refused
    const char *scratch_failed;                             // the message of a scratch buffer that could not be had
    std::function<int64_t(int64_t planned_48k, int up, int down)> plane;
    std::function<int64_t(int64_t len)> frames;             // of a track of `len` samples at the features' rate
    std::function<int64_t(int n, const int64_t *planned_48k, int up, int down, int64_t *feat_offsets)> layout;
    std::function<int(int n, const opusgpu_mel_span *spans, const void *d_in, void *d_feat)> run; // the kernel, into the grid at d_feat
    int width = 0, frames_major = 0;                        // of a cell's row and the grid's layout (FEATURE BATCHES reads them)
    const struct FeatDense *dense = nullptr;                // STFT BATCHES: the flow's own dense tensor (below), or none
};
// The flow of a record whose grid is feat_grid_layout's (every record's but TRACK FEATURES'): `ok` is its rules' verdict, and only
// with it are rate, width and frames_major read; the three functions are called only behind it.
template <class Frames, class Layout, class Run>
static FeatFlow feat_record_flow(bool ok, int rate, int width, int frames_major, const char *scratch_failed, Frames frames, Layout layout,
                                 Run run) {
    FeatFlow flow;
    flow.sample_rate = ok ? rate : 0;
    flow.scratch_failed = scratch_failed;
    flow.plane = [=](int64_t planned, int u, int d) { return feat_plane(frames, planned, u, d); };
    flow.frames = frames;
    flow.layout = layout;
    flow.run = run;
    if (ok) flow.width = width, flow.frames_major = frames_major;
    return flow;
}
// STFT BATCHES (og_stft_batch.hpp), as files_stft_run hands them to files_feature_run: the tensor has every track `stride` frames
// (`width` floats each) apart.  `wrong` is the reason of a refusal that needs no track, or nullptr.  direct: the tensor is itself
// a grid for the kernel (plane = stride, a multiple of 64), which writes d_out, and run(n, cells, nullptr, d_out) the pad cells
// behind it; else the kernel writes a scratch grid of the flow's own layout and run(n, cells, d_grid, d_out) the tensor from there.
struct FeatDense {
    int64_t stride;
    bool direct;
    const char *wrong, *stride_short;
    std::function<int(int n, const opusgpu_feat_span *cells, const void *d_grid, void *d_out)> run;
};

// FEATURE BATCHES (og_feat_batch.hpp, behind the feature headers): the stage that turns a packed grid into the dense tensor.
static const char *feat_batch_shape_wrong(const opusgpu_feat_batch_req &r, int affine_width, int W);
static int feat_batch_run(int device, hipStream_t s, int n_tracks, const opusgpu_feat_span *spans, int W, int layout,
                          const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid, void *d_out,
                          const TrackFail &hip_failed, const std::function<void(const char *)> &why);

// Every whole-file call that ends in a feature kernel: what it refuses before any device work -- on top of the resampling call's own
// refusals the result is one channel, at the rate the params name --, then files_resampled_run (`rate`, with up = down = 0) or
// files_ratio_run (rate 0) with the owner's decoder into a scratch buffer of int16 mono tracks at the features' rate, on that call's
// grid -- the 48 kHz scratch is theirs and is gone when they return --, then the kernel from there into d_out.  The caller's arrays
// are written last.
static int files_feature_run(const FilesOwner &own, int rate, int up, int down, int mono, const opusgpu_mix_matrix *mix, const float *scale,
                             void *d_out, int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out,
                             const FeatFlow &flow) {
    const og_batch &b = own.b;
    const int sample_rate = flow.sample_rate;
    if (!sample_rate || ((uintptr_t)d_out & 127)) return OPUSGPU_BAD_ARG;
    if (mix ? mono || mix->out_channels != 1 : !mono) return OPUSGPU_BAD_ARG;
    if (rate) {
        if (up || down) return OPUSGPU_BAD_ARG;
        const int D = rs_args_factor(b.channels, rate, mono, OPUSGPU_TRACKS_S16, mix);
        if (!D) return OPUSGPU_BAD_ARG;
        up = 1, down = D;
    } else {
        if (!rr_args_taps(b.channels, up, down, mono, OPUSGPU_TRACKS_S16, mix)) return OPUSGPU_BAD_ARG;
        if (48000LL * up % down) return OPUSGPU_BAD_ARG; // the track's rate is no integer: no sample_rate names it
    }
    if ((int64_t)sample_rate * down != 48000LL * up) return OPUSGPU_BAD_ARG;
    if (!rs_scale_ok(OPUSGPU_TRACKS_F32, scale, b.n_files)) return OPUSGPU_BAD_ARG;
    const size_t n = (size_t)b.n_files;
    std::vector<int64_t> planned(n), offs(n, 0), len(n, 0), lengths(n, 0), feat(n, 0);
    std::vector<int32_t> status(2 * n, 0);
    for (size_t i = 0; i < n; i++) planned[i] = b.info[i].track_samples;
    const int64_t total = rate ? opusgpu_resample_layout((int)n, planned.data(), rate, nullptr)
                               : opusgpu_resample_ratio_layout((int)n, planned.data(), up, down, nullptr);
    const int64_t feat_total = total < 0 ? -1 : flow.layout((int)n, planned.data(), up, down, feat.data());
    if (feat_total < 0) return OPUSGPU_BAD_ARG;
    // FEATURE BATCHES: with a request on, the kernel writes a scratch grid and feat_batch_run the caller's buffer from there
    const FeatBatchState *fb = own.fbatch && own.fbatch->req.enabled ? own.fbatch : nullptr;
    if (fb) {
        const char *bad = feat_batch_shape_wrong(fb->req, (int)fb->sub.size(), flow.width);
        for (size_t i = 0; i < n && !bad; i++)
            if (flow.frames((planned[i] * up + down - 1) / down) > fb->req.stride_frames)
                bad = "feature batch: stride_frames is below the frames of a track's planned length";
        if (bad) {
            if (own.refused) own.refused(bad);
            return OPUSGPU_BAD_ARG;
        }
    }
    const FeatDense *dn = fb ? nullptr : flow.dense;
    if (dn) {
        const char *bad = dn->wrong;
        for (size_t i = 0; i < n && !bad; i++)
            if (flow.frames((planned[i] * up + down - 1) / down) > dn->stride) bad = dn->stride_short;
        if (bad) {
            if (own.refused) own.refused(bad);
            return OPUSGPU_BAD_ARG;
        }
    }
    const bool scratch_grid = fb || (dn && !dn->direct);
    RsDevBuf y; // the int16 mono tracks at the features' rate, for the length of this call
    RsDevBuf grid; // FEATURE BATCHES, STFT BATCHES: the packed features, for the length of this call
    if (!b.segs.empty()) {
        hipError_t e = hipSetDevice(own.device);
        if (e == hipSuccess) e = y.alloc((size_t)total * 2 + 128);
        if (e != hipSuccess) return own.hip_failed(OPUSGPU_ALLOC_FAIL, flow.scratch_failed, e);
    }
    if (scratch_grid && n) {
        hipError_t e = hipSetDevice(own.device);
        if (e == hipSuccess) e = grid.alloc((size_t)feat_total * 4 + 128);
        if (e != hipSuccess) return own.hip_failed(OPUSGPU_ALLOC_FAIL, flow.scratch_failed, e);
    }
    FilesOwner inner = own; // TRACK LOUDNESS: measured there on the 48 kHz scratch, the gain applied here with the scale
    inner.scale_later = true;
    const int rc = rate ? files_resampled_run(inner, rate, mono, mix, OPUSGPU_TRACKS_S16, nullptr, y.p, offs.data(), len.data(), lengths.data(),
                                              status.data())
                        : files_ratio_run(inner, up, down, mono, mix, OPUSGPU_TRACKS_S16, nullptr, y.p, offs.data(), len.data(), lengths.data(),
                                          status.data());
    if (rc) return rc;
    std::vector<opusgpu_mel_span> spans(n);
    for (size_t i = 0; i < n; i++)
        spans[i] = opusgpu_mel_span{offs[i], len[i], dn && dn->direct ? (int64_t)i * dn->stride * flow.width : feat[i],
                                    dn && dn->direct ? dn->stride : flow.plane(planned[i], up, down),
                                    loud_normalizes(own) ? loud_scale(own, scale, i) : scale ? scale[i] : 1.0f / 32768, 0};
    if (int rc2 = flow.run((int)n, spans.data(), y.p, scratch_grid ? grid.p : d_out)) return rc2;
    if (dn) {
        std::vector<opusgpu_feat_span> cells(n);
        for (size_t i = 0; i < n; i++) cells[i] = opusgpu_feat_span{feat[i], spans[i].plane, flow.frames(len[i])};
        if (int rc2 = dn->run((int)n, cells.data(), dn->direct ? nullptr : grid.p, d_out)) return rc2;
        for (size_t i = 0; i < n; i++) feat[i] = (int64_t)i * dn->stride * flow.width;
    }
    if (fb) {
        std::vector<opusgpu_feat_span> cells(n);
        for (size_t i = 0; i < n; i++) cells[i] = opusgpu_feat_span{feat[i], spans[i].plane, flow.frames(len[i])};
        if (int rc2 = feat_batch_run(own.device, own.stream, (int)n, cells.data(), flow.width, flow.frames_major, &fb->req, fb->sub.data(),
                                     fb->mul.data(), grid.p, d_out, own.hip_failed, own.refused))
            return rc2;
        opusgpu_feat_batch_layout((int)n, flow.width, fb->req.stride_frames, feat.data());
    }
    for (size_t i = 0; i < n; i++) {
        if (feat_offsets) feat_offsets[i] = feat[i];
        if (frames_out) frames_out[i] = flow.frames(len[i]);
        if (track_lengths_out) track_lengths_out[i] = lengths[i];
    }
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    return OPUSGPU_OK;
}
