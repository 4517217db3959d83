// og_tracks_resample.hpp -- tracks at 8 / 12 / 16 / 24 kHz, the mono downmix and the channel mix (include/opusgpu.h, TRACK RATES and
// CHANNEL MIX): the kernels that turn packed int16 tracks into decimated ones, their host side, and the whole-file calls that end in them.  Included at the end of
// og_api.hip behind og_tracks.hpp (files_decode_run, track_f32, track_store4) and in front of og_ms_tracks.hpp.
#pragma once
#include <cmath>
#include <cstdlib>
#define OG_RS_PAIRS_ROM static __device__ const
#include "og_resample_taps.hpp"
#include "og_downmix_tables.hpp"

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_resample<D>: one workgroup per entry of a tile table built on the host, a tile being `tile` consecutive output samples
// of every output channel of one track (a 1-D grid: a long track among short ones costs its own tiles and nothing else).
//   1. STAGE.  The tile's input window -- (tile + 24) D samples of every channel, 12 D of them in front of the first output's own
//      sample -- comes into LDS through aligned 16-byte loads of the interleaved track, one piece per lane.  Samples outside
//      [0, in_samples) are zeros (pieces without a sample inside are not fetched: nothing is read behind the 16-byte piece that
//      holds a track's last sample), a stereo pair becomes (l + r + 1) >> 1 here when `mono`.  In LDS the window is de-interleaved
//      twice: one plane per channel and PHASE, sample n0 + D q + p of channel c at place q of plane (c, p).  Tap k = D a + p of
//      output j then meets place j + a of plane p: lanes that step through a plane side by side read consecutive words, whatever D.
//      A last tile that is not full stages n_out + 24 places of a plane, and its last group of four outputs reads up to three
//      places more: words nobody wrote.  They meet only tap pairs that are zero (place j + 24 of an output j that is stored has
//      the one tap of phase 0, and the pair's other half and the places behind it belong to taps that do not exist) or feed
//      outputs at j >= n_out, which are never stored, as are the unwritten results behind them that a partial last piece reads
//      in step 3.  The arithmetic is integer: there is no NaN to spread, and no value to trap on.
//   2. MAC.  A lane owns four consecutive outputs of one channel.  Per phase it reads the 14 words (28 places) they need once and
//      feeds them to v_dot2_i32_i16, two neighbouring places against two taps D apart per instruction: 13 per output and phase,
//      for 24 + 1 / D taps.  The tap pairs are literals of the instruction (og_resample_taps.hpp, generated; the loops are
//      unrolled), so they are wave-uniform by construction.  Outputs at odd places take the same words against pairs shifted by
//      one tap.  The sum starts at 16384 and is exact in int32 (sum |h| <= 65535); >> 15 and the clamp make the int16 result,
//      which goes to a second LDS area in the order of the destination.
//   3. STORE.  A lane owns an aligned 16-byte piece of the destination -- 8 int16 or 4 floats ((float)y * scale, track_f32) of the
//      interleaved track, or 4 floats of one plane -- and stores it whole (track_store4 for floats); tracks begin at multiples
//      of 64 samples and tiles at multiples of `tile`, so only a track's last piece can be partial: it goes out as element stores.
// D = 1 (rate 48000, mono only) has no filter: the staged downmix is the result.
// Steps 2 and 3 are functions (rs_mac, rs_store) that k_tracks_resample_mix<D>, the kernel with a channel mix in step 1, shares.
struct ResampleSpan {
    long long in_offset, in_samples, out_offset, out_plane;
    float scale;
    i32 reserved;
};
struct ResampleTile {
    i32 track, reserved;
    long long first; // the tile's first output sample, a multiple of the tile length
};
static_assert(sizeof(opusgpu_resample_span) == sizeof(ResampleSpan) && sizeof(ResampleSpan) == 40, "resample span layout");

// Places behind a plane's `tile`: a group of four outputs at place 4 i reads places [4 i, 4 i + 28), of which a partial last tile
// has written those below n_out + 24 (the rest is harmless, see STAGE above); 40 keeps planes 16-byte aligned and 20 banks apart.
constexpr int RS_PLANE_PAD = 40;

template <int D>
__device__ __forceinline__ const u32 *rs_pairs() {
    if constexpr (D == 2) return og_rs_pairs_2;
    if constexpr (D == 3) return og_rs_pairs_3;
    if constexpr (D == 4) return og_rs_pairs_4;
    if constexpr (D == 6) return og_rs_pairs_6;
    return nullptr;
}
// (rs_dot2, the multiply-accumulate of step 2: og_common.hpp, where tests/gpu_kat can reach it without this file's host side)

// Step 2 of k_tracks_resample<D> and k_tracks_resample_mix<D>: the planes of CO channels -> the tile's results in `yo`.
template <int D>
__device__ __forceinline__ void rs_mac(const i16 *lds, i16 *yo, int CO, int tile_shift, int n_out, bool planar, int tid) {
    if constexpr (D > 1) { // four outputs per lane
        const int tile = 1 << tile_shift, Q = tile + RS_PLANE_PAD;
        const u32 *const pairs = rs_pairs<D>();
        const int items = CO << (tile_shift - 2);
        for (int x = tid; x < items; x += 256) {
            const int c = x >> (tile_shift - 2), i = x & ((tile >> 2) - 1);
            if (4 * i >= n_out) continue;
            i32 acc[4] = {16384, 16384, 16384, 16384};
#pragma unroll
            for (int p = 0; p < D; p++) {
                const uint2 *src = reinterpret_cast<const uint2 *>(lds + (c * D + p) * Q + 4 * i); // 8-byte aligned
                u32 X[14];
#pragma unroll
                for (int w = 0; w < 7; w++) {
                    const uint2 t = src[w];
                    X[2 * w] = t.x, X[2 * w + 1] = t.y;
                }
#pragma unroll
                for (int w = 0; w < OG_RS_PAIRS; w++) {
                    const u32 te = pairs[(2 * p) * OG_RS_PAIRS + w], to = pairs[(2 * p + 1) * OG_RS_PAIRS + w];
                    acc[0] = rs_dot2(X[w], te, acc[0]);
                    acc[1] = rs_dot2(X[w], to, acc[1]);
                    acc[2] = rs_dot2(X[w + 1], te, acc[2]);
                    acc[3] = rs_dot2(X[w + 1], to, acc[3]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const i32 y = acc[r] >> 15;
                const int j = 4 * i + r;
                yo[planar ? c * tile + j : j * CO + c] = (i16)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
            }
        }
        __syncthreads();
    }
}

// Step 3 of both kernels: the tile's n_out results of CO channels -> the track, 16 bytes per lane and store.
__device__ __forceinline__ void rs_store(const i16 *yo, const ResampleSpan &sp, const ResampleTile &tl, int CO, int n_out, int tile, int format,
                                         bool planar, void *__restrict__ out, int tid) {
    const float k = sp.scale;
    if (format == OPUSGPU_TRACKS_S16) {
        i16 *const dst = static_cast<i16 *>(out) + (sp.out_offset + tl.first) * CO;
        const int EN = n_out * CO;
        for (int q = tid; q < (EN + 7) >> 3; q += 256) {
            const uint4 v = *reinterpret_cast<const uint4 *>(yo + 8 * q);
            if (8 * q + 8 <= EN) {
                *reinterpret_cast<uint4 *>(dst + 8 * q) = v;
            } else {
                const u32 w32[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int h = 0; h < 8; h++)
                    if (8 * q + h < EN) dst[8 * q + h] = (i16)(w32[h >> 1] >> (16 * (h & 1)));
            }
        }
    } else {
        // interleaved: one run of n_out * CO elements; planar: CO runs of n_out, one per plane (a mono track is its plane)
        const int runs = planar ? CO : 1, EN = planar ? n_out : n_out * CO;
        const int pp = (EN + 3) >> 2; // pieces per run
        float *const base = static_cast<float *>(out) + (planar ? sp.out_offset * CO + tl.first : (sp.out_offset + tl.first) * CO);
        for (int x = tid; x < runs * pp; x += 256) {
            const int c = planar ? x / pp : 0, q = x - c * pp;
            const uint2 v = *reinterpret_cast<const uint2 *>(yo + c * tile + 4 * q);
            const float f[4] = {track_f32(v.x, k), track_f32(v.x >> 16, k), track_f32(v.y, k), track_f32(v.y >> 16, k)};
            float *const d = base + c * sp.out_plane + 4 * q;
            if (4 * q + 4 <= EN) {
                track_store4(d, f);
            } else {
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (4 * q + h < EN) d[h] = f[h];
            }
        }
    }
}

// Step 1 of k_tracks_resample<D>, and of k_tracks_resample_ratio without a mix: the window of Wn samples from sample n0 of the track
// (negative at a track's head), all C channels or their mono downmix -> put(channel, sample in the window, value), which says where
// in LDS it goes.
template <class Put>
__device__ __forceinline__ void rs_stage(const i16 *__restrict__ in, const ResampleSpan &sp, int C, bool mono, long long n0, int Wn, int tid,
                                         Put put) {
    const int W = Wn * C;                                 // the window's elements, all input channels
    const long long G0 = (sp.in_offset + n0) * C;         // its first element in the buffer
    const int mis = (int)(G0 & 7);                        // elements between the aligned piece's first and it
    const long long V0 = sp.in_offset * C, V1 = (sp.in_offset + sp.in_samples) * C; // the track's elements; V0 is a multiple of 8
    const int pieces = (W + mis + 7) >> 3;
    const bool mix = mono && C == 2;
    for (int k = tid; k < pieces; k += 256) {
        const long long g = G0 - mis + 8LL * k;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g >= V0 && g < V1) v = *reinterpret_cast<const uint4 *>(in + g);
        const u32 w32[4] = {v.x, v.y, v.z, v.w};
        const int w = 8 * k - mis;        // the piece's first window element (-7 .. -1 possible in piece 0)
        int rel = (w + 8 * C) / C - 8;    // its sample in the window (floor) and channel
        int ch = w - rel * C;
        if (mix) { // pairs never straddle pieces: G0 is even
#pragma unroll
            for (int h = 0; h < 8; h += 2) {
                if (w + h >= 0 && w + h < W) {
                    const int r = rel + (h >> 1);
                    const long long n = n0 + r;
                    const u32 lr = w32[h >> 1];
                    const int m = n >= 0 && n < sp.in_samples ? ((int)(i16)lr + (int)(i16)(lr >> 16) + 1) >> 1 : 0;
                    put(0, r, (i16)m);
                }
            }
        } else {
#pragma unroll
            for (int h = 0; h < 8; h++) {
                if (w + h >= 0 && w + h < W) {
                    const long long n = n0 + rel;
                    const i16 s = n >= 0 && n < sp.in_samples ? (i16)(w32[h >> 1] >> (16 * (h & 1))) : (i16)0;
                    put(ch, rel, s);
                }
                if (++ch == C) ch = 0, rel++;
            }
        }
    }
}

template <int D>
__global__ void __launch_bounds__(256) k_tracks_resample(const ResampleTile *__restrict__ tiles, const ResampleSpan *__restrict__ spans,
                                                          const i16 *__restrict__ in, int C, int mono, int format, int tile_shift,
                                                          void *__restrict__ out) {
    extern __shared__ __align__(16) i16 lds[]; // [CO * D] planes of Q places, then the tile's results [CO * tile]
    const int tid = (int)threadIdx.x;
    const ResampleTile tl = tiles[blockIdx.x];
    const ResampleSpan sp = spans[tl.track];
    const int tile = 1 << tile_shift, Q = tile + RS_PLANE_PAD;
    const int CO = mono ? 1 : C;
    constexpr int LEAD = D == 1 ? 0 : 12; // places of a plane in front of an output's own: (L - 1) / 2 = 12 D samples
    const long long out_len = (sp.in_samples + D - 1) / D;
    const long long left = out_len - tl.first;
    const int n_out = left < tile ? (int)left : tile;
    if (n_out <= 0) return;
    i16 *const yo = D == 1 ? lds : lds + CO * D * Q;
    const bool planar = format == OPUSGPU_TRACKS_F32_PLANAR;

    // 1. the window -> LDS: sample r of channel ch at place r / D of plane (ch, r % D)
    rs_stage(in, sp, C, mono != 0, (tl.first - LEAD) * D, (n_out + 2 * LEAD) * D, tid,
             [=](int ch, int r, i16 s) { lds[(ch * D + r % D) * Q + r / D] = s; });
    __syncthreads();

    rs_mac<D>(lds, yo, CO, tile_shift, n_out, planar, tid);          // 2. four outputs per lane
    rs_store(yo, sp, tl, CO, n_out, tile, format, planar, out, tid); // 3. LDS -> the track
}

// k_tracks_resample_mix<D>: the same kernel with a channel mix in step 1 (include/opusgpu.h, CHANNEL MIX); steps 2 and 3 then run
// for CO = the matrix's rows.  A mix needs all C channels of a sample in one lane, so the window is cut by SAMPLE here: a lane owns
// 8 consecutive samples of the track, aligned to 8 from the track's start (in_offset is a multiple of 8: they are exactly C aligned
// 16-byte pieces), and loads them as C uint4 -- a piece whose first element lies outside the track is not fetched, as above.  C is
// a template parameter of the staging body (a wave-uniform switch in the kernel picks it), so that every element position is a
// literal and the 4 C words stay in registers.  For each output channel o (a wave-uniform loop) and each of the 8 samples the sum
// runs word by word through v_dot2_i32_i16: the word that holds channels (c, c + 1) of the sample against the pair
// (M[o][c], M[o][c + 1]).  Where a sample begins or ends in the middle of a word (odd C) the pair's other half is a coefficient
// that does not exist -- M[o][-1] or M[o][C], both 0 in the table -- and meets the neighbouring sample's element.  The table comes
// by value with the kernel's arguments, pair[o][c + 1] = (M[o][c], M[o][c + 1]) for c = -1 .. 7, and is indexed by o and literals:
// scalar loads, scalar operands.  The sum starts at 8192 and is exact in int32 (a row's sum |M| <= 65535); >> 14 and the clamp make
// x_o, 0 for a sample outside [0, in_samples), which goes to place r / D of plane (o, r % D) -- for D = 1 straight to the result
// area in the order of the destination.
struct RsMixArgs {
    i32 co;
    u32 pair[8][9];
};

// at_of(sample in the window) says where a sample goes within an output channel's area, put(o, that place, value) stores it:
// k_tracks_resample_ratio stages its own layout through the same body.
template <int C, class At, class Put>
__device__ __forceinline__ void rs_stage_mix_at(const i16 *__restrict__ in, const ResampleSpan &sp, const RsMixArgs &mx, long long n0, int Wn,
                                                int tid, At at_of, Put put) {
    const int CO = mx.co;
    const long long a0 = n0 & ~7LL;  // the group of 8 that holds the window's first sample (floor, also in front of the track)
    const int lead = (int)(n0 - a0); // samples of it in front of the window
    const int groups = (lead + Wn + 7) >> 3;
    const long long V0 = sp.in_offset * C, V1 = (sp.in_offset + sp.in_samples) * C; // the track's elements; V0 is a multiple of 8
    for (int k = tid; k < groups; k += 256) {
        const long long nb = a0 + 8LL * k;           // the lane's first sample, counted from the track's
        const long long g = (sp.in_offset + nb) * C; // its first element in the buffer, a multiple of 8
        u32 w[4 * C];
#pragma unroll
        for (int j = 0; j < C; j++) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g + 8 * j >= V0 && g + 8 * j < V1) v = *reinterpret_cast<const uint4 *>(in + g + 8 * j);
            w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
        }
        const int r0 = 8 * k - lead; // the lane's first sample in the window (-7 .. -1 possible in group 0)
        int at[8];                   // where sample s goes in the area of channel 0, -1: outside the window
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const int r = r0 + s;
            at[s] = r < 0 || r >= Wn ? -1 : at_of(r);
        }
        for (int o = 0; o < CO; o++) {
#pragma unroll
            for (int s = 0; s < 8; s++) {
                i32 acc = 8192;
#pragma unroll
                for (int wi = (s * C) >> 1; wi <= (s * C + C - 1) >> 1; wi++) acc = rs_dot2(w[wi], mx.pair[o][2 * wi - s * C + 1], acc);
                acc >>= 14;
                const long long n = nb + s;
                const i16 x = n >= 0 && n < sp.in_samples ? (i16)(acc < -32768 ? -32768 : acc > 32767 ? 32767 : acc) : (i16)0;
                if (at[s] >= 0) put(o, at[s], x);
            }
        }
    }
}

template <int D, int C>
__device__ __forceinline__ void rs_stage_mix(i16 *lds, const i16 *__restrict__ in, const ResampleSpan &sp, const RsMixArgs &mx, long long n0,
                                             int Wn, int Q, int tile, bool planar, int tid) {
    const int CO = mx.co;
    rs_stage_mix_at<C>(
        in, sp, mx, n0, Wn, tid, [=](int r) { return D == 1 ? r : (r % D) * Q + r / D; },
        [=](int o, int at, i16 x) { lds[D == 1 ? (planar ? o * tile + at : at * CO + o) : o * D * Q + at] = x; });
}

template <int D>
__global__ void __launch_bounds__(256) k_tracks_resample_mix(const ResampleTile *__restrict__ tiles, const ResampleSpan *__restrict__ spans,
                                                              const i16 *__restrict__ in, int C, RsMixArgs mx, int format, int tile_shift,
                                                              void *__restrict__ out) {
    extern __shared__ __align__(16) i16 lds[]; // as above, CO the matrix's rows
    const int tid = (int)threadIdx.x;
    const ResampleTile tl = tiles[blockIdx.x];
    const ResampleSpan sp = spans[tl.track];
    const int tile = 1 << tile_shift, Q = tile + RS_PLANE_PAD;
    const int CO = mx.co;
    constexpr int LEAD = D == 1 ? 0 : 12;
    const long long out_len = (sp.in_samples + D - 1) / D;
    const long long left = out_len - tl.first;
    const int n_out = left < tile ? (int)left : tile;
    if (n_out <= 0) return;
    i16 *const yo = D == 1 ? lds : lds + CO * D * Q;
    const bool planar = format == OPUSGPU_TRACKS_F32_PLANAR;
    const long long n0 = (tl.first - LEAD) * D; // the window's first input sample; negative at a track's head
    const int Wn = (n_out + 2 * LEAD) * D;      // its samples
    switch (C) {                                // 1. the window, mixed -> LDS
        case 1: rs_stage_mix<D, 1>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
        case 2: rs_stage_mix<D, 2>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
        case 3: rs_stage_mix<D, 3>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
        case 4: rs_stage_mix<D, 4>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
        case 5: rs_stage_mix<D, 5>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
        case 6: rs_stage_mix<D, 6>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
        case 7: rs_stage_mix<D, 7>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
        default: rs_stage_mix<D, 8>(lds, in, sp, mx, n0, Wn, Q, tile, planar, tid); break;
    }
    __syncthreads();
    rs_mac<D>(lds, yo, CO, tile_shift, n_out, planar, tid);          // 2. and 3. as in k_tracks_resample
    rs_store(yo, sp, tl, CO, n_out, tile, format, planar, out, tid);
}

// ---- host side ----------------------------------------------------------------------------------------
// 48000 / rate for the rates there are, else 0
static int rs_factor(int rate) {
    switch (rate) {
        case 48000: return 1;
        case 24000: return 2;
        case 16000: return 3;
        case 12000: return 4;
        case 8000: return 6;
    }
    return 0;
}
static int64_t rs_round64(int64_t v) { return (v + 63) / 64 * 64; }

// CHANNEL MIX: what a matrix for tracks of `channels` channels must keep.
static bool rs_mix_ok(const opusgpu_mix_matrix &m, int channels) {
    if (m.out_channels < 1 || m.out_channels > 8 || m.in_channels < 1 || m.in_channels > 8 || m.in_channels != channels) return false;
    for (int o = 0; o < m.out_channels; o++) {
        int sum = 0;
        for (int c = 0; c < m.in_channels; c++) sum += std::abs((int)m.m[o][c]);
        if (sum > 65535) return false;
    }
    return true;
}
// The matrix as the kernel takes it: pair[o][k] = (M[o][k - 1], M[o][k]), entries outside the matrix 0 whatever the record holds.
static RsMixArgs rs_mix_args(const opusgpu_mix_matrix &m) {
    RsMixArgs a{};
    a.co = m.out_channels;
    for (int o = 0; o < m.out_channels; o++)
        for (int k = 0; k <= 8; k++) {
            const u32 lo = k >= 1 && k - 1 < m.in_channels ? (uint16_t)m.m[o][k - 1] : 0, hi = k < m.in_channels ? (uint16_t)m.m[o][k] : 0;
            a.pair[o][k] = lo | hi << 16;
        }
    return a;
}

// What every resampling call refuses before any device work: -> the factor D, or 0.  With a matrix there is no `mono`, and 48000
// is the mix alone.
static int rs_args_factor(int channels, int rate, int mono, int format, const opusgpu_mix_matrix *mix = nullptr) {
    const int D = rs_factor(rate);
    if (!D || channels < 1 || channels > 8) return 0;
    if (mix ? mono || !rs_mix_ok(*mix, channels) : (D == 1 && !mono) || (mono && channels > 2)) return 0;
    if (format != OPUSGPU_TRACKS_S16 && format != OPUSGPU_TRACKS_F32 && format != OPUSGPU_TRACKS_F32_PLANAR) return 0;
    return D;
}
// A files call's scale: none with S16, finite entries otherwise (track_places' rule).
static bool rs_scale_ok(int format, const float *scale, int n) {
    if (format == OPUSGPU_TRACKS_S16) return !scale;
    for (int i = 0; scale && i < n; i++)
        if (!std::isfinite(scale[i])) return false;
    return true;
}

// A tile's outputs per channel, as a shift: 1,024 outputs of one channel .. 256 of eight, four per lane of k_tracks_resample.
static int rs_tile_shift(int CO) { return CO == 1 ? 10 : CO == 2 ? 9 : 8; }
// The spans held against the rules of opusgpu_resample_span for tracks of ceil(in_samples * up / down) outputs (TRACK RATES: up 1,
// down D), and the tile table of their outputs; false: a span breaks a rule, or there are more tiles than a grid takes.
static bool rs_tiles(int n_tracks, const opusgpu_resample_span *spans, int up, int down, int tile_shift, int format,
                     std::vector<ResampleTile> &tiles) {
    const int64_t tile = (int64_t)1 << tile_shift;
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_resample_span &sp = spans[t];
        if (sp.in_offset < 0 || sp.in_offset % 8 || sp.in_samples < 0 || sp.out_offset < 0 || sp.out_offset % 64) return false;
        if (sp.in_samples > INT64_MAX / 256) return false; // in_samples * up stays an int64
        const int64_t out_len = (sp.in_samples * up + down - 1) / down;
        if (format == OPUSGPU_TRACKS_F32_PLANAR && (sp.out_plane % 64 || sp.out_plane < out_len)) return false;
        if (format != OPUSGPU_TRACKS_S16 && !std::isfinite(sp.scale)) return false;
        if ((out_len + tile - 1) / tile + (int64_t)tiles.size() > 0x7fffffff) return false;
        for (int64_t m = 0; m < out_len; m += tile) tiles.push_back(ResampleTile{t, 0, m});
    }
    return true;
}

// The kernel over n tracks: checks the spans, builds the tile table, uploads both, launches on `s` and waits.
static int tracks_resample_run(int device, hipStream_t s, int n_tracks, const opusgpu_resample_span *spans, const void *d_in, int channels,
                               int rate, int mono, int format, void *d_out, const TrackFail &hip_failed,
                               const opusgpu_mix_matrix *mix = nullptr) {
    const int D = rs_args_factor(channels, rate, mono, format, mix);
    if (!D || n_tracks < 0 || (n_tracks && !spans)) return OPUSGPU_BAD_ARG;
    const int CO = mix ? mix->out_channels : mono ? 1 : channels;
    const int tile_shift = rs_tile_shift(CO);
    std::vector<ResampleTile> tiles;
    if (!rs_tiles(n_tracks, spans, 1, D, tile_shift, format, tiles)) return OPUSGPU_BAD_ARG;
    const int64_t tile = (int64_t)1 << tile_shift;
    if (tiles.empty()) return OPUSGPU_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 127)) return OPUSGPU_BAD_ARG;
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles;
    TRK_CHK(d_spans.upload(spans, (size_t)n_tracks * sizeof(ResampleSpan)));
    TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(ResampleTile)));
    const size_t lds = ((size_t)CO * D * (tile + RS_PLANE_PAD) + (size_t)CO * tile) * 2;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles.size()), dim3(256), lds, s, (const ResampleTile *)d_tiles.p, (const ResampleSpan *)d_spans.p,
                           (const i16 *)d_in, channels, mono ? 1 : 0, format, tile_shift, d_out);
    };
    const RsMixArgs mx = mix ? rs_mix_args(*mix) : RsMixArgs{};
    auto go_mix = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles.size()), dim3(256), lds, s, (const ResampleTile *)d_tiles.p, (const ResampleSpan *)d_spans.p,
                           (const i16 *)d_in, channels, mx, format, tile_shift, d_out);
    };
    switch (mix ? -D : D) {
        case 1: go(k_tracks_resample<1>); break;
        case 2: go(k_tracks_resample<2>); break;
        case 3: go(k_tracks_resample<3>); break;
        case 4: go(k_tracks_resample<4>); break;
        case 6: go(k_tracks_resample<6>); break;
        case -1: go_mix(k_tracks_resample_mix<1>); break;
        case -2: go_mix(k_tracks_resample_mix<2>); break;
        case -3: go_mix(k_tracks_resample_mix<3>); break;
        case -4: go_mix(k_tracks_resample_mix<4>); break;
        default: go_mix(k_tracks_resample_mix<6>); break;
    }
    TRK_CHK(hipGetLastError());
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// The spans of a planned batch whose S16 tracks have been decoded: final lengths in, the grid of the tracks at up / down of their
// rate out (TRACK RATES: up 1, down D).
static void rs_batch_spans(const og_batch &b, int up, int down, const int64_t *final_lengths, const float *scale,
                           std::vector<int64_t> &out_offsets, std::vector<opusgpu_resample_span> &spans) {
    const size_t n = (size_t)b.n_files;
    out_offsets.resize(n);
    spans.resize(n);
    int64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        const int64_t plane = rs_round64((b.info[i].track_samples * up + down - 1) / down);
        out_offsets[i] = at;
        spans[i] = opusgpu_resample_span{b.info[i].track_offset, final_lengths[i], at, plane, scale ? scale[i] : 1.0f / 32768, 0};
        at += plane;
    }
}

// WAVE BATCHES (og_wave_batch.hpp, behind the feature headers): the stage that turns packed int16 tracks into the dense tensor.
static const char *wave_batch_shape_wrong(const opusgpu_wave_batch_req &r, int C, int format);
static int wave_batch_run(int device, hipStream_t s, int n_tracks, const opusgpu_wave_span *spans, int C, int format,
                          const opusgpu_wave_batch_req *req, const void *d_s16, void *d_out, opusgpu_wave_stat *recs,
                          const TrackFail &hip_failed, const std::function<void(const char *)> &why);
// WAVE TRIM (og_wave_trim.hpp, behind it): the stage in front of the wave batch that cuts leading and trailing silence off its spans.
static int wave_trim_spans(const FilesOwner &own, WaveTrimState &st, std::vector<opusgpu_wave_span> &tracks, int C, const void *d_s16);
#define OG_TRIM_NEEDS_BATCH                                                                                                        \
    "wave trim: a request is on without a wave-batch request -- the packed grids are planned on the host and cannot shrink, only " \
    "the dense tensor's rows can"

// What every whole-file call that ends in a resampling kernel does around its owner's decoder, its arguments checked by the caller:
// own.decode runs the batch into the scratch S16 tracks, `run(n, spans, d_s16, format, d_dst)` the kernel that makes tracks of CO
// channels at up / down of their rate from them, in `format` at d_dst.  That is the call's own format and d_out -- unless the owner
// holds a WAVE BATCHES request and the tracks are the call's result (they are not where they feed a feature kernel): then the
// kernel writes int16 into a scratch grid of its own layout and wave_batch_run writes d_out from there -- from the spans that
// wave_trim_spans has shortened first, where the owner holds a WAVE TRIM request as well.
template <class Run>
static int files_resampled_to(const FilesOwner &own, int up, int down, int CO, int format, const float *scale, void *d_out,
                              int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out, int32_t *status_out, Run run) {
    const og_batch &b = own.b;
    if (!rs_scale_ok(format, scale, b.n_files)) return OPUSGPU_BAD_ARG;
    // TRACK LOUDNESS: int16 tracks take no gain, unless they only feed a feature kernel that applies it
    if (loud_normalizes(own) && format == OPUSGPU_TRACKS_S16 && !own.scale_later) return OPUSGPU_BAD_ARG;
    if (loud_on(own) && own.loud->req.n_weights && own.loud->req.n_weights != b.channels) return OPUSGPU_BAD_ARG;
    const size_t n = (size_t)b.n_files;
    WaveBatchState *const wb = own.wave && own.wave->req.enabled && !own.scale_later ? own.wave : nullptr;
    WaveTrimState *const trim = own.trim && own.trim->req.enabled && !own.scale_later ? own.trim : nullptr;
    if (trim && !wb) {
        if (own.refused) own.refused(OG_TRIM_NEEDS_BATCH);
        return OPUSGPU_BAD_ARG;
    }
    int64_t mid_total = 0; // the scratch grid of a wave batch, in samples per channel
    if (wb) {
        const char *bad = wave_batch_shape_wrong(wb->req, CO, format);
        for (size_t i = 0; i < n && !bad; i++) {
            const int64_t planned = (b.info[i].track_samples * up + down - 1) / down;
            if (planned > wb->req.stride_samples) bad = "wave batch: stride_samples is below a track's planned output length";
            mid_total += rs_round64(planned);
        }
        if (bad) {
            if (own.refused) own.refused(bad);
            return OPUSGPU_BAD_ARG;
        }
    }
    std::vector<int64_t> lengths(n, 0), offsets;
    std::vector<int32_t> status(2 * n, 0);
    std::vector<opusgpu_resample_span> spans;
    RsDevBuf s16; // the int16 tracks: track_samples x channels, for the length of this call
    RsDevBuf mid; // WAVE BATCHES: the int16 tracks at the output's rate and channels, for the length of this call
    if (!b.segs.empty()) {
        hipError_t e = hipSetDevice(own.device);
        if (e == hipSuccess) e = s16.alloc((size_t)b.track_samples * b.channels * 2);
        if (e == hipSuccess && wb) e = mid.alloc((size_t)mid_total * CO * 2 + 128);
        if (e != hipSuccess) return own.hip_failed(OPUSGPU_ALLOC_FAIL, "hipMalloc(resample scratch)", e);
    }
    if (int rc = own.decode(s16.p, lengths.data(), status.data())) return rc;
    if (loud_on(own)) // the S16 tracks at their final lengths, all decoded channels, in front of the mix and the rate
        if (int rc = files_loudness(own, s16.p, lengths.data())) return rc;
    rs_batch_spans(b, up, down, lengths.data(), scale, offsets, spans);
    if (loud_normalizes(own) && format != OPUSGPU_TRACKS_S16)
        for (size_t i = 0; i < n; i++) spans[i].scale = loud_scale(own, scale, i);
    if (int rc = run(b.n_files, spans.data(), s16.p, wb ? (int)OPUSGPU_TRACKS_S16 : format, wb ? mid.p : d_out)) return rc;
    if (wb) {
        std::vector<opusgpu_wave_span> tracks(n);
        std::vector<opusgpu_wave_stat> recs(n);
        for (size_t i = 0; i < n; i++) {
            tracks[i] = opusgpu_wave_span{offsets[i], (lengths[i] * up + down - 1) / down, spans[i].scale, 0};
            offsets[i] = (int64_t)i * wb->req.stride_samples;
        }
        if (trim) // WAVE TRIM: the wave batch sees the tracks without their leading and trailing silence
            if (int rc = wave_trim_spans(own, *trim, tracks, CO, mid.p)) return rc;
        if (int rc = wave_batch_run(own.device, own.stream, b.n_files, tracks.data(), CO, format, &wb->req, mid.p, d_out, recs.data(),
                                    own.hip_failed, own.refused))
            return rc;
        wb->records = recs;
    }
    for (size_t i = 0; i < n; i++) {
        if (out_offsets) out_offsets[i] = offsets[i];
        if (out_lengths) out_lengths[i] = trim ? trim->records[i].count : (lengths[i] * up + down - 1) / down;
        if (track_lengths_out) track_lengths_out[i] = lengths[i];
    }
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    return OPUSGPU_OK;
}

// files_resampled_to for the rates of TRACK RATES, behind a mono downmix or a channel mix.
static int files_resampled_run(const FilesOwner &own, int rate, int mono, const opusgpu_mix_matrix *mix, int format, const float *scale,
                               void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out, int32_t *status_out) {
    const int D = rs_args_factor(own.b.channels, rate, mono, format, mix);
    if (!D) return OPUSGPU_BAD_ARG;
    return files_resampled_to(own, 1, D, mix ? mix->out_channels : mono ? 1 : own.b.channels, format, scale, d_out, out_offsets, out_lengths,
                              track_lengths_out, status_out, [&](int n, const opusgpu_resample_span *spans, const void *d_s16, int fmt, void *d_dst) {
                                  return tracks_resample_run(own.device, own.stream, n, spans, d_s16, own.b.channels, rate, mono, fmt, d_dst,
                                                             own.hip_failed, mix);
                              });
}

extern "C" {

int opusgpu_resample_taps(int rate, const int16_t **taps) {
    const int16_t *h = nullptr;
    switch (rate) {
        case 24000: h = og_rs_taps_2; break;
        case 16000: h = og_rs_taps_3; break;
        case 12000: h = og_rs_taps_4; break;
        case 8000: h = og_rs_taps_6; break;
        default: return OPUSGPU_BAD_ARG; // 48000 included: the downmix has no table (its one tap, 32768, is no int16)
    }
    if (taps) *taps = h;
    return 24 * rs_factor(rate) + 1;
}

int64_t opusgpu_resample_layout(int n, const int64_t *planned_samples, int rate, int64_t *out_offsets) {
    const int D = rs_factor(rate);
    if (!D || n < 0 || (n && !planned_samples)) return OPUSGPU_BAD_ARG;
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        if (planned_samples[i] < 0) return OPUSGPU_BAD_ARG;
        if (out_offsets) out_offsets[i] = at;
        at += rs_round64((planned_samples[i] + D - 1) / D);
    }
    return at;
}

int opusgpu_tracks_resample_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_resample_span *spans, const void *d_in, int channels, int rate,
                                   int mono, int format, void *d_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_resample_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in, channels, rate, mono,
                               format, d_out, track_fail(ctx));
}

int opusgpu_files_decode_resampled(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int mono, int format, const float *scale,
                                   void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                                   int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    return files_resampled_run(files_owner(ctx, batch), rate, mono, nullptr, format, scale, d_out, out_offsets, out_lengths, track_lengths_out,
                               status_out);
}

int opusgpu_downmix_matrix(int channels, int out_channels, opusgpu_mix_matrix *m) {
    if (channels < 1 || channels > 8 || out_channels < 1 || out_channels > 2 || !m) return OPUSGPU_BAD_ARG;
    *m = opusgpu_mix_matrix{};
    m->out_channels = out_channels, m->in_channels = channels;
    for (int o = 0; o < out_channels; o++)
        for (int c = 0; c < channels; c++) m->m[o][c] = out_channels == 1 ? og_downmix_mono[channels - 1][c] : og_downmix_stereo[channels - 1][o][c];
    return OPUSGPU_OK;
}

int opusgpu_tracks_resample_mixed_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_resample_span *spans, const void *d_in, int channels,
                                         int rate, const opusgpu_mix_matrix *mix, int format, void *d_out, void *hip_stream) {
    if (!ctx || !mix) return OPUSGPU_BAD_ARG;
    return tracks_resample_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in, channels, rate, 0, format,
                               d_out, track_fail(ctx), mix);
}

int opusgpu_files_decode_mixed(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, const opusgpu_mix_matrix *mix, int format,
                               const float *scale, void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                               int32_t *status_out) {
    if (!ctx || !batch || !mix) return OPUSGPU_BAD_ARG;
    return files_resampled_run(files_owner(ctx, batch), rate, 0, mix, format, scale, d_out, out_offsets, out_lengths, track_lengths_out,
                               status_out);
}

} // extern "C"
