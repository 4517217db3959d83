// og_tracks_resample_ratio.hpp -- tracks at up / down of 48 kHz by a rational polyphase FIR (include/opusgpu.h, TRACK RATIOS: 44.1 kHz
// is 147 / 160, 32 kHz 2 / 3, 22.05 kHz 147 / 320): the tap builder, the kernel, its host side and the whole-file call that ends in
// it.  Included at the end of og_api.hip behind og_tracks_resample.hpp, whose tile table, staging (rs_stage, rs_stage_mix_at),
// rs_dot2, rs_store and whole-file driver (files_resampled_to) it shares, and in front of og_ms_tracks.hpp.
#pragma once
#include <map>
#include <utility>

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_resample_ratio: one workgroup per entry of k_tracks_resample's tile table, `tile` consecutive outputs of every output
// channel of one track.  Output m sits at t = m down + c on the 48000 up grid (c = 12 down): its phase is p = t mod up, its newest
// input sample b = floor(t / up), and with T = ceil(Lp / up) taps per phase
//     y[m] = sum_i row_p[i] x[b - T + 1 + i],   row_p[i] = h[p + (T - 1 - i) up],  i in [0, R), R = T rounded up to 4,
// row entries whose tap index falls outside [0, Lp) being 0.
//   1. STAGE.  The tile's window -- the samples from b - T + 1 of its first output to b - T + R of its last, Wn of them -- comes in
//      through k_tracks_resample's staging (aligned 16-byte loads, nothing fetched behind the piece that holds the track's last
//      sample, zeros outside [0, in_samples), `mono` and the Q14 mix formed here) and is kept TWICE per output channel: plane A
//      holds window sample r at place r, plane B at place r - 1.  An output whose first sample lies at an even r reads A, one at an
//      odd r reads B: either way its samples (r + 2 k, r + 2 k + 1) are one aligned 32-bit word, the operand of v_dot2_i32_i16.
//      The tap rows come into LDS as well, from a table the host has ordered [group of 4 taps][m mod up][4]: the phase depends on
//      m mod up alone, so the lanes of a wave, which own consecutive m, read consecutive 8-byte slots of a group (ds_read_b64 over a
//      whole bank row) however far apart their phases are -- a phase-major table would put them T half-words apart, on a few banks.
//      Every window word that an output which is stored reads has been written: its last word ends at place s + R - 1 <= Wn - 1 of
//      A, one less of B.  Places T .. R - 1 of a row are zero taps (as are those whose tap lies behind Lp); they meet samples that
//      were staged like any other.  The only words read that nobody wrote are results behind the tile's last one, which a partial
//      last piece of step 3 loads and does not store.  The arithmetic is integer: there is no NaN to spread.
//   2. MAC.  A lane owns one output of one channel: R / 4 steps of one 8-byte tap read, two window words and two v_dot2_i32_i16.
//      The sum starts at 16384 and is exact in int32 (a phase's sum |h| <= 65535, held where the taps are made); >> 15 and the
//      clamp make the int16 result, which goes to the result area in the order of the destination.
//   3. STORE.  rs_store, as in k_tracks_resample.
// All arithmetic on m down is 64-bit up to the tile's first output; inside a tile the offsets are below 2^20.
struct RrArgs {
    i32 up, down;
    i32 taps_per_phase; // T
    i32 groups;         // R / 4
    i32 plane;          // places of a window plane (int16), a multiple of 8, 32 mod 64: planes A and B lie half a bank row apart
    i32 has_mix;
};

__global__ void __launch_bounds__(256) k_tracks_resample_ratio(const ResampleTile *__restrict__ tiles, const ResampleSpan *__restrict__ spans,
                                                                const i16 *__restrict__ in, int C, int mono, RsMixArgs mx, RrArgs ra,
                                                                const uint4 *__restrict__ taps, int format, int tile_shift,
                                                                void *__restrict__ out) {
    extern __shared__ __align__(16) i16 lds[]; // [CO][A, B] planes of ra.plane places, the tap groups [groups][up] of 8 bytes, the results
    const int tid = (int)threadIdx.x;
    const ResampleTile tl = tiles[blockIdx.x];
    const ResampleSpan sp = spans[tl.track];
    const int tile = 1 << tile_shift, Q = ra.plane, up = ra.up, down = ra.down;
    const int CO = ra.has_mix ? mx.co : mono ? 1 : C;
    const long long out_len = (sp.in_samples * up + down - 1) / down;
    const long long left = out_len - tl.first;
    const int n_out = left < tile ? (int)left : tile;
    if (n_out <= 0) return;
    const int tap_pieces = (ra.groups * up + 1) >> 1; // 16-byte pieces of the tap table
    uint2 *const tp = reinterpret_cast<uint2 *>(lds + 2 * CO * Q);
    i16 *const yo = lds + 2 * CO * Q + 8 * tap_pieces;
    const bool planar = format == OPUSGPU_TRACKS_F32_PLANAR;
    const long long t0 = tl.first * down + 12LL * down; // the first output on the fine grid
    const long long b0 = t0 / up;
    const int p0 = (int)(t0 - b0 * up), mm0 = (int)(tl.first % up);
    const int R = 4 * ra.groups;
    const int Wn = (p0 + (n_out - 1) * down) / up + R; // the window's samples: <= ra.plane (tracks_resample_ratio_run)
    const long long n0 = b0 - ra.taps_per_phase + 1;   // its first; negative at a track's head

    // 1. the taps and the window -> LDS
    for (int q = tid; q < tap_pieces; q += 256) reinterpret_cast<uint4 *>(tp)[q] = taps[q];
    auto put = [=](int o, int r, i16 x) {
        lds[2 * o * Q + r] = x;
        if (r) lds[(2 * o + 1) * Q + r - 1] = x;
    };
    if (ra.has_mix) {
        auto at_of = [](int r) { return r; };
        switch (C) {
            case 1: rs_stage_mix_at<1>(in, sp, mx, n0, Wn, tid, at_of, put); break;
            case 2: rs_stage_mix_at<2>(in, sp, mx, n0, Wn, tid, at_of, put); break;
            case 3: rs_stage_mix_at<3>(in, sp, mx, n0, Wn, tid, at_of, put); break;
            case 4: rs_stage_mix_at<4>(in, sp, mx, n0, Wn, tid, at_of, put); break;
            case 5: rs_stage_mix_at<5>(in, sp, mx, n0, Wn, tid, at_of, put); break;
            case 6: rs_stage_mix_at<6>(in, sp, mx, n0, Wn, tid, at_of, put); break;
            case 7: rs_stage_mix_at<7>(in, sp, mx, n0, Wn, tid, at_of, put); break;
            default: rs_stage_mix_at<8>(in, sp, mx, n0, Wn, tid, at_of, put); break;
        }
    } else {
        rs_stage(in, sp, C, mono != 0, n0, Wn, tid, put);
    }
    __syncthreads();

    // 2. one output per lane
    for (int x = tid; x < CO << tile_shift; x += 256) {
        const int c = x >> tile_shift, j = x & (tile - 1);
        if (j >= n_out) continue;
        const int s = (p0 + j * down) / up; // the output's first sample in the window
        const u32 *const xw = reinterpret_cast<const u32 *>(lds + (2 * c + (s & 1)) * Q + (s & ~1));
        const uint2 *const row = tp + (mm0 + j) % up;
        i32 acc = 16384;
        for (int g = 0; g < ra.groups; g++) {
            const uint2 h = row[g * up];
            acc = rs_dot2(xw[2 * g], h.x, acc);
            acc = rs_dot2(xw[2 * g + 1], h.y, acc);
        }
        acc >>= 15;
        yo[planar ? c * tile + j : j * CO + c] = (i16)(acc < -32768 ? -32768 : acc > 32767 ? 32767 : acc);
    }
    __syncthreads();

    rs_store(yo, sp, tl, CO, n_out, tile, format, planar, out, tid); // 3. LDS -> the track
}

// ---- taps ---------------------------------------------------------------------------------------------
// TRACK RATIOS, TAPS: the table of one reduced ratio, made in double at first use and kept for the life of the process.
struct RrTaps {
    int up = 0, down = 0, lp = 0, taps_per_phase = 0, groups = 0;
    std::vector<int16_t> h;     // [lp], what opusgpu_resample_ratio_taps hands out
    std::vector<int16_t> rows;  // the kernel's order [groups][up][4], padded to whole 16-byte pieces
};

static double rr_bessel_i0(double x) { // sum_k ((x / 2)^k / k!)^2: every term positive, below 1e-17 of the sum within 40 terms for x <= 8
    double sum = 1, term = 1;
    for (int k = 1; k < 64; k++) {
        term *= (x / 2) / k;
        sum += term * term;
    }
    return sum;
}

// 1 <= up <= 160, up < down <= min(8 up, 640), after the gcd has been taken out; false: not a ratio of TRACK RATIOS
static bool rr_reduce(int &up, int &down) {
    if (up < 1 || down < 1) return false;
    int a = up, b = down;
    while (b) {
        const int t = a % b;
        a = b, b = t;
    }
    up /= a, down /= a;
    return up <= 160 && up < down && down <= 8 * up && down <= 640;
}

static bool rr_taps_make(int up, int down, RrTaps &t) {
    const double pi = 3.14159265358979323846;
    const int lp = 24 * down + 1, c = 12 * down;
    const double fc = 0.92 / down, i0_8 = rr_bessel_i0(8.0);
    std::vector<double> g((size_t)lp);
    for (int i = 0; i < lp; i++) {
        const double d = i - c, a = pi * fc * d, u = d / c;
        g[(size_t)i] = fc * (d == 0 ? 1.0 : std::sin(a) / a) * rr_bessel_i0(8.0 * std::sqrt(std::max(0.0, 1 - u * u))) / i0_8;
    }
    t.up = up, t.down = down, t.lp = lp;
    t.taps_per_phase = (lp + up - 1) / up;
    t.groups = (t.taps_per_phase + 3) / 4;
    t.h.assign((size_t)lp, 0);
    for (int p = 0; p < up; p++) { // each phase: DC gain exactly 1 in Q15
        double sum = 0;
        for (int i = p; i < lp; i += up) sum += g[(size_t)i];
        if (!(sum > 0)) return false;
        long long total = 0, abs_total = 0;
        int best = p;
        long long best_v = INT64_MIN;
        for (int i = p; i < lp; i += up) {
            const long long v = (long long)std::nearbyint(g[(size_t)i] * (32768.0 / sum));
            if (v > best_v) best_v = v, best = i; // the largest, the first of them when tied
            t.h[(size_t)i] = (int16_t)v;
            total += v;
        }
        const long long fixed = best_v + (32768 - total);
        if (fixed < -32768 || fixed > 32767) return false;
        t.h[(size_t)best] = (int16_t)fixed;
        for (int i = p; i < lp; i += up) abs_total += std::abs((int)t.h[(size_t)i]);
        if (abs_total > 65535) return false; // what keeps the kernel's int32 sum exact
    }
    // the kernel's rows: output m takes phase (m down + c) mod up, which depends on m mod up alone
    const int R = 4 * t.groups, T = t.taps_per_phase;
    t.rows.assign(((size_t)t.groups * up * 4 + 7) / 8 * 8, 0);
    for (int mm = 0; mm < up; mm++) {
        const int p = (int)(((long long)mm * down + c) % up);
        for (int i = 0; i < R; i++) {
            const long long k = p + (long long)(T - 1 - i) * up;
            t.rows[((size_t)(i / 4) * up + mm) * 4 + (i & 3)] = i < T && k < lp ? t.h[(size_t)k] : (int16_t)0;
        }
    }
    return true;
}

// The table of a REDUCED ratio of TRACK RATIOS, or null should its builder refuse it; safe from any number of threads.
static const RrTaps *rr_taps(int up, int down) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, std::unique_ptr<RrTaps>> cache;
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({up, down});
    if (it == cache.end()) {
        std::unique_ptr<RrTaps> t(new RrTaps);
        if (!rr_taps_make(up, down, *t)) t.reset();
        it = cache.emplace(std::make_pair(up, down), std::move(t)).first;
    }
    return it->second.get();
}

// ---- host side ----------------------------------------------------------------------------------------
// What every ratio call refuses before any device work: -> the table of the reduced ratio (up and down reduced in place), or null.
// `mono` and a mix exclude each other; without either all channels go through.
static const RrTaps *rr_args_taps(int channels, int &up, int &down, int mono, int format, const opusgpu_mix_matrix *mix) {
    if (!rr_reduce(up, down) || channels < 1 || channels > 8) return nullptr;
    if (mix ? mono || !rs_mix_ok(*mix, channels) : mono && channels > 2) return nullptr;
    if (format != OPUSGPU_TRACKS_S16 && format != OPUSGPU_TRACKS_F32 && format != OPUSGPU_TRACKS_F32_PLANAR) return nullptr;
    return rr_taps(up, down);
}

// A launch's tile and LDS: k_tracks_resample's tile for CO channels, halved while a workgroup would take more than 64 KB (eight
// channels at 1 / 8 or at 147 / 640 do at 256 outputs: 75 KB), so that two workgroups always fit a CU's 160 KB.
struct RrPlan {
    int tile_shift = 0, plane = 0;
    size_t lds = 0;
};
static RrPlan rr_plan(const RrTaps &t, int CO) {
    RrPlan pl;
    for (pl.tile_shift = rs_tile_shift(CO);; pl.tile_shift--) {
        const int64_t tile = (int64_t)1 << pl.tile_shift;
        // the widest window: the first output at phase up - 1, the last (tile - 1) down further on, and a row behind it
        const int64_t wn = ((t.up - 1) + (tile - 1) * t.down) / t.up + 4 * t.groups;
        pl.plane = (int)((wn + 31) / 64 * 64 + 32); // >= wn, 32 mod 64
        pl.lds = ((size_t)2 * CO * pl.plane + (size_t)(t.groups * t.up + 1) / 2 * 8 + (size_t)CO * tile) * 2;
        if (pl.lds <= 65536 || pl.tile_shift == 5) return pl;
    }
}

// The kernel over n tracks, as tracks_resample_run: checks the spans, builds the tile table, uploads it, the spans and the tap rows,
// launches on `s` and waits.
static int tracks_resample_ratio_run(int device, hipStream_t s, int n_tracks, const opusgpu_resample_span *spans, const void *d_in,
                                     int channels, int up, int down, int mono, const opusgpu_mix_matrix *mix, int format, void *d_out,
                                     const TrackFail &hip_failed) {
    const RrTaps *const t = rr_args_taps(channels, up, down, mono, format, mix);
    if (!t || n_tracks < 0 || (n_tracks && !spans)) return OPUSGPU_BAD_ARG;
    const int CO = mix ? mix->out_channels : mono ? 1 : channels;
    const RrPlan pl = rr_plan(*t, CO);
    std::vector<ResampleTile> tiles;
    if (!rs_tiles(n_tracks, spans, up, down, pl.tile_shift, format, tiles)) return OPUSGPU_BAD_ARG;
    if (tiles.empty()) return OPUSGPU_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 127)) return OPUSGPU_BAD_ARG;
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles, d_taps;
    TRK_CHK(d_spans.upload(spans, (size_t)n_tracks * sizeof(ResampleSpan)));
    TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(ResampleTile)));
    TRK_CHK(d_taps.upload(t->rows.data(), t->rows.size() * sizeof(int16_t)));
    const RrArgs ra{up, down, t->taps_per_phase, t->groups, pl.plane, mix ? 1 : 0};
    const RsMixArgs mx = mix ? rs_mix_args(*mix) : RsMixArgs{};
    hipLaunchKernelGGL(k_tracks_resample_ratio, dim3((unsigned)tiles.size()), dim3(256), pl.lds, s, (const ResampleTile *)d_tiles.p,
                       (const ResampleSpan *)d_spans.p, (const i16 *)d_in, channels, mono ? 1 : 0, mx, ra, (const uint4 *)d_taps.p, format,
                       pl.tile_shift, d_out);
    TRK_CHK(hipGetLastError());
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// files_resampled_to for a ratio: what opusgpu_files_decode_ratio and opusgpu_ms_files_decode_ratio (og_ms_tracks.hpp) share.
static int files_ratio_run(const FilesOwner &own, int up, int down, int mono, const opusgpu_mix_matrix *mix, int format, const float *scale,
                           void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out, int32_t *status_out) {
    if (!rr_args_taps(own.b.channels, up, down, mono, format, mix)) return OPUSGPU_BAD_ARG;
    return files_resampled_to(own, up, down, mix ? mix->out_channels : mono ? 1 : own.b.channels, format, scale, d_out, out_offsets, out_lengths,
                              track_lengths_out, status_out, [&](int n, const opusgpu_resample_span *spans, const void *d_s16, int fmt, void *d_dst) {
                                  return tracks_resample_ratio_run(own.device, own.stream, n, spans, d_s16, own.b.channels, up, down, mono, mix,
                                                                   fmt, d_dst, own.hip_failed);
                              });
}

extern "C" {

int opusgpu_resample_ratio_taps(int up, int down, const int16_t **taps) {
    if (!rr_reduce(up, down)) return OPUSGPU_BAD_ARG;
    const RrTaps *const t = rr_taps(up, down);
    if (!t) return OPUSGPU_BAD_ARG;
    if (taps) *taps = t->h.data();
    return t->lp;
}

int64_t opusgpu_resample_ratio_layout(int n, const int64_t *planned_samples, int up, int down, int64_t *out_offsets) {
    if (!rr_reduce(up, down) || n < 0 || (n && !planned_samples)) return OPUSGPU_BAD_ARG;
    int64_t at = 0;
    for (int i = 0; i < n; i++) {
        if (planned_samples[i] < 0 || planned_samples[i] > INT64_MAX / 256) return OPUSGPU_BAD_ARG;
        if (out_offsets) out_offsets[i] = at;
        at += rs_round64((planned_samples[i] * up + down - 1) / down);
    }
    return at;
}

int opusgpu_tracks_resample_ratio_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_resample_span *spans, const void *d_in, int channels,
                                         int up, int down, int mono, const opusgpu_mix_matrix *mix, int format, void *d_out,
                                         void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_resample_ratio_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in, channels, up, down,
                                     mono, mix, format, d_out, track_fail(ctx));
}

int opusgpu_files_decode_ratio(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int up, int down, int mono, const opusgpu_mix_matrix *mix,
                               int format, const float *scale, void *d_out, int64_t *out_offsets, int64_t *out_lengths,
                               int64_t *track_lengths_out, int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    return files_ratio_run(files_owner(ctx, batch), up, down, mono, mix, format, scale, d_out, out_offsets, out_lengths, track_lengths_out,
                           status_out);
}

} // extern "C"
