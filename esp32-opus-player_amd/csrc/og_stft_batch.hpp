// og_stft_batch.hpp -- STFT batches (include/opusgpu.h, STFT BATCHES): the packed grid of TRACK STFT, up to 1025 bins of real cells or
// (Re, Im) pairs, collated into one dense tensor of n * S * bins * c floats, every track normalised by statistics of its own real
// cells and padded to S frames.  Included by og_api.hip behind og_tracks_stft.hpp, whose whole-file call (files_stft_run) ends here
// when the owner holds a request, and behind og_feat_batch.hpp, whose partial and statistics records and whose accumulation step
// (fbat_take) it shares so that a bin's sums are the same bits in both stages.  FEATURE BATCHES' kernels are not touched.  DESIGN.md
// section 13n.
#pragma once

// ---- kernels ------------------------------------------------------------------------------------------
// The general path is FEATURE BATCHES' stage at any width: the grid is read once for the statistics (norms that have any) and once
// for the tensor, the tensor is written once.  All plain vector loads and stores, no scratch:
//   k_stft_stats  a workgroup of four waves per (track, segment of FBAT_SEG frames, chunk of 128 bins): per bin the segment's max
//                 (WHISPER, REFMAX) or its sum and sum of squares in double (CMN, CMVN), into the partial table at
//                 (place[t] + segment) * bins + bin.  The chunk keeps the frames-major combine at k_feat_stats' 8,192 bytes of LDS;
//   k_stft_fold   one wave per (track, chunk of 128 bins): folds the segments in ascending order and leaves per bin what the cells
//                 need -- the track's max, or the mean and the divisor;
//   k_stft_batch  a lane owns an aligned 16-byte piece of the DESTINATION, fetches its four floats or pad values and stores it whole.
// The direct path (norm NONE, S a multiple of 64) has k_tracks_stft write the real cells into the tensor itself, and
//   k_stft_pad    writes the cells f in [F[t], S) of every track, and nothing else.
// Pairs (c = 2) are rows of twice the floats: element b of a row is member b & 1 of cell b >> 1, so one index walk serves both.
struct SbatTile {
    i32 track, seg, chunk;
};
struct SbatArgs {
    long long S;
    double var_floor;
    int B, c, frames_major, norm, pad_normalized;
    float pad_value, range, add, mul;
};
static_assert(sizeof(opusgpu_stft_batch_req) == 64 && sizeof(opusgpu_stft_batch_span) == 24, "stft batch records");
static_assert(sizeof(opusgpu_stft_batch_req) == sizeof(opusgpu_feat_batch_req), "the fields of opusgpu_feat_batch_req");
constexpr int SBAT_CHUNK = 128;    // bins of a workgroup of k_stft_stats and of a wave of k_stft_fold
constexpr int SBAT_MAX_BINS = 1025;

__device__ __forceinline__ bool sbat_keeps_max(int norm) { return norm == OPUSGPU_FEAT_NORM_WHISPER || norm == OPUSGPU_STFT_NORM_REFMAX; }

// k_feat_stats over one chunk of bins: the same cells in the same order per bin, whatever `bins` is.
__global__ void __launch_bounds__(256) k_stft_stats(const SbatTile *__restrict__ tiles, const FbatSpan *__restrict__ spans,
                                                    const float *__restrict__ grid, SbatArgs A, FbatPart *__restrict__ part) {
    __shared__ double red[4][SBAT_CHUNK][2];
    static_assert(sizeof(red) == FBAT_COMBINE_LDS, "the combine's LDS is k_feat_stats'");
    const SbatTile tile = tiles[blockIdx.x];
    const FbatSpan sp = spans[tile.track];
    const int B = A.B, lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const bool mxn = sbat_keeps_max(A.norm);
    const int k0 = SBAT_CHUNK * tile.chunk, nb = B - k0 < SBAT_CHUNK ? B - k0 : SBAT_CHUNK; // this chunk's bins, >= 1
    const long long f0 = (long long)tile.seg * FBAT_SEG;
    const int nf = (int)(sp.frames - f0 < FBAT_SEG ? sp.frames - f0 : FBAT_SEG); // this segment's real frames, >= 1
    FbatPart *out = part + (sp.place + tile.seg) * B + k0;
    const float NEG = -__builtin_inff();
    if (!A.frames_major) {
        // a wave per bin row: the row's segment begins at a multiple of 1024 floats from a 256-byte aligned row
        for (int j = wave; j < nb; j += 4) {
            const float *row = grid + sp.grid_offset + (long long)(k0 + j) * sp.plane + f0;
            float mx = NEG;
            double s = 0, q = 0;
#pragma unroll
            for (int k = 0; k < FBAT_SEG / 256; k++) {
                const int f = 4 * (lane + 64 * k);
                if (f < nf) { // the piece lies inside the plane: plane is a multiple of 64 and >= F
                    const float4 v = *reinterpret_cast<const float4 *>(row + f);
                    fbat_take(mxn, v.x, mx, s, q);
                    if (f + 1 < nf) fbat_take(mxn, v.y, mx, s, q);
                    if (f + 2 < nf) fbat_take(mxn, v.z, mx, s, q);
                    if (f + 3 < nf) fbat_take(mxn, v.w, mx, s, q);
                }
            }
#pragma unroll
            for (int d = 32; d; d >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, d, 64));
                s += __shfl_xor(s, d, 64);
                q += __shfl_xor(q, d, 64);
            }
            if (lane == 0) out[j] = mxn ? FbatPart{(double)mx, 0.0} : FbatPart{s, q};
        }
    } else {
        // lane <-> bin of the chunk (two bins a lane), a wave every fourth frame: 256 contiguous bytes a wave and load
        const bool two = lane + 64 < nb;
        float mx = NEG;
        double s0 = 0, q0 = 0, s1 = 0, q1 = 0;
        if (lane < nb) {
            const float *cell = grid + sp.grid_offset + f0 * B + k0 + lane;
            for (int f = wave; f < nf; f += 4) {
                fbat_take(mxn, cell[(long long)f * B], mx, s0, q0);
                if (two) fbat_take(mxn, cell[(long long)f * B + 64], mx, s1, q1);
            }
        }
        // (a max is the same in any order: it goes through the sums' slots as a double)
        red[wave][lane][0] = mxn ? (double)mx : s0, red[wave][lane][1] = q0;
        red[wave][lane + 64][0] = mxn ? (double)NEG : s1, red[wave][lane + 64][1] = q1;
        __syncthreads();
        const int j = (int)threadIdx.x;
        if (j < nb) {
            if (mxn) {
                // both bins of a lane went into slot `lane`; bin j >= 64 has nothing of its own
                const double m = fmax(fmax(red[0][j][0], red[1][j][0]), fmax(red[2][j][0], red[3][j][0]));
                out[j] = FbatPart{m, 0.0};
            } else {
                out[j] = FbatPart{((red[0][j][0] + red[1][j][0]) + red[2][j][0]) + red[3][j][0],
                                ((red[0][j][1] + red[1][j][1]) + red[2][j][1]) + red[3][j][1]};
            }
        }
    }
}

// One wave per (track, chunk of 128 bins), blockIdx.x = track * chunks + chunk; lane <-> two bins of the chunk, the segments in
// ascending order.  The track's max covers every bin, so each wave of a track folds the whole of the track's partial maxima (a few
// doubles per bin and segment) in one fixed order: the lanes stride the bins, then the butterfly.  A max has one value in any order.
__global__ void __launch_bounds__(64) k_stft_fold(const FbatSpan *__restrict__ spans, const FbatPart *__restrict__ part, SbatArgs A, int chunks,
                                                  FbatStat *__restrict__ stat) {
    const int t = (int)(blockIdx.x / (unsigned)chunks), ch = (int)(blockIdx.x % (unsigned)chunks), lane = (int)threadIdx.x, B = A.B;
    const FbatSpan sp = spans[t];
    const long long segs = (sp.frames + FBAT_SEG - 1) / FBAT_SEG;
    const bool mxn = sbat_keeps_max(A.norm);
    const FbatPart *p0 = part + sp.place * B;
    double m = -(double)__builtin_inff(), s[2] = {0, 0}, q[2] = {0, 0};
    if (mxn) {
        for (int j = lane; j < B; j += 64)
            for (long long g = 0; g < segs; g++) m = fmax(m, p0[g * B + j].a);
#pragma unroll
        for (int d = 32; d; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    } else {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int j = SBAT_CHUNK * ch + lane + 64 * h;
            if (j >= B) continue;
            for (long long g = 0; g < segs; g++) {
                const FbatPart v = p0[g * B + j];
                s[h] += v.a, q[h] += v.b;
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int j = SBAT_CHUNK * ch + lane + 64 * h;
        if (j >= B) continue;
        FbatStat r{m, 1.0};
        if (!mxn) {
            const double F = (double)sp.frames;
            const double mean = sp.frames ? s[h] / F : 0.0;
            r.a = mean;
            if (A.norm == OPUSGPU_FEAT_NORM_CMVN) {
                const double var = sp.frames ? q[h] / F - mean * mean : 0.0;
                r.d = sqrt(fmax(var, A.var_floor));
            }
        }
        stat[(long long)t * B + j] = r;
    }
}

// The normalisation of one float (a cell, a member of a pair, or the pad value) of bin j: fbat_norm's forms and REFMAX.
__device__ __forceinline__ float sbat_norm(const SbatArgs &A, float x, const FbatStat *__restrict__ st, const float2 *__restrict__ aff, int j) {
    switch (A.norm) {
        case OPUSGPU_FEAT_NORM_WHISPER: {
            const float lo = __fsub_rn((float)st[0].a, A.range);
            return __fmul_rn(__fadd_rn(fmaxf(x, lo), A.add), A.mul);
        }
        case OPUSGPU_STFT_NORM_REFMAX: {
            const float m = (float)st[0].a; // a float32 max, kept in a double: exact
            const float lo = __fsub_rn(m, A.range);
            return __fmul_rn(__fsub_rn(fmaxf(x, lo), m), A.mul);
        }
        case OPUSGPU_FEAT_NORM_CMN: return (float)((double)x - st[j].a);
        case OPUSGPU_FEAT_NORM_CMVN: {
            const FbatStat r = st[j];
            return (float)(((double)x - r.a) / r.d);
        }
        case OPUSGPU_FEAT_NORM_AFFINE: {
            const float2 r = aff[j];
            return __fmul_rn(__fsub_rn(x, r.x), r.y);
        }
        default: return x;
    }
}

// k_feat_batch's split of the work: blockIdx.y walks the tracks, blockIdx.x and the lanes the aligned 16-byte pieces of the tensor
// that a track's n = S * bins * c floats touch.  Float i of a track is row a = i / D, place b = i % D of a row of D floats: D = S * c
// bins-major (a the bin, b >> (c - 1) the frame), D = bins * c frames-major (a the frame, b >> (c - 1) the bin); b & (c - 1) is the
// member of a pair.  One 32-bit division a piece, the other three floats by carry.  A piece wholly inside the track goes out as one
// 16-byte store; the track's first and last piece, where they are shared with a neighbour or end the tensor, as guarded 4-byte stores
// of this track's floats alone, so every element is written once.  The source row (bins-major: plane * c floats, 256-byte aligned)
// is misaligned against the destination's in general: four coalesced 4-byte loads then, and one 16-byte load where the source
// piece is aligned, real and in one row.
__global__ void __launch_bounds__(256) k_stft_batch(const FbatSpan *__restrict__ spans, int n_tracks, const float *__restrict__ grid, SbatArgs A,
                                                    const FbatStat *__restrict__ stat, const float2 *__restrict__ aff,
                                                    float *__restrict__ out) {
    const u32 B = (u32)A.B, S = (u32)A.S, c = (u32)A.c, cs = c - 1, n = S * B * c; // S * B * c <= 0x7fffffff (stft_batch_run)
    const u32 D = (A.frames_major ? B : S) * c;
    for (int t = (int)blockIdx.y; t < n_tracks; t += (int)gridDim.y) {
        const FbatSpan sp = spans[t];
        const u32 F = (u32)sp.frames;
        const bool padn = A.pad_normalized && !(A.norm == OPUSGPU_STFT_NORM_REFMAX && F == 0); // no maximum: the value verbatim
        const FbatStat *st = stat + (long long)t * B;
        const float *src = grid + sp.grid_offset;
        const long long rowlen = A.frames_major ? (long long)D : sp.plane * c; // floats between two rows of the source
        const u32 real = A.frames_major ? D : F * c;                           // bins-major: the real floats of a row
        const long long e0 = (long long)t * n;                                 // the track's first element of the tensor
        const long long p0 = e0 >> 2, pieces = ((e0 + n - 1) >> 2) - p0 + 1;
        for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pieces; p += (long long)gridDim.x * 256) {
            const long long g = (p0 + p) << 2;
            const long long i0 = g - e0; // -3 .. n - 1
            const u32 first = i0 < 0 ? 0u : (u32)i0;
            u32 a = first / D, b = first - a * D;
            float v[4];
            const bool whole = i0 >= 0 && i0 + 4 <= (long long)n;
            // the source piece in one load: all four floats real, in one row, and the row's piece aligned
            bool wide = false;
            if (whole) {
                if (A.frames_major)
                    wide = (e0 & 3) == 0 && first + 3 < F * D; // source float = grid_offset + i: aligned with the destination
                else
                    wide = (b & 3) == 0 && b + 3 < real; // b + 3 < F * c <= D: one row
                if (wide) {
                    const float4 x = *reinterpret_cast<const float4 *>(src + (long long)a * rowlen + b);
                    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
                }
            }
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const long long i = i0 + h;
                if (i >= 0 && i < (long long)n) {
                    const u32 j = A.frames_major ? b >> cs : a;
                    const bool is_real = A.frames_major ? a < F : b < real;
                    float y;
                    if (is_real) {
                        const float x = wide ? v[h] : src[(long long)a * rowlen + b];
                        y = sbat_norm(A, x, st, aff, (int)j);
                    } else {
                        y = padn ? sbat_norm(A, A.pad_value, st, aff, (int)j) : A.pad_value;
                    }
                    v[h] = y;
                    if (++b == D) b = 0, a++;
                }
            }
            if (whole) {
                *reinterpret_cast<float4 *>(out + g) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (i0 + h >= 0 && i0 + h < (long long)n) out[g + h] = v[h];
            }
        }
    }
}

// The direct path's pad cells.  A track has `rows` pad runs of the tensor: bins-major one per bin, floats [(k S + F) c, (k + 1) S c)
// of the track; frames-major one, [F bins c, S bins c).  Work item q of a track is piece q % P of run q / P, P = the most aligned
// 16-byte pieces a run of its length touches; a piece wholly inside its run is one 16-byte store, the run's first and last piece
// guarded 4-byte stores of the run's own floats -- the floats in front of a run are real cells that k_tracks_stft wrote.  A track
// with F = S has no item.
__global__ void __launch_bounds__(256) k_stft_pad(const FbatSpan *__restrict__ spans, int n_tracks, SbatArgs A, float *__restrict__ out) {
    const u32 B = (u32)A.B, S = (u32)A.S, c = (u32)A.c, n = S * B * c;
    const float pad = A.pad_value;
    for (int t = (int)blockIdx.y; t < n_tracks; t += (int)gridDim.y) {
        const u32 F = (u32)spans[t].frames;
        if (F >= S) continue;
        const u32 rows = A.frames_major ? 1u : B;
        const u32 len = (S - F) * c * (A.frames_major ? B : 1u); // floats of a run, >= 1
        const u32 P = (len + 3) / 4 + 1;
        const u32 items = rows * P; // <= n / 4 + 2 bins
        const long long e0 = (long long)t * n;
        for (u32 q = blockIdx.x * 256 + threadIdx.x; q < items; q += gridDim.x * 256) {
            const u32 row = q / P, pi = q - row * P;
            const long long r1 = A.frames_major ? e0 + n : e0 + (long long)(row + 1) * S * c, r0 = r1 - len;
            const long long g = ((r0 >> 2) + pi) << 2;
            if (g >= r1) continue;
            if (g >= r0 && g + 4 <= r1) {
                *reinterpret_cast<float4 *>(out + g) = make_float4(pad, pad, pad, pad);
            } else {
#pragma unroll
                for (int h = 0; h < 4; h++)
                    if (g + h >= r0 && g + h < r1) out[g + h] = pad;
            }
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------
// What a request must be, wherever it comes from: -> nullptr, or what is wrong with it (feat_batch_req_wrong with this section's
// norms and widths).
static const char *stft_batch_req_wrong(const opusgpu_stft_batch_req *r, const float *sub, const float *mul_vec, int bins) {
    if (!r) return "stft batch: no request";
    if (r->norm < OPUSGPU_FEAT_NORM_NONE || r->norm > OPUSGPU_STFT_NORM_REFMAX) return "stft batch: an unknown norm";
    if (r->pad_mode != OPUSGPU_FEAT_PAD_VALUE && r->pad_mode != OPUSGPU_FEAT_PAD_NORMALIZED) return "stft batch: an unknown pad mode";
    if (!std::isfinite(r->pad_value) || !std::isfinite(r->range) || !std::isfinite(r->add) || !std::isfinite(r->mul) ||
        !std::isfinite(r->var_floor))
        return "stft batch: a field that is not finite";
    if (!(r->var_floor > 0)) return "stft batch: var_floor must be > 0";
    if (r->stride_frames < 1) return "stft batch: stride_frames must be >= 1";
    for (int32_t w : r->reserved)
        if (w) return "stft batch: a reserved word that is not 0";
    if (r->norm == OPUSGPU_FEAT_NORM_AFFINE) {
        if (!sub || !mul_vec || bins < 1 || bins > SBAT_MAX_BINS) return "stft batch: AFFINE needs sub and mul of 1 - 1025 entries";
        for (int j = 0; j < bins; j++)
            if (!std::isfinite(sub[j]) || !std::isfinite(mul_vec[j])) return "stft batch: an AFFINE entry that is not finite";
    }
    return nullptr;
}

// What ties a request to a grid of `bins` bins of c floats: -> nullptr, or the reason of the refusal.
static const char *stft_batch_shape_wrong(const opusgpu_stft_batch_req &r, int affine_bins, int bins, int c) {
    if (bins < 1 || bins > SBAT_MAX_BINS) return "stft batch: the bins must be 1 - 1025";
    if (c != 1 && c != 2) return "stft batch: c must be 1 (real cells) or 2 (pairs)";
    if (r.stride_frames > 0x7fffffffLL / (bins * c)) return "stft batch: stride_frames * bins * c is above 0x7fffffff";
    if (r.norm == OPUSGPU_FEAT_NORM_AFFINE && affine_bins != bins) return "stft batch: the AFFINE vectors do not have the spectrogram's bins";
    if (c == 2 && r.norm != OPUSGPU_FEAT_NORM_NONE && r.norm != OPUSGPU_FEAT_NORM_AFFINE)
        return "stft batch: pairs take the norms NONE and AFFINE only";
    return nullptr;
}
#define OG_STFT_STRIDE_SHORT "stft batch: stride_frames is below the frames of a track"

static SbatArgs stft_batch_args(const opusgpu_stft_batch_req &r, int bins, int c, int layout) {
    return SbatArgs{r.stride_frames, r.var_floor, bins, c, layout == OPUSGPU_MEL_FRAMES_MAJOR ? 1 : 0, r.norm,
                    r.pad_mode == OPUSGPU_FEAT_PAD_NORMALIZED ? 1 : 0, r.pad_value, r.range, r.add, r.mul};
}

// The stage over n tracks: checks, the tile table, the uploads, the launches on `s` and the wait; every device buffer of the call is
// freed on every way out.  sub / mul_vec: `bins` floats each for AFFINE.  why(reason) is told what a refusal was.
static int stft_batch_run(int device, hipStream_t s, int n_tracks, const opusgpu_stft_batch_span *spans, int bins, int c, int layout,
                          const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid, void *d_out,
                          const TrackFail &hip_failed, const std::function<void(const char *)> &why) {
    auto refuse = [&](const char *reason) {
        if (why) why(reason);
        return (int)OPUSGPU_BAD_ARG;
    };
    if (n_tracks < 0 || (n_tracks && !spans)) return refuse("stft batch: no spans");
    if (layout != OPUSGPU_MEL_BANDS_MAJOR && layout != OPUSGPU_MEL_FRAMES_MAJOR) return refuse("stft batch: an unknown layout");
    if (const char *bad = stft_batch_req_wrong(req, sub, mul_vec, bins)) return refuse(bad);
    if (const char *bad = stft_batch_shape_wrong(*req, bins, bins, c)) return refuse(bad);
    const int64_t S = req->stride_frames;
    const bool stats = req->norm == OPUSGPU_FEAT_NORM_WHISPER || req->norm == OPUSGPU_FEAT_NORM_CMN || req->norm == OPUSGPU_FEAT_NORM_CMVN ||
                       req->norm == OPUSGPU_STFT_NORM_REFMAX;
    const int chunks = (bins + SBAT_CHUNK - 1) / SBAT_CHUNK;
    if ((int64_t)n_tracks * chunks > 0x7fffffff) return refuse("stft batch: too many tracks");
    std::vector<FbatSpan> sp((size_t)n_tracks);
    std::vector<SbatTile> tiles;
    int64_t places = 0;
    bool any = false;
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_stft_batch_span &u = spans[t];
        if (u.grid_offset < 0 || u.grid_offset % 64 || u.plane < 0 || u.plane % 64 || u.frames < 0 || u.frames >= (1LL << 29) ||
            u.plane < u.frames || u.grid_offset > INT64_MAX / 8 || u.plane > (1LL << 40))
            return refuse("stft batch: a span that breaks a rule");
        if (u.frames > S) return refuse(OG_STFT_STRIDE_SHORT);
        const int64_t segs = (u.frames + FBAT_SEG - 1) / FBAT_SEG;
        if ((places + segs) * chunks > 0x7fffffff) return refuse("stft batch: too many segments");
        sp[(size_t)t] = FbatSpan{u.grid_offset, u.plane, u.frames, places};
        if (stats)
            for (int64_t g = 0; g < segs; g++)
                for (int ch = 0; ch < chunks; ch++) tiles.push_back(SbatTile{t, (i32)g, ch});
        places += segs;
        any |= u.frames > 0;
    }
    if (!n_tracks) return OPUSGPU_OK;
    if (!d_out || ((uintptr_t)d_out & 127) || (any && (!d_grid || ((uintptr_t)d_grid & 127)))) return refuse("stft batch: a buffer that is NULL or not 128-byte aligned");
    const SbatArgs A = stft_batch_args(*req, bins, c, layout);
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles, d_part, d_stat, d_aff;
    TRK_CHK(d_spans.upload(sp.data(), sp.size() * sizeof(FbatSpan)));
    if (stats) {
        TRK_CHK(d_part.alloc((size_t)std::max<int64_t>(places, 1) * bins * sizeof(FbatPart)));
        TRK_CHK(d_stat.alloc((size_t)n_tracks * bins * sizeof(FbatStat)));
        if (!tiles.empty()) {
            TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(SbatTile)));
            hipLaunchKernelGGL(k_stft_stats, dim3((unsigned)tiles.size()), dim3(256), 0, s, (const SbatTile *)d_tiles.p, (const FbatSpan *)d_spans.p,
                               (const float *)d_grid, A, (FbatPart *)d_part.p);
            TRK_CHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_stft_fold, dim3((unsigned)(n_tracks * chunks)), dim3(64), 0, s, (const FbatSpan *)d_spans.p, (const FbatPart *)d_part.p, A,
                           chunks, (FbatStat *)d_stat.p);
        TRK_CHK(hipGetLastError());
    } else if (req->norm == OPUSGPU_FEAT_NORM_AFFINE) {
        std::vector<float> pairs(2 * (size_t)bins);
        for (int j = 0; j < bins; j++) pairs[2 * (size_t)j] = sub[j], pairs[2 * (size_t)j + 1] = mul_vec[j];
        TRK_CHK(d_aff.upload(pairs.data(), pairs.size() * sizeof(float)));
    }
    // a workgroup per 16 KB of a track (4 pieces a lane), at most 1024 of them a track
    const int64_t pieces = S * bins * c / 4 + 2;
    const int64_t gx = std::min<int64_t>((pieces + 1023) / 1024, 1024);
    hipLaunchKernelGGL(k_stft_batch, dim3((unsigned)gx, (unsigned)std::min(n_tracks, 65535)), dim3(256), 0, s, (const FbatSpan *)d_spans.p, n_tracks,
                       (const float *)d_grid, A, (const FbatStat *)d_stat.p, (const float2 *)d_aff.p, (float *)d_out);
    TRK_CHK(hipGetLastError());
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// The direct path behind k_tracks_stft, which has written frames [0, frames[t]) of every track into the tensor at d_out: the pad
// cells.  The request is one that files_stft_run has checked (norm NONE, so a normalised pad value is the value).
static int stft_pad_run(int device, hipStream_t s, int n_tracks, const int64_t *frames, int bins, int c, int layout,
                        const opusgpu_stft_batch_req &req, void *d_out, const TrackFail &hip_failed) {
    if (n_tracks <= 0) return OPUSGPU_OK;
    const int64_t S = req.stride_frames;
    std::vector<FbatSpan> sp((size_t)n_tracks);
    bool any = false;
    for (int t = 0; t < n_tracks; t++) {
        if (frames[t] < 0 || frames[t] > S) return OPUSGPU_BAD_ARG;
        sp[(size_t)t] = FbatSpan{0, 0, frames[t], 0};
        any |= frames[t] < S;
    }
    if (!any) return OPUSGPU_OK;
    if (!d_out || ((uintptr_t)d_out & 127)) return OPUSGPU_BAD_ARG;
    const SbatArgs A = stft_batch_args(req, bins, c, layout);
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans;
    TRK_CHK(d_spans.upload(sp.data(), sp.size() * sizeof(FbatSpan)));
    const int64_t items = S * bins * c / 4 + 2 * (int64_t)bins; // the most work items of a track (k_stft_pad), 4 a lane
    const int64_t gx = std::min<int64_t>((items + 1023) / 1024, 1024);
    hipLaunchKernelGGL(k_stft_pad, dim3((unsigned)gx, (unsigned)std::min(n_tracks, 65535)), dim3(256), 0, s, (const FbatSpan *)d_spans.p, n_tracks, A,
                       (float *)d_out);
    TRK_CHK(hipGetLastError());
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// What a request must keep (opusgpu_set_stft_batch): -> the state a context holds, off for NULL or `enabled` 0.
static int stft_batch_set(StftBatchState &st, const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, int bins) {
    if (!req || !req->enabled) {
        st = StftBatchState{};
        return OPUSGPU_OK;
    }
    if (stft_batch_req_wrong(req, sub, mul_vec, bins)) return OPUSGPU_BAD_ARG;
    st.req = *req;
    st.sub.clear(), st.mul.clear();
    if (req->norm == OPUSGPU_FEAT_NORM_AFFINE) st.sub.assign(sub, sub + bins), st.mul.assign(mul_vec, mul_vec + bins);
    return OPUSGPU_OK;
}

extern "C" {

int64_t opusgpu_stft_batch_layout(int n, int bins, int c, int64_t stride_frames, int64_t *feat_offsets) {
    if (n < 0 || bins < 1 || bins > SBAT_MAX_BINS || (c != 1 && c != 2) || stride_frames < 1 || stride_frames > 0x7fffffffLL / (bins * c))
        return OPUSGPU_BAD_ARG;
    for (int t = 0; t < n; t++)
        if (feat_offsets) feat_offsets[t] = (int64_t)t * stride_frames * bins * c;
    return (int64_t)n * stride_frames * bins * c;
}

int opusgpu_set_stft_batch(opusgpu_ctx *ctx, const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, int bins) {
    return ctx ? stft_batch_set(ctx->sbatch, req, sub, mul_vec, bins) : OPUSGPU_BAD_ARG;
}

int opusgpu_ms_set_stft_batch(opusgpu_ms *ms, const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, int bins) {
    return ms ? stft_batch_set(ms->sbatch, req, sub, mul_vec, bins) : OPUSGPU_BAD_ARG;
}

int opusgpu_tracks_stft_batch_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_stft_batch_span *spans, int bins, int c, int layout,
                                     const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid,
                                     void *d_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return stft_batch_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, bins, c, layout, req, sub, mul_vec,
                          d_grid, d_out, track_fail(ctx), [ctx](const char *why) { snprintf(ctx->err, sizeof(ctx->err), "%s", why); });
}

} // extern "C"
