// og_feat_batch.hpp -- feature batches (include/opusgpu.h, FEATURE BATCHES): the packed feature grid of TRACK FEATURES, TRACK
// SPECTROGRAMS or TRACK KALDI FEATURES collated into one dense tensor of n * S * W floats, every track normalised by statistics of
// its own real cells and padded to S frames.  Included by og_api.hip behind og_tracks_fbank.hpp; files_feature_run
// (og_feat.hpp) calls feat_batch_run behind its feature kernel when the owner holds a request.  DESIGN.md section 13k.
#pragma once

// ---- kernels ------------------------------------------------------------------------------------------
// A streaming stage: the grid is read once for the statistics (norms that have any) and once for the tensor, the tensor is written
// once.  Three kernels, all plain vector loads and stores:
//   k_feat_stats  a workgroup of four waves per (track, segment of FBAT_SEG frames): per bin the segment's max (WHISPER) or its sum and
//                 sum of squares in double (CMN, CMVN), into the partial table at (place[t] + segment) * W + bin;
//   k_feat_fold   one wave per track: folds the track's segments in ascending order and leaves per bin what the cells need -- the
//                 track's max, or the mean and the divisor;
//   k_feat_batch  a lane owns an aligned 16-byte piece of the DESTINATION, fetches its four cells or pad values and stores it whole.
// The order of every sum is fixed by the track's own F, W and layout: a lane's cells in ascending frame order, the lanes by a
// butterfly (bands-major) or the four waves in ascending order through LDS (frames-major), the segments in ascending order.
constexpr int FBAT_SEG = OPUSGPU_FEAT_SEG;
static_assert(FBAT_SEG == 1024, "a bands-major segment is four 16-byte pieces a lane");
struct FbatSpan {
    long long grid_offset, plane, frames;
    long long place; // the track's first row of the partial table, in segments
};
struct FbatTile {
    i32 track, seg;
};
struct FbatPart { // per (segment, bin): WHISPER keeps the max in a
    double a, b;
};
struct FbatStat { // per (track, bin).  WHISPER: a = the track's max;  CMN: a = mean_j, d = 1;  CMVN: a = mean_j, d = sqrt(max(var_j, floor))
    double a, d;
};
struct FbatArgs {
    long long S;
    double var_floor;
    int W, frames_major, norm, pad_normalized;
    float pad_value, range, add, mul;
};
static_assert(sizeof(opusgpu_feat_batch_req) == 64 && sizeof(opusgpu_feat_span) == 24, "feature batch records");

__device__ __forceinline__ void fbat_take(bool whisper, float x, float &mx, double &s, double &q) {
    if (whisper) {
        mx = fmaxf(mx, x);
    } else {
        const double v = (double)x;
        s += v;
        q += v * v;
    }
}

// FBAT_COMBINE_LDS: the frames-major combine of four waves' (sum, sum of squares) over 128 bins, 8,192 bytes -- 19 workgroups a CU by
// LDS, far past the 8 that 8 waves per SIMD need.
constexpr int FBAT_COMBINE_LDS = 4 * 128 * 2 * 8;
__global__ void __launch_bounds__(256) k_feat_stats(const FbatTile *__restrict__ tiles, const FbatSpan *__restrict__ spans,
                                                    const float *__restrict__ grid, FbatArgs A, FbatPart *__restrict__ part) {
    __shared__ double red[4][128][2];
    static_assert(sizeof(red) == FBAT_COMBINE_LDS, "the combine's LDS");
    const FbatTile tile = tiles[blockIdx.x];
    const FbatSpan sp = spans[tile.track];
    const int W = A.W, lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const bool whisper = A.norm == OPUSGPU_FEAT_NORM_WHISPER;
    const long long f0 = (long long)tile.seg * FBAT_SEG;
    const int nf = (int)(sp.frames - f0 < FBAT_SEG ? sp.frames - f0 : FBAT_SEG); // this segment's real frames, >= 1
    FbatPart *out = part + (sp.place + tile.seg) * W;
    const float NEG = -__builtin_inff();
    if (!A.frames_major) {
        // a wave per band: the row's segment begins at a multiple of 1024 floats from a 256-byte aligned row
        for (int j = wave; j < W; j += 4) {
            const float *row = grid + sp.grid_offset + (long long)j * sp.plane + f0;
            float mx = NEG;
            double s = 0, q = 0;
#pragma unroll
            for (int k = 0; k < FBAT_SEG / 256; k++) {
                const int f = 4 * (lane + 64 * k);
                if (f < nf) { // the piece lies inside the plane: plane is a multiple of 64 and >= F
                    const float4 v = *reinterpret_cast<const float4 *>(row + f);
                    fbat_take(whisper, v.x, mx, s, q);
                    if (f + 1 < nf) fbat_take(whisper, v.y, mx, s, q);
                    if (f + 2 < nf) fbat_take(whisper, v.z, mx, s, q);
                    if (f + 3 < nf) fbat_take(whisper, v.w, mx, s, q);
                }
            }
#pragma unroll
            for (int d = 32; d; d >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, d, 64));
                s += __shfl_xor(s, d, 64);
                q += __shfl_xor(q, d, 64);
            }
            if (lane == 0) out[j] = whisper ? FbatPart{(double)mx, 0.0} : FbatPart{s, q};
        }
    } else {
        // lane <-> bin (two bins a lane for W > 64), a wave every fourth frame
        const bool two = lane + 64 < W;
        float mx = NEG;
        double s0 = 0, q0 = 0, s1 = 0, q1 = 0;
        if (lane < W) {
            const float *cell = grid + sp.grid_offset + f0 * W + lane;
            for (int f = wave; f < nf; f += 4) {
                fbat_take(whisper, cell[(long long)f * W], mx, s0, q0);
                if (two) fbat_take(whisper, cell[(long long)f * W + 64], mx, s1, q1);
            }
        }
        // (a max is the same in any order: it goes through the sums' slots as a double)
        red[wave][lane][0] = whisper ? (double)mx : s0, red[wave][lane][1] = q0;
        red[wave][lane + 64][0] = whisper ? (double)NEG : s1, red[wave][lane + 64][1] = q1;
        __syncthreads();
        const int j = (int)threadIdx.x;
        if (j < W) {
            if (whisper) {
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

// One wave per track, lane <-> bin (two for W > 64): the segments in ascending order.
__global__ void __launch_bounds__(64) k_feat_fold(const FbatSpan *__restrict__ spans, const FbatPart *__restrict__ part, FbatArgs A,
                                                  FbatStat *__restrict__ stat) {
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x, W = A.W;
    const FbatSpan sp = spans[t];
    const long long segs = (sp.frames + FBAT_SEG - 1) / FBAT_SEG;
    const bool whisper = A.norm == OPUSGPU_FEAT_NORM_WHISPER;
    double m = -(double)__builtin_inff(), s[2] = {0, 0}, q[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int j = lane + 64 * h;
        if (j >= W) continue;
        const FbatPart *p = part + sp.place * W + j;
        for (long long g = 0; g < segs; g++) {
            const FbatPart v = p[g * W];
            if (whisper)
                m = fmax(m, v.a);
            else
                s[h] += v.a, q[h] += v.b;
        }
    }
    if (whisper) {
#pragma unroll
        for (int d = 32; d; d >>= 1) m = fmax(m, __shfl_xor(m, d, 64));
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int j = lane + 64 * h;
        if (j >= W) continue;
        FbatStat r{m, 1.0};
        if (!whisper) {
            const double F = (double)sp.frames;
            const double mean = sp.frames ? s[h] / F : 0.0;
            r.a = mean;
            if (A.norm == OPUSGPU_FEAT_NORM_CMVN) {
                const double var = sp.frames ? q[h] / F - mean * mean : 0.0;
                r.d = sqrt(fmax(var, A.var_floor));
            }
        }
        stat[(long long)t * W + j] = r;
    }
}

// The normalisation of one cell (or of the pad value) of bin j.  `st` is the track's row of k_feat_fold's table (not read by NONE
// and AFFINE), `aff` the (sub, mul) pairs of AFFINE.
__device__ __forceinline__ float fbat_norm(const FbatArgs &A, float x, const FbatStat *__restrict__ st, const float2 *__restrict__ aff, int j) {
    switch (A.norm) {
        case OPUSGPU_FEAT_NORM_WHISPER: {
            const float lo = __fsub_rn((float)st[0].a, A.range);
            return __fmul_rn(__fadd_rn(fmaxf(x, lo), A.add), A.mul);
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

// blockIdx.y walks the tracks, blockIdx.x and the lanes the aligned 16-byte pieces of the tensor that a track's S * W floats touch, as
// k_tracks_fill_tail splits its work.  Element i of a track is (j, f) = (i / S, i % S) bands-major and (f, j) = (i / W, i % W)
// frames-major: one 32-bit division a piece, the other three elements by carry.  A piece that lies wholly inside the track goes out
// as one 16-byte store; the track's first and last piece, where they are shared with a neighbour or end the tensor, as guarded
// 4-byte stores of this track's elements alone, so every element is written once.  Source and destination rows are misaligned
// against each other in general: the four cells are then four coalesced 4-byte loads, and one 16-byte load where the source piece
// is aligned and real.
__global__ void __launch_bounds__(256) k_feat_batch(const FbatSpan *__restrict__ spans, int n_tracks, const float *__restrict__ grid, FbatArgs A,
                                                    const FbatStat *__restrict__ stat, const float2 *__restrict__ aff,
                                                    float *__restrict__ out) {
    const u32 W = (u32)A.W, S = (u32)A.S, n = S * W; // S * W <= 0x7fffffff (feat_batch_run)
    const u32 D = A.frames_major ? W : S;
    for (int t = (int)blockIdx.y; t < n_tracks; t += (int)gridDim.y) {
        const FbatSpan sp = spans[t];
        const u32 F = (u32)sp.frames;
        const FbatStat *st = stat + (long long)t * W;
        const float *src = grid + sp.grid_offset;
        const long long e0 = (long long)t * n;                                  // the track's first element of the tensor
        const long long p0 = e0 >> 2, pieces = ((e0 + n - 1) >> 2) - p0 + 1;
        for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pieces; p += (long long)gridDim.x * 256) {
            const long long g = (p0 + p) << 2;
            const long long i0 = g - e0; // -3 .. n - 1
            const u32 first = i0 < 0 ? 0u : (u32)i0;
            u32 a = first / D, b = first - a * D;
            float v[4];
            const bool whole = i0 >= 0 && i0 + 4 <= (long long)n;
            // the source piece in one load: all four cells real, in one row, and the row's piece aligned
            bool wide = false;
            if (whole) {
                if (A.frames_major) {
                    wide = (e0 & 3) == 0 && first + 3 < F * W; // source element = grid_offset + i: aligned with the destination
                    if (wide) {
                        const float4 x = *reinterpret_cast<const float4 *>(src + first);
                        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
                    }
                } else {
                    wide = (b & 3) == 0 && b + 3 < F; // b + 3 < F <= S: one row
                    if (wide) {
                        const float4 x = *reinterpret_cast<const float4 *>(src + (long long)a * sp.plane + b);
                        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < 4; h++) {
                const long long i = i0 + h;
                if (i >= 0 && i < (long long)n) {
                    const u32 j = A.frames_major ? b : a, f = A.frames_major ? a : b;
                    float y;
                    if (f < F) {
                        const float x = wide ? v[h] : A.frames_major ? src[(long long)f * W + j] : src[(long long)j * sp.plane + f];
                        y = fbat_norm(A, x, st, aff, (int)j);
                    } else {
                        y = A.pad_normalized ? fbat_norm(A, A.pad_value, st, aff, (int)j) : A.pad_value;
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

// ---- host side ----------------------------------------------------------------------------------------
// What a request must be, wherever it comes from: -> nullptr, or what is wrong with it.
static const char *feat_batch_req_wrong(const opusgpu_feat_batch_req *r, const float *sub, const float *mul_vec, int width) {
    if (!r) return "feature batch: no request";
    if (r->norm < OPUSGPU_FEAT_NORM_NONE || r->norm > OPUSGPU_FEAT_NORM_AFFINE) return "feature batch: an unknown norm";
    if (r->pad_mode != OPUSGPU_FEAT_PAD_VALUE && r->pad_mode != OPUSGPU_FEAT_PAD_NORMALIZED) return "feature batch: an unknown pad mode";
    if (!std::isfinite(r->pad_value) || !std::isfinite(r->range) || !std::isfinite(r->add) || !std::isfinite(r->mul) ||
        !std::isfinite(r->var_floor))
        return "feature batch: a field that is not finite";
    if (!(r->var_floor > 0)) return "feature batch: var_floor must be > 0";
    if (r->stride_frames < 1) return "feature batch: stride_frames must be >= 1";
    for (int32_t w : r->reserved)
        if (w) return "feature batch: a reserved word that is not 0";
    if (r->norm == OPUSGPU_FEAT_NORM_AFFINE) {
        if (!sub || !mul_vec || width < 1 || width > 128) return "feature batch: AFFINE needs sub and mul of 1 - 128 entries";
        for (int j = 0; j < width; j++)
            if (!std::isfinite(sub[j]) || !std::isfinite(mul_vec[j])) return "feature batch: an AFFINE entry that is not finite";
    }
    return nullptr;
}

// What ties a request to a grid of width W: -> nullptr, or the reason of the refusal.
static const char *feat_batch_shape_wrong(const opusgpu_feat_batch_req &r, int affine_width, int W) {
    if (W < 1 || W > 128) return "feature batch: the feature width must be 1 - 128";
    if (r.stride_frames > 0x7fffffffLL / W) return "feature batch: stride_frames * width is above 0x7fffffff";
    if (r.norm == OPUSGPU_FEAT_NORM_AFFINE && affine_width != W) return "feature batch: the AFFINE vectors do not have the features' width";
    return nullptr;
}
#define OG_FEAT_STRIDE_SHORT "feature batch: stride_frames is below the frames of a track"

// The stage over n tracks: checks, the segment table, the uploads, the launches on `s` and the wait; every device buffer of the
// call is freed on every way out.  sub / mul_vec: W floats each for AFFINE.  why(reason) is told what a refusal was.
static int feat_batch_run(int device, hipStream_t s, int n_tracks, const opusgpu_feat_span *spans, int W, int layout,
                          const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid, void *d_out,
                          const TrackFail &hip_failed, const std::function<void(const char *)> &why) {
    auto refuse = [&](const char *reason) {
        if (why) why(reason);
        return (int)OPUSGPU_BAD_ARG;
    };
    if (n_tracks < 0 || (n_tracks && !spans)) return refuse("feature batch: no spans");
    if (layout != OPUSGPU_MEL_BANDS_MAJOR && layout != OPUSGPU_MEL_FRAMES_MAJOR) return refuse("feature batch: an unknown layout");
    if (const char *bad = feat_batch_req_wrong(req, sub, mul_vec, W)) return refuse(bad);
    if (const char *bad = feat_batch_shape_wrong(*req, W, W)) return refuse(bad);
    const int64_t S = req->stride_frames;
    const bool stats = req->norm == OPUSGPU_FEAT_NORM_WHISPER || req->norm == OPUSGPU_FEAT_NORM_CMN || req->norm == OPUSGPU_FEAT_NORM_CMVN;
    std::vector<FbatSpan> sp((size_t)n_tracks);
    std::vector<FbatTile> tiles;
    int64_t places = 0;
    bool any = false;
    for (int t = 0; t < n_tracks; t++) {
        const opusgpu_feat_span &u = spans[t];
        if (u.grid_offset < 0 || u.grid_offset % 64 || u.plane < 0 || u.plane % 64 || u.frames < 0 || u.frames >= (1LL << 29) ||
            u.plane < u.frames || u.grid_offset > INT64_MAX / 8 || u.plane > INT64_MAX / 1024)
            return refuse("feature batch: a span that breaks a rule");
        if (u.frames > S) return refuse(OG_FEAT_STRIDE_SHORT);
        const int64_t segs = (u.frames + FBAT_SEG - 1) / FBAT_SEG;
        if (places + segs > 0x7fffffff) return refuse("feature batch: too many segments");
        sp[(size_t)t] = FbatSpan{u.grid_offset, u.plane, u.frames, places};
        if (stats)
            for (int64_t g = 0; g < segs; g++) tiles.push_back(FbatTile{t, (i32)g});
        places += segs;
        any |= u.frames > 0;
    }
    if (!n_tracks) return OPUSGPU_OK;
    if (!d_out || ((uintptr_t)d_out & 127) || (any && (!d_grid || ((uintptr_t)d_grid & 127)))) return refuse("feature batch: a buffer that is NULL or not 128-byte aligned");
    FbatArgs A{S, req->var_floor, W, layout == OPUSGPU_MEL_FRAMES_MAJOR ? 1 : 0, req->norm, req->pad_mode == OPUSGPU_FEAT_PAD_NORMALIZED ? 1 : 0,
             req->pad_value, req->range, req->add, req->mul};
    TRK_CHK(hipSetDevice(device));
    RsDevBuf d_spans, d_tiles, d_part, d_stat, d_aff;
    TRK_CHK(d_spans.upload(sp.data(), sp.size() * sizeof(FbatSpan)));
    if (stats) {
        TRK_CHK(d_part.alloc((size_t)std::max<int64_t>(places, 1) * W * sizeof(FbatPart)));
        TRK_CHK(d_stat.alloc((size_t)n_tracks * W * sizeof(FbatStat)));
        if (!tiles.empty()) {
            TRK_CHK(d_tiles.upload(tiles.data(), tiles.size() * sizeof(FbatTile)));
            hipLaunchKernelGGL(k_feat_stats, dim3((unsigned)tiles.size()), dim3(256), 0, s, (const FbatTile *)d_tiles.p, (const FbatSpan *)d_spans.p,
                               (const float *)d_grid, A, (FbatPart *)d_part.p);
            TRK_CHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_feat_fold, dim3((unsigned)n_tracks), dim3(64), 0, s, (const FbatSpan *)d_spans.p, (const FbatPart *)d_part.p, A,
                           (FbatStat *)d_stat.p);
        TRK_CHK(hipGetLastError());
    } else if (req->norm == OPUSGPU_FEAT_NORM_AFFINE) {
        std::vector<float> pairs(2 * (size_t)W);
        for (int j = 0; j < W; j++) pairs[2 * (size_t)j] = sub[j], pairs[2 * (size_t)j + 1] = mul_vec[j];
        TRK_CHK(d_aff.upload(pairs.data(), pairs.size() * sizeof(float)));
    }
    // a workgroup per 16 KB of a track (4 pieces a lane), at most 1024 of them a track
    const int64_t pieces = S * W / 4 + 2;
    const int64_t gx = std::min<int64_t>((pieces + 1023) / 1024, 1024);
    hipLaunchKernelGGL(k_feat_batch, dim3((unsigned)gx, (unsigned)std::min(n_tracks, 65535)), dim3(256), 0, s, (const FbatSpan *)d_spans.p, n_tracks,
                       (const float *)d_grid, A, (const FbatStat *)d_stat.p, (const float2 *)d_aff.p, (float *)d_out);
    TRK_CHK(hipGetLastError());
    TRK_CHK(hipStreamSynchronize(s));
    return OPUSGPU_OK;
}

// What a request must keep (opusgpu_set_feature_batch): -> the state a context holds, off for NULL or `enabled` 0.
static int feat_batch_set(FeatBatchState &st, const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, int width) {
    if (!req || !req->enabled) {
        st = FeatBatchState{};
        return OPUSGPU_OK;
    }
    if (feat_batch_req_wrong(req, sub, mul_vec, width)) return OPUSGPU_BAD_ARG;
    st.req = *req;
    st.sub.clear(), st.mul.clear();
    if (req->norm == OPUSGPU_FEAT_NORM_AFFINE) st.sub.assign(sub, sub + width), st.mul.assign(mul_vec, mul_vec + width);
    return OPUSGPU_OK;
}

extern "C" {

int64_t opusgpu_feat_batch_layout(int n, int width, int64_t stride_frames, int64_t *feat_offsets) {
    if (n < 0 || width < 1 || width > 128 || stride_frames < 1 || stride_frames > 0x7fffffffLL / width) return OPUSGPU_BAD_ARG;
    for (int t = 0; t < n; t++)
        if (feat_offsets) feat_offsets[t] = (int64_t)t * stride_frames * width;
    return (int64_t)n * stride_frames * width;
}

int opusgpu_set_feature_batch(opusgpu_ctx *ctx, const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, int width) {
    return ctx ? feat_batch_set(ctx->fbatch, req, sub, mul_vec, width) : OPUSGPU_BAD_ARG;
}

int opusgpu_ms_set_feature_batch(opusgpu_ms *ms, const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, int width) {
    return ms ? feat_batch_set(ms->fbatch, req, sub, mul_vec, width) : OPUSGPU_BAD_ARG;
}

int opusgpu_tracks_feature_batch_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_feat_span *spans, int width, int layout,
                                        const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid,
                                        void *d_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return feat_batch_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, width, layout, req, sub, mul_vec,
                          d_grid, d_out, track_fail(ctx), [ctx](const char *why) { snprintf(ctx->err, sizeof(ctx->err), "%s", why); });
}

} // extern "C"
