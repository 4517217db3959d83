// og_tracks_fbank.hpp -- Kaldi's fbank and MFCC features of the mono track at any rate (include/opusgpu.h, TRACK KALDI FEATURES): the
// tables per parameter set, the kernel that turns packed int16 mono tracks into float32 feature tracks, its host side, and the
// whole-file call that ends in it.  Included at the end of og_api.hip behind og_feat.hpp, whose window stage, tile and span
// records, run function, filterbank packer, record rules and whole-file flow it shares, and in front of
// og_ms_tracks.hpp, which holds the multistream twin of the whole-file call.
#pragma once

// ---- kernel -------------------------------------------------------------------------------------------
// k_tracks_fbank: k_tracks_melspec's shape -- one workgroup per entry of a tile table, a tile T = 128, 64 or 32 consecutive frames of
// one track, 32 per wave, the window in LDS cut by phase, both products on v_mfma_f32_32x32x2_f32 -- with Kaldi's computation:
//   1. STAGE (og_feat.hpp: feat_stage_window).  The tile's window is W = (T - 1) H + L samples and starts at the first frame's s:
//      H * first with snip_edges, H * first + H / 2 - L / 2 without.  The track comes through aligned 16-byte loads of the buffer, nothing read behind the piece that
//      holds its last sample.  Without snip_edges the places in front of the track and behind it are filled by Kaldi's reflection
//      repeated until it lies inside (q mod 2n, mirrored in the upper half), from LDS where the source is in the window, else from
//      the track.  With snip_edges no frame that exists reads such a place; they are zeroed for the frames of a working wave that
//      do not exist, which are computed and not stored.
//   2. MEAN.  With remove_dc every lane sums half of its frame's L samples in int32 (L * 32768 < 2^31) and takes the other half from
//      the lane 32 away.  The sum stays an integer: a sample's d is (float)(L x - sum), and 1 / L goes into the scale, so a constant
//      track has d = 0 exactly.  Without remove_dc the sum is 0 and L is 1 in that formula.
//   3. OPERAND, DFT.  The spectrum is turned by e^{i pi k (L - 1) / N}, which changes no magnitude and makes the basis symmetric about
//      the frame's centre: with u_i = t_i + t_{L-1-i}, v_i = t_i - t_{L-1-i}, Re = sum_i u_i w[i] cos(th), Im = sum_i v_i w[i] sin(th),
//      th = 2 pi k (i - (L - 1) / 2) / N, over the half = ceil(L / 2) taps i < half; the middle tap of an odd L has its cosine halved
//      (u = 2 t there) and no sine.  The window is in the basis (w[i] = w[L - 1 - i]); the operand is (e_i +- e_{L-1-i}) * scale / L.
//      The half wave kh = 0 walks taps 0 .. KSr - 1 upwards, kh = 1 taps KSr .. half - 1, KSr = ceil(half / 2): consecutive taps, so
//      that the pre-emphasis' predecessor d_{i-1} is the lane's last step's sample (and, for the mirror tap walking downwards, the
//      sample it reads is the next step's own): two LDS reads a k-step, no second copy of the frame.  Steps behind a half wave's
//      last tap (the table is padded to groups of 4 k-steps) multiply zeros of the basis and read nothing.
//   4. POWER, MEL.  As k_tracks_melspec, over N / 2 bins (no Nyquist bin): only the blocks of 32 bins some band weights are walked.
//   5. FLOOR, LOG, MFCC.  max(mel, floor) and logf in the accumulators.  For MFCC they ARE the B operand of a third product, c[q][f] +=
//      (lift D)[q][j] g[j][f], with the lifted DCT packed like a filterbank whose "bins" are the bands: fused, in registers, no LDS.
//   6. STORE.  k_tracks_melspec's, with the feature width (n_ceps, else n_mels): a copy, as is step 4 (og_feat.hpp says why).
// No float atomics, no sum whose order depends on the launch: the same input gives the same bits.
struct FbArgs {
    i32 L, H, n_mels, n_ceps;
    i32 n_blocks;                   // kept blocks of 32 bins
    i32 half, ksr, ks4;             // taps of the folded frame, those of half wave 0, k-steps of a block in the table (a multiple of 4)
    i32 dct_off;                    // where the packed lifted DCT begins in `fb`, in floats
    i32 power, log, snip, remove_dc, frames_major;
    float floor, preemph;
    u8 mask[MS_MAXBLK + 3];         // bit mm of mask[b]: band block mm has a weight in kept bin block b
};

__global__ void __launch_bounds__(256) k_tracks_fbank(const MelTile *__restrict__ tiles, const MelSpan *__restrict__ spans,
                                                      const i16 *__restrict__ in, const float2 *__restrict__ basis,
                                                      const float *__restrict__ fb, FbArgs a, float *__restrict__ out) {
    extern __shared__ __align__(16) i16 lds[]; // the window by phase, W places (feat_window_lds_bytes); afterwards a store area of [32][MEL_STG] floats per wave
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int T = nthr >> 1, L = a.L, H = a.H;
    const MelTile tl = tiles[blockIdx.x];
    const MelSpan sp = spans[tl.track];
    const long long n = sp.in_samples;
    const long long F = a.snip ? (n < L ? 0 : 1 + (n - L) / H) : (n + H / 2) / H;
    const long long left = F - tl.first;
    const int nf = left < T ? (int)left : T; // frames of this tile that exist
    if (nf <= 0) return;
    const int waves_on = (nf + 31) >> 5;                       // waves that have a frame
    const int W = (T - 1) * H + L;                             // the tile's window, which fixes the places
    const int Wuse = (32 * waves_on - 1) * H + L;              // what the working waves read of it
    const FeatPhase ph(W, H);

    // 1. the window -> LDS: its first sample, counted from the track's, is the first frame's
    feat_stage_window(lds, ph, in + sp.in_offset, n, (long long)H * tl.first + (a.snip ? 0 : H / 2 - L / 2), Wuse, tid, nthr,
                      FeatEdgeKaldi{a.snip});

    // 2. to 5. 32 frames per wave
    const int fl = lane & 31, kh = lane >> 5;
    og_f32x16 mel[4];
#pragma unroll
    for (int mm = 0; mm < 4; mm++)
#pragma unroll
        for (int r = 0; r < 16; r++) mel[mm][r] = 0.f;
    if (wave < waves_on) {
        if (a.n_blocks > 0) { // (no kept block: no band has a weight, and mel stays 0)
            const int f = wave * 32 + fl; // the lane's frame in the tile
            int Lm = 1, sum = 0;
            if (a.remove_dc) {
                Lm = L;
                const int i0 = kh ? L >> 1 : 0, i1 = kh ? L : L >> 1;
                int row = i0 % H, col = i0 / H + f;
                for (int i = i0; i < i1; i++) {
                    sum += lds[ph.at(row, col)];
                    if (++row >= H) row = 0, col++;
                }
                sum += __shfl_xor(sum, 32);
            }
            const float sl = sp.scale / (float)Lm, c = a.preemph;
            auto dval = [=](int x) { return (float)(__mul24(x, Lm) - sum); };
            // the lane's walk: upwards from tap i0, downwards from tap L - 1 - i0, whose predecessor L - 2 - i0 is the first it reads
            const int i0 = kh * a.ksr, lim = kh ? a.half - a.ksr : a.ksr; // (half - ksr <= ksr)
            const int ip = i0 ? i0 - 1 : 0, jc = L - 1 - i0, jn = jc - 1;  // tap 0 is its own predecessor
            const float dpu0 = dval(lds[ph.at(ip % H, ip / H + f)]), dcd0 = dval(lds[ph.at(jc % H, jc / H + f)]);
            const int pa0 = i0 % H, ca0 = i0 / H + f;
            const int pb0 = jn < 0 ? H - 1 : jn % H, cb0 = (jn < 0 ? -1 : jn / H) + f; // (jn = -1 for L = 2 alone, where it is never read)
            // the basis comes a k-step at a time, 512 bytes per wave: requested two groups of 4 k-steps ahead of its use, as in
            // k_tracks_melspec (the table is one run over all kept blocks)
            const int G = a.ks4 >> 2, GT = a.n_blocks * G;
            const float2 *const bp = basis + lane;
            float2 w0[4], w1[4], w2[4];
#pragma unroll
            for (int j = 0; j < 4; j++) w0[j] = bp[(size_t)j * 64], w1[j] = bp[(size_t)(4 * (GT > 1 ? 1 : 0) + j) * 64];
            int gg = 0;
            for (int b = 0; b < a.n_blocks; b++) {
                og_f32x16 re, im;
#pragma unroll
                for (int r = 0; r < 16; r++) re[r] = 0.f, im[r] = 0.f;
                int pa = pa0, ca = ca0, pb = pb0, cb = cb0, ks = 0;
                float dpu = dpu0, dcd = dcd0;
                for (int g = 0; g < G; g++, gg++) {
                    const int ahead = gg + 2 < GT ? gg + 2 : GT - 1;
#pragma unroll
                    for (int j = 0; j < 4; j++) w2[j] = bp[(size_t)(4 * ahead + j) * 64];
#pragma unroll
                    for (int j = 0; j < 4; j++, ks++) {
                        int xu = 0, xd = 0;
                        if (ks < lim) xu = lds[ph.at(pa, ca)], xd = lds[ph.at(pb, cb)];
                        if (++pa >= H) pa = 0, ca++;
                        if (--pb < 0) pb = H - 1, cb--;
                        const float du = dval(xu), dd = dval(xd);
                        const float ea = fmaf(-c, dpu, du), eb = fmaf(-c, dd, dcd);
                        dpu = du, dcd = dd;
                        re = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[j].x, __fmul_rn(ea + eb, sl), re, 0, 0, 0);
                        im = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[j].y, __fmul_rn(ea - eb, sl), im, 0, 0, 0);
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
        // 5. floor and log where they are: register r of the lane is band 8 (r >> 2) + 4 kh + (r & 3) of the block, frame fl
#pragma unroll
        for (int mm = 0; mm < 4; mm++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float v = fmaxf(mel[mm][r], a.floor);
                mel[mm][r] = a.log ? logf(v) : v;
            }
        if (a.n_ceps > 0) { // bands behind n_mels hold logf(floor), finite, against zeros of the table
            og_f32x16 cep[4];
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
#pragma unroll
                for (int r = 0; r < 16; r++) cep[qq][r] = 0.f;
                if (32 * qq < a.n_ceps) {
#pragma unroll
                    for (int mm = 0; mm < 4; mm++) {
                        if (32 * mm < a.n_mels) {
                            const float *const fp = fb + a.dct_off + (size_t)((mm * 4 + qq) * 16) * 64 + lane;
#pragma unroll
                            for (int r = 0; r < 16; r++)
                                cep[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(fp[r * 64], mel[mm][r], cep[qq], 0, 0, 0);
                        }
                    }
                }
            }
#pragma unroll
            for (int qq = 0; qq < 4; qq++) mel[qq] = cep[qq];
        }
    }
    __syncthreads(); // every wave has read its last sample

    // 6. out, 32 features at a time
    float *const stg = reinterpret_cast<float *>(lds) + wave * 32 * MEL_STG;
    const int wf = nf - wave * 32 < 32 ? nf - wave * 32 : 32; // frames of this wave that exist (may be <= 0)
    float *const dst = out + sp.out_offset;
    const long long f0 = (long long)tl.first + wave * 32;
    const int width = a.n_ceps > 0 ? a.n_ceps : a.n_mels, frames_major = a.frames_major;
    const bool whole4 = (width & 3) == 0;
#pragma unroll
    for (int mm = 0; mm < 4; mm++) {
        if (32 * mm < width) { // the same for every wave: the barriers inside are reached by all
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int band = 8 * (r >> 2) + 4 * kh + (r & 3);
                stg[frames_major ? fl * MEL_STG + band : band * MEL_STG + fl] = mel[mm][r];
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < 4; it++) { // 32 rows of 8 pieces
                const int row = (lane + 64 * it) >> 3, pc = lane & 7;
                const og_f32x4 v = *reinterpret_cast<const og_f32x4 *>(stg + row * MEL_STG + 4 * pc);
                if (frames_major) { // row: frame, piece: features 32 mm + 4 pc .. + 3
                    const int j0 = 32 * mm + 4 * pc;
                    if (row < wf && j0 < width) {
                        float *const d = dst + (f0 + row) * width + j0;
                        if (whole4) {
                            *reinterpret_cast<og_f32x4 *>(d) = v;
                        } else {
#pragma unroll
                            for (int h = 0; h < 4; h++)
                                if (j0 + h < width) d[h] = v[h];
                        }
                    }
                } else {            // row: feature, piece: frames f0 + 4 pc .. + 3
                    if (32 * mm + row < width && 4 * pc < wf) {
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
// TRACK KALDI FEATURES, TABLES: made in double at first use, rounded once, kept per distinct set of the fields that reach them for
// the life of the process: the tables as the accessors hand them out, and what the kernel's lanes load in their order.
struct FbankTables {
    int L = 0, N = 0, bins = 0, n_mels = 0, n_ceps = 0, half = 0, ksr = 0, ks4 = 0;
    std::vector<float> w;           // [L]
    std::vector<float> bank;        // [n_mels][bins]
    std::vector<float> dct;         // [n_ceps][n_mels], lifted
    std::vector<int> blocks;        // the blocks of 32 bins in which the bank has a non-zero entry
    std::vector<float> basis;       // [kept block][ks4][64 lanes][cos, sin]: tap (lane >> 5) * ksr + ks, bin 32 nb + (lane & 31)
    std::vector<float> fb;          // feat_pack_fb of the bank, then (at dct_off) of the lifted DCT over the blocks of 32 bands
    size_t dct_off = 0;
    u8 mask[MS_MAXBLK + 3] = {};
};
typedef std::tuple<int, int, int, int, int, int, float, double, float> FbankKey; // sample_rate, L, N, n_mels, n_ceps, window, low, high, lifter

static int fbank_n_fft(const opusgpu_fbank_params &p) {
    if (p.n_fft) return p.n_fft;
    int N = 64;
    while (N < p.frame_length) N <<= 1;
    return N;
}
static int fbank_width(const opusgpu_fbank_params &p) { return p.n_ceps > 0 ? p.n_ceps : p.n_mels; }
static double fbank_high(const opusgpu_fbank_params &p) {
    return p.high_freq > 0.f ? (double)p.high_freq : p.sample_rate / 2.0 + (double)p.high_freq;
}

static bool fbank_params_ok(const opusgpu_fbank_params *p) {
    if (!p) return false;
    if (p->sample_rate < 1 || p->sample_rate > 1048576) return false;
    if (p->frame_length < 2 || p->frame_length > 2048) return false;
    if (p->frame_shift < 1 || 31LL * p->frame_shift + p->frame_length > MS_MAXW) return false;
    if (p->n_fft && (p->n_fft < 64 || p->n_fft > 2048 || p->n_fft % 16 || p->n_fft < p->frame_length)) return false;
    if (p->n_mels < 3 || p->n_mels > 128 || p->n_ceps < 0 || p->n_ceps > p->n_mels) return false;
    if (p->window < OPUSGPU_FBANK_POVEY || p->window > OPUSGPU_FBANK_BLACKMAN) return false;
    if (p->snip_edges > 1 || p->remove_dc > 1 || (p->power != 1 && p->power != 2)) return false;
    if (p->log != OPUSGPU_FBANK_LOG_NONE && p->log != OPUSGPU_FBANK_LOG_LN) return false;
    if (p->n_ceps && p->log != OPUSGPU_FBANK_LOG_LN) return false;
    if (p->layout != OPUSGPU_MEL_BANDS_MAJOR && p->layout != OPUSGPU_MEL_FRAMES_MAJOR) return false;
    if (!(p->preemphasis >= 0.f) || !(p->preemphasis <= 1.f)) return false;
    const double high = fbank_high(*p);
    if (!(p->low_freq >= 0.f) || !((double)p->low_freq < high) || !(high <= p->sample_rate / 2.0)) return false;
    if (!std::isfinite(p->floor) || p->floor < 0.f || (p->log != OPUSGPU_FBANK_LOG_NONE && !(p->floor > 0.f))) return false;
    if (!std::isfinite(p->cepstral_lifter) || p->cepstral_lifter < 0.f) return false;
    return !p->reserved[0] && !p->reserved[1];
}

static std::unique_ptr<FbankTables> fbank_tables_make(const opusgpu_fbank_params &p) {
    const double pi = 3.14159265358979323846;
    std::unique_ptr<FbankTables> t(new FbankTables);
    const int L = p.frame_length, N = fbank_n_fft(p), bins = N / 2, n_mels = p.n_mels, n_ceps = p.n_ceps;
    t->L = L, t->N = N, t->bins = bins, t->n_mels = n_mels, t->n_ceps = n_ceps;
    std::vector<double> w(L);
    for (int i = 0; i < L; i++) {
        const double a = 2.0 * pi * i / (double)(L - 1);
        switch (p.window) {
        case OPUSGPU_FBANK_HANNING: w[i] = 0.5 - 0.5 * std::cos(a); break;
        case OPUSGPU_FBANK_POVEY: w[i] = std::pow(0.5 - 0.5 * std::cos(a), 0.85); break;
        case OPUSGPU_FBANK_HAMMING: w[i] = 0.54 - 0.46 * std::cos(a); break;
        case OPUSGPU_FBANK_BLACKMAN: w[i] = 0.42 - 0.5 * std::cos(a) + 0.08 * std::cos(2.0 * a); break;
        default: w[i] = 1.0;
        }
    }
    t->w.assign(w.begin(), w.end());
    // B: triangles linear in mel
    const double bw = (double)p.sample_rate / N;
    auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
    const double m_lo = mel((double)p.low_freq), m_hi = mel(fbank_high(p)), delta = (m_hi - m_lo) / (n_mels + 1);
    t->bank.assign((size_t)n_mels * bins, 0.f);
    for (int j = 0; j < n_mels; j++) {
        const double left = m_lo + j * delta, centre = left + delta, right = centre + delta;
        for (int k = 0; k < bins; k++) {
            const double m = mel(k * bw);
            t->bank[(size_t)j * bins + k] = (float)std::fmax(0.0, std::fmin((m - left) / (centre - left), (right - m) / (right - centre)));
        }
    }
    // lift[q] D[q][j]
    t->dct.assign((size_t)n_ceps * n_mels, 0.f);
    const double Q = (double)p.cepstral_lifter;
    for (int q = 0; q < n_ceps; q++) {
        const double lift = Q > 0.0 ? 1.0 + 0.5 * Q * std::sin(pi * q / Q) : 1.0;
        for (int j = 0; j < n_mels; j++) {
            const double d = q ? std::sqrt(2.0 / n_mels) * std::cos(pi * q * (j + 0.5) / n_mels) : std::sqrt(1.0 / n_mels);
            t->dct[(size_t)q * n_mels + j] = (float)(lift * d);
        }
    }
    // what the kernel loads
    t->blocks = feat_kept_blocks(t->bank, bins, n_mels);
    const int half = (L + 1) / 2, ksr = (half + 1) / 2, ks4 = (ksr + 3) / 4 * 4;
    t->half = half, t->ksr = ksr, t->ks4 = ks4;
    t->basis.assign(t->blocks.size() * ks4 * 64 * 2, 0.f);
    for (size_t b = 0; b < t->blocks.size(); b++)
        for (int ks = 0; ks < ksr; ks++)
            for (int lane = 0; lane < 64; lane++) {
                const int i = (lane >> 5) * ksr + ks, k = 32 * t->blocks[b] + (lane & 31);
                if (i >= half || k >= bins) continue;
                float *const d = &t->basis[((b * ks4 + ks) * 64 + lane) * 2];
                if (2 * i == L - 1) { // the middle tap of an odd L: u = 2 t, v = 0
                    d[0] = (float)(0.5 * w[i]);
                    continue;
                }
                // th = 2 pi k (i - (L - 1) / 2) / N = pi (k (2 i - L + 1)) / N, reduced in integers mod 2 N
                const long long m = ((long long)k * (2 * i - L + 1)) % (2 * N);
                const double th = pi * (double)m / (double)N;
                d[0] = (float)(w[i] * std::cos(th));
                d[1] = (float)(w[i] * std::sin(th));
            }
    t->fb = feat_pack_fb(t->bank, bins, n_mels, t->blocks, 4, [&](int b, int mm) { t->mask[b] |= (u8)(1u << mm); });
    t->dct_off = t->fb.size();
    if (n_ceps) {
        std::vector<int> band_blocks;
        for (int mm = 0; 32 * mm < n_mels; mm++) band_blocks.push_back(mm);
        const std::vector<float> d = feat_pack_fb(t->dct, n_mels, n_ceps, band_blocks, 4, [](int, int) {});
        t->fb.insert(t->fb.end(), d.begin(), d.end());
    }
    return t;
}

// The tables of a parameter set that fbank_params_ok has passed; safe from any number of threads.
static const FbankTables &fbank_tables(const opusgpu_fbank_params &p) {
    const FbankKey key(p.sample_rate, p.frame_length, fbank_n_fft(p), p.n_mels, p.n_ceps, p.window, p.low_freq, fbank_high(p),
                       p.n_ceps ? p.cepstral_lifter : 0.f);
    return feat_cached<FbankKey, FbankTables>(key, [&] { return fbank_tables_make(p); });
}

// ---- host side ----------------------------------------------------------------------------------------
static int64_t fbank_frames(const opusgpu_fbank_params &p, int64_t n) {
    if (p.snip_edges) return n < p.frame_length ? 0 : 1 + (n - p.frame_length) / p.frame_shift;
    return (n + p.frame_shift / 2) / p.frame_shift;
}

// k_tracks_fbank over n tracks (og_feat.hpp: tracks_feature_run).
static int tracks_fbank_run(int device, hipStream_t s, int n_tracks, const opusgpu_mel_span *spans, const void *d_in,
                            const opusgpu_fbank_params *params, void *d_out, const TrackFail &hip_failed) {
    if (!fbank_params_ok(params)) return OPUSGPU_BAD_ARG;
    const int T = feat_dense_tile(params->frame_shift, params->frame_length);
    const FbankTables *tab = nullptr;
    return tracks_feature_run(
        device, s, n_tracks, spans, d_in, d_out, T, 0x7fffffff - T, [&](int64_t n) { return fbank_frames(*params, n); },
        [&] {
            tab = &fbank_tables(*params);
            return FeatTables{&tab->basis, &tab->fb};
        },
        [&](unsigned n_tiles, const MelTile *d_tiles, const MelSpan *d_spans, const float2 *d_basis, const float *d_fb) {
            FbArgs a{};
            a.L = params->frame_length, a.H = params->frame_shift, a.n_mels = params->n_mels, a.n_ceps = params->n_ceps;
            a.n_blocks = (i32)tab->blocks.size(), a.half = tab->half, a.ksr = tab->ksr, a.ks4 = tab->ks4, a.dct_off = (i32)tab->dct_off;
            a.power = params->power, a.log = params->log, a.snip = params->snip_edges, a.remove_dc = params->remove_dc;
            a.frames_major = params->layout == OPUSGPU_MEL_FRAMES_MAJOR, a.floor = params->floor, a.preemph = params->preemphasis;
            std::copy(std::begin(tab->mask), std::end(tab->mask), a.mask);
            hipLaunchKernelGGL(k_tracks_fbank, dim3(n_tiles), dim3(2 * T),
                               feat_window_lds_bytes(params->frame_shift, params->frame_length, T, true), s, d_tiles, d_spans,
                               (const i16 *)d_in, d_basis, d_fb, a, (float *)d_out);
        },
        hip_failed);
}

// opusgpu_files_decode_fbank and its multistream twin (og_ms_tracks.hpp): files_feature_run at the record's rate.
static int files_fbank_run(const FilesOwner &own, int rate, int up, int down, int mono, const opusgpu_mix_matrix *mix,
                           const opusgpu_fbank_params *params, const float *scale, void *d_out, int64_t *feat_offsets, int64_t *frames_out,
                           int64_t *track_lengths_out, int32_t *status_out) {
    const bool ok = fbank_params_ok(params);
    const FeatFlow flow = feat_record_flow(
        ok, ok ? (int)params->sample_rate : 0, ok ? fbank_width(*params) : 0, ok && params->layout == OPUSGPU_MEL_FRAMES_MAJOR,
        "hipMalloc(fbank scratch)", [=](int64_t len) { return fbank_frames(*params, len); },
        [=](int n, const int64_t *planned, int u, int d, int64_t *feat) { return opusgpu_fbank_layout(n, planned, u, d, params, feat); },
        [&own, params](int n, const opusgpu_mel_span *spans, const void *d_in, void *d_feat) {
            return tracks_fbank_run(own.device, own.stream, n, spans, d_in, params, d_feat, own.hip_failed);
        });
    return files_feature_run(own, rate, up, down, mono, mix, scale, d_out, feat_offsets, frames_out, track_lengths_out, status_out, flow);
}

extern "C" {

int opusgpu_fbank_window(const opusgpu_fbank_params *p, const float **w) {
    if (!fbank_params_ok(p)) return OPUSGPU_BAD_ARG;
    const FbankTables &t = fbank_tables(*p);
    if (w) *w = t.w.data();
    return t.L;
}

int opusgpu_fbank_filterbank(const opusgpu_fbank_params *p, const float **b) {
    if (!fbank_params_ok(p)) return OPUSGPU_BAD_ARG;
    const FbankTables &t = fbank_tables(*p);
    if (b) *b = t.bank.data();
    return t.n_mels * t.bins;
}

int opusgpu_fbank_dct(const opusgpu_fbank_params *p, const float **d) {
    if (!fbank_params_ok(p)) return OPUSGPU_BAD_ARG;
    const FbankTables &t = fbank_tables(*p);
    if (d) *d = t.n_ceps ? t.dct.data() : nullptr;
    return t.n_ceps * t.n_mels;
}

int64_t opusgpu_fbank_layout(int n, const int64_t *planned_48k_samples, int up, int down, const opusgpu_fbank_params *p, int64_t *feat_offsets) {
    if (!fbank_params_ok(p)) return OPUSGPU_BAD_ARG;
    return feat_grid_layout(n, planned_48k_samples, up, down, fbank_width(*p), [=](int64_t len) { return fbank_frames(*p, len); }, feat_offsets);
}

int opusgpu_tracks_fbank_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in_mono,
                                const opusgpu_fbank_params *p, void *d_out, void *hip_stream) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    return tracks_fbank_run(ctx->device, hip_stream ? (hipStream_t)hip_stream : ctx->stream, n_tracks, spans, d_in_mono, p, d_out,
                            track_fail(ctx));
}

int opusgpu_files_decode_fbank(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int up, int down, int mono,
                               const opusgpu_mix_matrix *mix, const opusgpu_fbank_params *p, const float *scale, void *d_out,
                               int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out) {
    if (!ctx || !batch) return OPUSGPU_BAD_ARG;
    return files_fbank_run(files_owner(ctx, batch), rate, up, down, mono, mix, p, scale, d_out, feat_offsets, frames_out, track_lengths_out,
                           status_out);
}

} // extern "C"
