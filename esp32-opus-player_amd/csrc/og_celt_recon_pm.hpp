// og_celt_recon_pm.hpp -- the reconstruction's phase-major band loop (20 ms frames from band 0: every CELT-only frame of the BASELINE
// workloads).  Part of og_celt_recon.hpp, which includes it between the general band loop and the reconstruction's driver: it uses
// RecCur, LcgTab and recon_band_mono from there.
#pragma once

namespace og {

// recon_all_bands above walks the bands one after another because the reference does; but once the leaf pass has run,
// what a band still needs is local to it -- undoing its time-frequency change (Haar / Hadamard), its stereo merge --
// except for two things that look back: a leaf WITHOUT pulses is filled from earlier bands (their collapse masks, their
// spectrum as the folding source, the noise seed), and anti-collapse needs every band's mask.  Measured on the bench
// payloads 3 of a frame's 42 jobs have such a leaf; the per-band walk nevertheless paid ~20 dependent LDS round trips and
// ~700 scalar instructions per band for control (half of k_celt_recon's time, 15 k SALU instructions per frame).  Here:
//   B  one LANE per job (band x decode slot) reads the job's words, derives its time-frequency steps and -- for jobs
//      whose leaves all carry pulses -- its collapse mask;
//   C  those jobs' time-frequency changes are undone for the whole spectrum at once, a lane per group of 8 coefficients
//      (every band of a 20 ms frame is a multiple of 8 wide and 16-byte aligned): the interleave as a gather, Haar steps
//      of stride 1 / 2 / 4 in registers;
//   D  the jobs that do fill a leaf run one after another in decode order through the same code as the band walk
//      (recon_band_mono); their folding source is made on demand from the spectrum (the band walk's `norm` rows are
//      exactly scale(band) * X of earlier bands, taken before the stereo merge -- which is why the merge waits for E);
//   E  all stereo merges: partial sums per group of 8, one lane per band for the gains, one apply pass;
//   F  collapse masks per band (anti-collapse reads them).
// Same arithmetic per coefficient as the band walk (src/celt.cpp:1526-1741, :1113-1213), reordered only where the
// reference's order carries no dependency.
struct PmLds { // overlays the folding-history rows S.v[V_NORM ..], which this path never materialises
    u32 jdesc[2 * NBANDS];  // per (band, channel): JD_*
    u32 jaux[2 * NBANDS];   // per (band, decode slot): word position of the job header | channel << 16 | exists << 17 | fills << 18 | has pulses << 19
    u32 bw0[NBANDS], bw1[NBANDS], bw2[NBANDS];
    i32 scale[NBANDS];
    u32 mpar[NBANDS][2];    // stereo merge of the band: mode | kl << 8 | kr << 16, lgain | rgain << 16 (the mid gain is in bw2)
    u16 jcm[2 * NBANDS];    // per (band, channel): the job's collapse mask
    u8 binband[100], binoff[100]; // 5 ms bin (= group of 8 coefficients; 100 of them are coded) -> band, group index within the band
};
#ifdef OG_RECON_TIGHT
constexpr int V_PART = V_IY; // the stereo merges' partial sums take the two scratch rows (the fill jobs are done by then)
static_assert(sizeof(PmLds) <= sizeof(i16) * (V_IY - V_NORM) && 800 <= sizeof(i16) * (V_WIN - V_IY), "the phase-major tables");
#else
constexpr int V_PART = V_NORM + 600;
static_assert(sizeof(PmLds) <= sizeof(i16) * 600 && 600 + 400 <= 1248, "the phase-major tables overlay the folding-history rows");
#endif
OG_DEV PmLds &PM() { return *reinterpret_cast<PmLds *>(&S.v[V_NORM]); }
typedef i32 PmPart[2]; // per group of 8 coefficients: sum y*x, sum y*y
OG_DEV PmPart *pm_part() { return reinterpret_cast<PmPart *>(&S.v[V_PART]); }

enum { // PmLds::jdesc
    JD_VALID = 1, JD_FILL = 2,          // the job exists / has a leaf without pulses (phase D does everything for it)
    JD_PERM_SHIFT = 2 /* 3 bits: log2 of the interleave stride, 0 = none */, JD_HAD = 1 << 5,
    JD_STEP_SHIFT = 8 /* 3 Haar steps x 4 bits: 0 none, else log2(stride) + 1 */
};

struct V8 { i32 v[8]; };
OG_DEV V8 ld8(int pos) { // eight consecutive coefficients, pos a multiple of 8
    V8 r;
#ifdef OG_HOST_EMUL
    for (int k = 0; k < 8; k++) r.v[k] = S.v[pos + k];
#else
    const og_v4i p = *reinterpret_cast<const og_v4i *>(&S.v[pos]);
    r.v[0] = (i32)(i16)p.x; r.v[1] = p.x >> 16; r.v[2] = (i32)(i16)p.y; r.v[3] = p.y >> 16;
    r.v[4] = (i32)(i16)p.z; r.v[5] = p.z >> 16; r.v[6] = (i32)(i16)p.w; r.v[7] = p.w >> 16;
#endif
    return r;
}
OG_DEV void st8(int pos, const V8 &r) {
#ifdef OG_HOST_EMUL
    for (int k = 0; k < 8; k++) S.v[pos + k] = (i16)r.v[k];
#else
    og_v4i p;
    p.x = (i32)(((u32)r.v[0] & 0xffffu) | (u32)r.v[1] << 16); p.y = (i32)(((u32)r.v[2] & 0xffffu) | (u32)r.v[3] << 16);
    p.z = (i32)(((u32)r.v[4] & 0xffffu) | (u32)r.v[5] << 16); p.w = (i32)(((u32)r.v[6] & 0xffffu) | (u32)r.v[7] << 16);
    *reinterpret_cast<og_v4i *>(&S.v[pos]) = p;
#endif
}
OG_DEV void haar_pair(i32 &a, i32 &b) { // one butterfly of haar1 celt.cpp:1202
    const i32 t1 = mul16(23170, a), t2 = mul16(23170, b);
    a = tr16(pshr32(t1 + t2, 15));
    b = tr16(pshr32(t1 - t2, 15));
}
template <int S_>
OG_DEV void haar8(V8 &r) { // the Haar step of stride S_ (1, 2, 4) inside one group of 8
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (!(i & S_)) haar_pair(r.v[i], r.v[i + S_]);
}

template <bool PACKED> struct PmHold { typedef V8 type; }; // a group held between the gather's reads and its writes
template <> struct PmHold<true> { typedef W4 type; };

struct PmGrp { int band, job, x, gj, N; u32 jd; };
constexpr int PM_GROUPS = 100; // coded groups of 8 per channel (eband5ms[21] = 100)
OG_DEV PmGrp pm_group(int g) { // group g of the coded spectrum: 0..99 first channel, 100..199 second
    const PmLds &P = PM();
    PmGrp r;
    const int ch = g >= PM_GROUPS, bin = g - PM_GROUPS * ch;
    r.band = P.binband[bin];
    r.gj = P.binoff[bin];
    r.job = 2 * r.band + ch;
    r.jd = P.jdesc[r.job];
    r.x = V_X + 960 * ch + 8 * (bin - r.gj);
    r.N = (int)(P.bw1[r.band] >> 22) & 255;
    return r;
}

// B: one lane per (band, decode slot).  Returns (wave-uniform) which time-frequency passes some job needs: bit 0 the
// interleave, bit 1 + 4 k + c the Haar stride 1 << c at step k; fill_lo / fill_hi: the jobs phase D has to run.
// (`start`: the frame's first band -- 17 for the CELT layer of a hybrid frame; the bands below it have no words in the record)
// (`bw_staged`: the kernel fetched the record's band_w with its first round trip and S.band_w_row() holds it -- one dependent trip
// to the record less here)
OG_DEV u32 pm_setup_jobs(const ParseRec *rec, int C, int B, u32 &fill_lo, u32 &fill_hi, int &dual_end, int start = 0, bool bw_staged = false) {
    PmLds &P = PM();
    OG_LSYNC();
    OG_FOR_LANES(bin, PM_GROUPS) { // (tables: the search they replace was up to 21 dependent loads per lane)
        P.binband[bin] = rom_bin2band[bin];
        P.binoff[bin] = rom_binoff[bin];
    }
    OG_FOR_LANES(i, 2 * NBANDS) {
        P.jdesc[i] = 0;
        P.jcm[i] = 0;
    }
    OG_LSYNC();
    u32 tfm = 0, flo = 0, fhi = 0, de = 0;
    const int logBf = ilog2(B);
    OG_FOR_LANES(l, 2 * NBANDS) {
        const int band = l >> 1, jb = l & 1, coded = band >= start;
#ifdef OG_RECON_TIGHT
        const int bw = !coded ? 0 : bw_staged ? (int)S.band_w_row()[band] : (int)rec->band_w[band];
#else
        const int bw = coded ? (int)rec->band_w[band] : 0;
#endif
        const u32 *wp = rec->words + bw;
        const u32 w0 = coded ? wp[0] : 0u, w1 = coded ? wp[1] : 0u, w2 = coded ? wp[2] : 0u, w3 = coded ? wp[3] : 0u, jw0 = coded ? wp[4] : 0u;
        const int N = (int)(w1 >> 22) & 255;
        const int stereo = (w0 & BW_STEREO) != 0, dual = (w0 & BW_DUAL) != 0, mid_first = (w0 & BW_MID_FIRST) != 0;
        const int njobs = !coded ? 0 : (stereo || dual) ? 2 : 1;
        if (jb == 0) {
            P.bw0[band] = w0;
            P.bw1[band] = w1;
            P.bw2[band] = w2;
            P.scale[band] = (i32)(i16)(w3 & 0xffff);
            if (w0 & BW_DUAL_END) de |= 1u << band;
        }
        const int exists = jb < njobs;
        const int ch = dual ? jb : stereo ? (((jb == 0) == mid_first) ? 0 : 1) : 0;
        const int jpos = bw + 4 + (jb ? 1 + 2 * (int)(jw0 & 31) : 0);
        u32 jw = jw0;
        if (jb && exists) jw = rec->words[OG_MIN(jpos, REC_WORDS_CAP - 1)];
        const int n_fill = (int)(jw & 31), n_pvq = (int)(jw >> JW_NPVQ_SHIFT) & 31;
        P.jaux[l] = (u32)jpos | (u32)ch << 16 | (u32)exists << 17 | (u32)(exists && n_fill > 0) << 18 | (u32)(n_pvq > 0) << 19;
        if (exists) {
            // the job's time-frequency bookkeeping (quant_band celt.cpp:1548-1580), as in recon_band_mono
            int tf_change = (int)((w0 >> BW_TF_SHIFT) & 7) - 4;
            int recombine = tf_change > 0 ? tf_change : 0, time_divide = 0;
            int logB = logBf - recombine, N_B = (N >> logBf) << recombine;
            while ((N_B & 1) == 0 && tf_change < 0) {
                logB++;
                N_B >>= 1;
                time_divide++;
                tf_change++;
            }
            const int logB0 = logB;
            u32 jd = JD_VALID;
            if (logB0 > 0) jd |= (u32)(logB0 + recombine) << JD_PERM_SHIFT | (B == 1 ? JD_HAD : 0);
            int step = 0;
            for (int k = 0; k < time_divide; k++, step++) jd |= (u32)(logB0 - 1 - k + 1) << (JD_STEP_SHIFT + 4 * step);
            for (int k = 0; k < recombine; k++, step++) jd |= (u32)(k + 1) << (JD_STEP_SHIFT + 4 * step);
            if (n_fill > 0) {
                jd |= JD_FILL;
                if (l < 32) flo |= 1u << l; else fhi |= 1u << (l - 32);
            } else {
                if (logB0 > 0) tfm |= 1u;
                for (int k = 0; k < 3; k++) {
                    const int c = (int)(jd >> (JD_STEP_SHIFT + 4 * k)) & 15;
                    if (c) tfm |= 1u << (1 + 4 * k + (c - 1));
                }
                // the collapse mask of a job whose leaves all carry pulses: the leaves' masks, then what the way back
                // up does to a mask (celt.cpp:1596-1611)
                u32 cm = n_pvq ? S.job_mask_row()[l] : 0u;
                for (int k = 0; k < time_divide; k++) {
                    logB--;
                    cm |= cm >> (1 << logB);
                }
                for (int k = 0; k < recombine; k++) {
                    const u32 c4 = cm & 0xF; // bit_deinterleave_table celt.cpp:1606
                    cm = ((c4 & 1) * 0x03) | ((c4 >> 1 & 1) * 0x0C) | ((c4 >> 2 & 1) * 0x30) | ((c4 >> 3 & 1) * 0xC0);
                }
                logB += recombine;
                P.jcm[2 * band + ch] = (u16)(cm & ((1u << (1 << logB)) - 1));
            }
            P.jdesc[2 * band + ch] = jd;
        }
    }
    tfm = wave_or(tfm);
    fill_lo = wave_or(flo);
    fill_hi = wave_or(fhi);
    de = wave_or(de);
    dual_end = de ? ilog2((i32)de) : NBANDS + 1; // (at most one band ends dual stereo)
    OG_LSYNC();
    return tfm;
}

// C: undo the time-frequency changes of every job without fill leaves, a lane per group of 8 coefficients.
// (PACKED: the group stays four packed words from its read to its write -- the gather by rows, the butterflies as dot products,
// og_celt_packed.hpp; what the device runs in the tight layout.  The host emulation runs the general forms.)
template <bool PACKED = PM_PACKED>
OG_DEV void pm_tf_undo(u32 tfm) {
    constexpr int NG = (2 * PM_GROUPS + OG_NLANES - 1) / OG_NLANES;
    typedef typename PmHold<PACKED>::type Hold;
    if (tfm & 1u) { // interleave_hadamard celt.cpp:1183 as a gather: all groups read, then all write
        Hold hold[NG];
        u8 mark[NG];
#pragma unroll
        for (int it = 0; it < NG; it++) {
            const int g = OG_LANE + it * OG_NLANES;
            mark[it] = 0;
            if (g < 2 * PM_GROUPS) {
                const PmGrp q = pm_group(g);
                const int ls = (int)(q.jd >> JD_PERM_SHIFT) & 7;
                if ((q.jd & JD_VALID) && !(q.jd & JD_FILL) && ls) {
                    const int stride = 1 << ls, n0 = q.N >> ls, had = (q.jd & JD_HAD) != 0;
                    if constexpr (PACKED)
                        hold[it] = pk_gather(&S.v[q.x], q.N, q.gj, ls, had);
                    else {
#pragma unroll
                        for (int k = 0; k < 8; k++) {
                            const int inter = 8 * q.gj + k, j = inter >> ls, i = inter & (stride - 1);
                            hold[it].v[k] = S.v[q.x + (had ? ordery(stride, i) : i) * n0 + j];
                        }
                    }
                    mark[it] = 1;
                }
            }
        }
        OG_LSYNC();
#pragma unroll
        for (int it = 0; it < NG; it++) {
            const int g = OG_LANE + it * OG_NLANES;
            if (mark[it]) {
                const PmGrp q = pm_group(g);
                if constexpr (PACKED) stw4(&S.v[q.x + 8 * q.gj], hold[it]);
                else st8(q.x + 8 * q.gj, hold[it]);
            }
        }
        OG_LSYNC();
    }
    if (tfm & (1u << (1 + 3))) { // a first Haar step of stride 8 (short blocks divided once more): pairs of groups
#pragma unroll
        for (int it = 0; it < NG; it++) {
            const int g = OG_LANE + it * OG_NLANES;
            if (g < 2 * PM_GROUPS) {
                const PmGrp q = pm_group(g);
                if ((q.jd & JD_VALID) && !(q.jd & JD_FILL) && ((q.jd >> JD_STEP_SHIFT) & 15) == 4 && !(q.gj & 1)) {
                    if constexpr (PACKED) {
                        W4 a = ldw4(&S.v[q.x + 8 * q.gj]), b = ldw4(&S.v[q.x + 8 * q.gj + 8]);
                        pk_haar16(a, b);
                        stw4(&S.v[q.x + 8 * q.gj], a);
                        stw4(&S.v[q.x + 8 * q.gj + 8], b);
                    } else {
                        V8 a = ld8(q.x + 8 * q.gj), b = ld8(q.x + 8 * q.gj + 8);
#pragma unroll
                        for (int k = 0; k < 8; k++) haar_pair(a.v[k], b.v[k]);
                        st8(q.x + 8 * q.gj, a);
                        st8(q.x + 8 * q.gj + 8, b);
                    }
                }
            }
        }
        OG_LSYNC();
    }
    if (tfm & 0x0eeeu) { // Haar steps of stride 1 / 2 / 4: inside a group, in registers, up to three in a row
#pragma unroll
        for (int it = 0; it < NG; it++) {
            const int g = OG_LANE + it * OG_NLANES;
            if (g < 2 * PM_GROUPS) {
                const PmGrp q = pm_group(g);
                const u32 steps = (q.jd & JD_VALID) && !(q.jd & JD_FILL) ? (q.jd >> JD_STEP_SHIFT) & 0xfffu : 0u;
                if (steps & 0x777u) { // (a step of stride 8 has code 4: bit 3 of its nibble only)
                    if constexpr (PACKED) {
                        W4 r = ldw4(&S.v[q.x + 8 * q.gj]);
                        for (int k = 0; k < 3; k++) {
                            const int c = (int)(steps >> (4 * k)) & 15;
                            if (c == 1) pk_haar8_1(r);
                            else if (c == 2) pk_haar8_2(r);
                            else if (c == 3) pk_haar8_4(r);
                        }
                        stw4(&S.v[q.x + 8 * q.gj], r);
                    } else {
                        V8 r = ld8(q.x + 8 * q.gj);
                        for (int k = 0; k < 3; k++) {
                            const int c = (int)(steps >> (4 * k)) & 15;
                            if (c == 1) haar8<1>(r);
                            else if (c == 2) haar8<2>(r);
                            else if (c == 3) haar8<4>(r);
                        }
                        st8(q.x + 8 * q.gj, r);
                    }
                }
            }
        }
        OG_LSYNC();
    }
}

// the folding source of job (band i, channel ch) made on demand: `n` entries from position p0 of the folding history as the
// band walk would hold it when band i starts (lowband_out of the earlier bands, celt.cpp:1617; the two channels' histories
// averaged once dual stereo has ended, celt.cpp:1856-1860)
// (p0 counts from the frame's first band, like the folding history of the band walk: norm_offset celt.cpp:1787.  `dup`: the
// second band of a frame that starts above band 0 is wider than the first, and the band walk fills the hole behind the first
// band's history with a copy of its end -- special_hybrid_folding celt.cpp:1743: entries from n1 on repeat the n2 - n1 before n1)
OG_DEV void pm_make_lowband(int dst, int p0, int n, int i, int use_y, int dual_end, int norm_offset = 0, int dup_n1 = 0, int dup_back = 0) {
    const PmLds &P = PM();
    OG_LSYNC();
    OG_FOR_LANES(j, n) {
        int r = p0 + j;
        const bool copied = dup_back && r >= dup_n1;
        if (copied) r -= dup_back;
        const int p = norm_offset + r, sb = P.binband[p >> 3];
        const i32 sc = P.scale[sb];
        i32 v;
        // (the copy is made before dual stereo is switched off at this very band, and that averages only the histories of the
        // bands before it, celt.cpp:1856-1860: the copied entries stay the first channel's)
        if (i >= dual_end && sb < dual_end && !copied)
            v = ((i32)(i16)mul16_q15(sc, S.v[V_X + p]) + (i32)(i16)mul16_q15(sc, S.v[V_X + 960 + p])) >> 1;
        else
            v = mul16_q15(sc, S.v[V_X + (use_y ? 960 : 0) + p]);
        S.v[dst + j] = (i16)v;
    }
    OG_LSYNC();
}

// collapse mask of band b, channel c (what the band walk keeps in S.cmask)
OG_DEV u32 pm_band_cm(int b, int c) {
    const PmLds &P = PM();
    const u32 w0 = (u32)OG_UNI(P.bw0[b]);
    if (w0 & BW_STEREO) return (u32)OG_UNI(P.jcm[2 * b]) | (u32)OG_UNI(P.jcm[2 * b + 1]);
    return (u32)OG_UNI(P.jcm[2 * b + ((w0 & BW_DUAL) ? c : 0)]);
}

// D: the jobs with leaves without pulses, in decode order
OG_DEV void pm_fill_jobs(const u32 *words, const LcgTab &lcg, u32 fill_lo, u32 fill_hi, int C, int B, int dual_end, u32 &seed,
                         int start = 0) {
    const int norm_offset = 8 * rom_eband[start];
    const int dup_n1 = 8 * (rom_eband[start + 1] - rom_eband[start]), dup_n2 = 8 * (rom_eband[start + 2] - rom_eband[start + 1]);
    PmLds &P = PM();
    RecCur cur;
    cur.words = words;
    cur.w = 0;
    cur.base = -64;
    cur.leaf = 0;
    for (int l = 0; l < 2 * NBANDS; l++) {
        if (!((l < 32 ? fill_lo >> l : fill_hi >> (l - 32)) & 1u)) continue;
        OG_MARK(5);
        OG_STAT(20, 1);                             // fill jobs
        const int i = l >> 1, jb = l & 1;
        const u32 aux = (u32)OG_UNI(P.jaux[l]), w0 = (u32)OG_UNI(P.bw0[i]), w1 = (u32)OG_UNI(P.bw1[i]);
        const int ch = (int)(aux >> 16) & 1;
        const int eb0 = (int)(w1 >> 11) & 2047, N = (int)(w1 >> 22) & 255;
        const int tf_change = (int)((w0 >> BW_TF_SHIFT) & 7) - 4;
        const int stereo = (w0 & BW_STEREO) != 0, dual = (w0 & BW_DUAL) != 0;
        u32 x_cm, y_cm;
        if (w0 & BW_HAS_LOW) {
            const int fold_end = (int)(w0 >> BW_FOLD1_SHIFT) & 31;
            int fold_i = (int)(w0 >> BW_FOLD0_SHIFT) & 31;
            x_cm = y_cm = 0;
            do {
                x_cm |= pm_band_cm(fold_i, 0);
                y_cm |= pm_band_cm(fold_i, C - 1);
            } while (++fold_i < fold_end);
        } else
            x_cm = y_cm = (1u << B) - 1;
        i32 jfill;
        int want_low;
        if (dual) {
            jfill = (i32)(jb ? y_cm : x_cm);
            want_low = 1;
        } else {
            i32 fill0 = (i32)(x_cm | y_cm);
            if (stereo) {
                if (w0 & BW_THETA0) fill0 &= (1 << B) - 1;
                if (w0 & BW_THETA1) fill0 &= ((1 << B) - 1) << B;
            }
            jfill = ch ? fill0 >> B : fill0; // (channel 1 of a stereo band is the side)
            want_low = !ch;                  // the side never folds (celt.cpp:1709)
        }
        if (jfill == 0 && !(OG_UNI(P.jaux[l]) >> 19 & 1)) { // nothing to fill with and no pulses: the job's spectrum stays zero
            OG_STAT(24, 1);
            continue; // (its mask P.jcm is zero from the set-up, the seed does not move: celt.cpp:1481-1520 under `if (fill)`)
        }
        cur.w = (int)(aux & 0xffff);
        OG_STAT(27, 1);                             // fill jobs that run
        const u32 jw = rec_word(cur);
        int low = -1;
        if ((w0 & BW_HAS_LOW) && want_low && (jw & JW_NEED_LOW)) {
            const int dup = (i == start + 1 && dup_n2 > dup_n1) ? dup_n2 - dup_n1 : 0;
            pm_make_lowband(V_IY, (int)(w1 & 2047), N, i, dual && ch, dual_end, norm_offset, dup_n1, dup);
            low = V_IY;
        }
        const u32 cm = recon_band_mono(cur, jw, lcg, tf_change, seed, V_X + 960 * ch + eb0, N, B, low, -1, 0, -1, jfill, l);
        if (OG_LANE == 0) P.jcm[2 * i + ch] = (u16)cm;
        OG_LSYNC();
    }
}

// E: every stereo merge of the frame (stereo_merge celt.cpp:1113, the sign flip of celt.cpp:1731)
// (PACKED: the sums and the apply pass on packed words, og_celt_packed.hpp; as for pm_tf_undo)
template <bool PACKED = PM_PACKED>
OG_DEV void pm_stereo_merge(int C) {
    PmLds &P = PM();
    if (C != 2) return;
    OG_LSYNC();
    // (the band edges of the lane-per-band pass below: requested here, ahead of the partial sums -- behind the barrier that
    // closes them the pass waited a round trip for the pair)
    const int eb_lo = rom_eband[OG_MIN(OG_LANE, NBANDS - 1)], eb_hi = rom_eband[OG_MIN(OG_LANE, NBANDS - 1) + 1];
    OG_FOR_LANES(g, PM_GROUPS) { // partial sums of a group of 8
        const int band = P.binband[g];
        if (P.bw0[band] & BW_STEREO) {
            OG_STAT(29, 1);                         // groups whose partial sums are taken
            i32 xp = 0, side = 0;
            if constexpr (PACKED)
                pk_merge_sums(ldw4(&S.v[V_X + 8 * g]), ldw4(&S.v[V_X + 960 + 8 * g]), xp, side);
            else {
                const V8 a = ld8(V_X + 8 * g), b = ld8(V_X + 960 + 8 * g);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    xp += mul16(b.v[k], a.v[k]);
                    side += mul16(b.v[k], b.v[k]);
                }
            }
            pm_part()[g][0] = xp;
            pm_part()[g][1] = side;
        }
    }
    OG_LSYNC();
    OG_FOR_LANES(band, NBANDS) { // the band's two gains
        const u32 w0 = P.bw0[band];
        if (w0 & BW_STEREO) {
            // (one band per lane and one pass, band == lane: the pair fetched above; the one-lane emulation walks the bands)
            const int g0 = OG_NLANES > 1 ? eb_lo : rom_eband[band], g1 = OG_NLANES > 1 ? eb_hi : rom_eband[band + 1];
            i32 xp = 0, side = 0;
            for (int g = g0; g < g1; g++) {
                xp += pm_part()[g][0];
                side += pm_part()[g][1];
            }
            const i32 mid = (i32)(i16)(P.bw2[band] & 0xffff);
            xp = mul16x32_q15(mid, xp);
            const i32 mid2 = tr16(mid >> 1);
            const i32 El = mul16(mid2, mid2) + side - 2 * xp, Er = mul16(mid2, mid2) + side + 2 * xp;
            i32 mode = 1, lgain = 0, rgain = 0;
            int kl = 0, kr = 0;
            if (Er < 161061 || El < 161061) // QCONST32(6e-4f, 28): the right channel becomes a copy of the left
                mode = 2;
            else {
                kl = ilog2(El) >> 1;
                kr = ilog2(Er) >> 1;
                lgain = rsqrt_norm(vshr32(El, (kl - 7) << 1));
                rgain = rsqrt_norm(vshr32(Er, (kr - 7) << 1));
                if (kl < 7) kl = 7;
                if (kr < 7) kr = 7;
            }
            if (w0 & BW_INV) mode |= 4;
            P.mpar[band][0] = (u32)(mode | kl << 8 | kr << 16);
            P.mpar[band][1] = ((u32)lgain & 0xffffu) | (u32)rgain << 16;
        } else
            P.mpar[band][0] = 0u;
    }
    OG_LSYNC();
    OG_FOR_LANES(g, PM_GROUPS) {
        const int band = P.binband[g];
        const i32 m0 = (i32)P.mpar[band][0];
        if (m0 & 3) {
            const u32 m1 = P.mpar[band][1];
            const i32 lgain = (i32)(i16)(m1 & 0xffff), rgain = (i32)m1 >> 16, mid = (i32)(i16)(P.bw2[band] & 0xffff);
            const int kl = (m0 >> 8) & 255, kr = (m0 >> 16) & 255;
            OG_STAT(37, 1);                         // groups merged
            OG_STAT(38, (m0 & 2) != 0);             // ... in the copy mode
            if constexpr (PACKED) {
                W4 a = ldw4(&S.v[V_X + 8 * g]), b;
                if (m0 & 2)
                    b = (m0 & 4) ? pk_neg(a) : a;
                else {
                    b = ldw4(&S.v[V_X + 960 + 8 * g]);
                    pk_merge_apply(a, b, mid, lgain, rgain, kl, kr, (m0 & 4) != 0);
                    stw4(&S.v[V_X + 8 * g], a);
                }
                stw4(&S.v[V_X + 960 + 8 * g], b);
            } else {
                V8 a = ld8(V_X + 8 * g), b = ld8(V_X + 960 + 8 * g);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    i32 xo, yo;
                    if (m0 & 2) {
                        xo = a.v[k];
                        yo = a.v[k];
                    } else {
                        const i32 l = tr16(mul16_p15(mid, a.v[k])), r = b.v[k];
                        xo = tr16(pshr32(mul16(lgain, sub16(l, r)), kl + 1));
                        yo = tr16(pshr32(mul16(rgain, add16(l, r)), kr + 1));
                    }
                    a.v[k] = xo;
                    b.v[k] = (m0 & 4) ? tr16(-yo) : yo;
                }
                if (!(m0 & 2)) st8(V_X + 8 * g, a);
                st8(V_X + 960 + 8 * g, b);
            }
        }
    }
    OG_LSYNC();
}

OG_DEV void recon_all_bands_pm(const ParseRec *rec, LcgTab &lcg, int C, int shortBlocks, u32 &seed_io, int start = 0, bool bw_staged = false) {
    const int B = shortBlocks ? 8 : 1;
    u32 fill_lo, fill_hi, seed = seed_io;
    int dual_end;
    OG_MARK(3);
    const u32 tfm = pm_setup_jobs(rec, C, B, fill_lo, fill_hi, dual_end, start, bw_staged);
    if (fill_lo | fill_hi) lcg.hold(); // the lane's noise-generator pair, for the fill jobs: in flight during the parallel pass
#if defined(OG_HOST_EMUL) && defined(OG_STATS)
    { // fill jobs per frame, and how far apart their words lie in the record (tests/test_fill_windows_emul.py)
        int n_fill_jobs = 0, w_prev = -1;
        bool close_pair = false;
        for (int l = 0; l < 2 * NBANDS; l++)
            if ((l < 32 ? fill_lo >> l : fill_hi >> (l - 32)) & 1u) {
                const int w = (int)(PM().jaux[l] & 0xffff);
                close_pair |= w_prev >= 0 && w - w_prev < 64;
                w_prev = w;
                n_fill_jobs++;
            }
        OG_STAT(33, n_fill_jobs == 0);              // frames with no / one / four or more fill jobs
        OG_STAT(34, n_fill_jobs == 1);
        OG_STAT(35, n_fill_jobs >= 4);
        OG_STAT(36, close_pair);                    // frames with two fill jobs less than a window apart
    }
    { // the parallel pass's work by class of job (tools/tf_undo_census.py): groups of 8 coefficients
        OG_STAT(25, (tfm & (1u << 4)) != 0);        // frames that run the pass over pairs of groups (a first Haar step of stride 8)
        OG_STAT(28, (tfm & 0x0eeeu) != 0);          // frames that run the pass of Haar steps inside a group
        for (int l = 0; l < 2 * NBANDS; l++) {
            const u32 jd = PM().jdesc[l];
            const int groups = (int)((PM().bw1[l >> 1] >> 22) & 255) / 8;
            if (!(jd & JD_VALID) || !(jd & ~(u32)(JD_VALID | JD_FILL))) continue; // no job, or a job without a change
            if (jd & JD_FILL) {
                OG_STAT(60, groups);                // groups of jobs with a change that phase D undoes (fill jobs)
                continue;
            }
            const u32 steps = (jd >> JD_STEP_SHIFT) & 0xfffu; // (step k in nibble k)
            const int ls = (int)(jd >> JD_PERM_SHIFT) & 7, had = (jd & JD_HAD) != 0;
            OG_STAT(ls == 2 && had && steps == 0x012u ? 39   // long block: stride 4 ordered, steps (2, 1)
                    : ls == 3 && had && steps == 0x123u ? 43 // long block: stride 8 ordered, steps (3, 2, 1)
                    : ls == 0 && steps == 0x321u ? 47        // transient: no interleave, steps (1, 2, 3)
                    : ls == 3 && !had && steps == 0x001u ? 48 // transient: stride 8, step (1)
                    : ls == 3 && !had && steps == 0u ? 49    // transient: stride 8, no step
                    : ls == 4 && !had && steps == 0x004u ? 54 // transient: stride 16, the step over pairs of groups
                    : 55, groups);                  // anything else
        }
    }
#endif
    OG_STAT(0, 1);                                  // frames
    OG_STAT(19, shortBlocks != 0);                  // transient frames
    OG_STAT(21, tfm != 0);                          // frames with a time-frequency change to undo in the parallel pass
    OG_STAT(22, (tfm & 1u) != 0);                   // ... with an interleave among them
    OG_STAT(23, (fill_lo | fill_hi) != 0);          // frames with fill jobs
    OG_MARK(8);
    if (tfm) pm_tf_undo(tfm);
    if (fill_lo | fill_hi) pm_fill_jobs(rec->words, lcg, fill_lo, fill_hi, C, B, dual_end, seed, start);
    OG_MARK(10);
    pm_stereo_merge(C);
    OG_MARK(4);
    OG_FOR_LANES(t, NBANDS * C) { // F: the bands' collapse masks where anti-collapse looks for them
        const PmLds &P = PM();
        const int b = t / C, c = t - b * C;
        const u32 w0 = P.bw0[b];
        const u32 cm = (w0 & BW_STEREO) ? (u32)P.jcm[2 * b] | (u32)P.jcm[2 * b + 1] : (u32)P.jcm[2 * b + ((w0 & BW_DUAL) ? c : 0)];
        S.cmask_row()[t] = (u8)cm;
    }
    OG_LSYNC();
    seed_io = seed;
}

#ifdef OG_RECON_TIGHT
// anti_collapse (celt.cpp:1010) of the 20 ms kernel, in whole-wave passes.  The band-by-band form (og_celt_recon.hpp) visits every
// (band, channel, block) cell of a transient frame -- 336 of them -- one after the other: a barrier, a fill by N0 <= 22 lanes
// and two dependent table loads per collapsed cell, a renormalise() per band touched.  What ties the cells together is only the
// noise generator, which the reference steps in the order band, channel, block, N0 draws per collapsed block; a jump ahead is
// one multiply-add (LcgTab), so every draw can be named by its position:
//   1  lane (band i, channel c), in the order e = i C + c, counts its collapsed blocks; an exclusive prefix over the wave of
//      (blocks x N0) is the number of draws before the entry, and lcg_skip by it (at most 1,600) the entry's seed;
//   2  a lane per group of 8 coefficients: coefficient j's eight blocks are the 16 contiguous bytes at x + 8 j.  Block k, if
//      collapsed, takes the sign of draw rank(k) N0 + j of its entry (rank: collapsed blocks below k; at most 7 * 22 + 21 = 175,
//      inside rom_lcg_jump).  The group's sum of squares is taken while its values are in registers;
//   3  a lane per entry adds its groups' sums (wrapping 32-bit sums: any order) and derives the gain of renormalise();
//   4  one apply pass over the groups of the entries that had a fill.
// The per-entry words lie beside r in the Hadamard scratch row, the groups' sums over the front of the band loop's tables
// (jdesc .. jcm: dead since the bands' collapse masks were gathered; binband / binoff behind them are still read here).
static_assert(sizeof(i32) * 2 * PM_GROUPS <= offsetof(PmLds, binband), "the groups' sums end before the bin tables");
static_assert(48 + 2 * 2 * NBANDS <= 200 && (V_TMP + 48) % 2 == 0, "r and the entries' words fit the scratch row");
OG_DEV void anti_collapse_pm(const LcgTab &lcg, int LM, int C, int size, int start, int end, u32 seed) {
    const PmLds &P = PM();
    const i16 *const rrow = anti_collapse_r(LM, C, start, end);
    u32 *const ent = reinterpret_cast<u32 *>(&S.v[V_TMP + 48]); // per entry e: its seed, then gain | shift << 16 | touched << 31
    i32 *const part = reinterpret_cast<i32 *>(&S.v[V_NORM]);    // per (channel, group): sum of squares
    const int NE = C * NBANDS;
    OG_STAT(32, 1);                                             // frames that run anti-collapse
    u32 run = 0; // (one lane: the prefix as a running sum)
    (void)run;
    OG_FOR_LANES(e, OG_NLANES > 1 ? OG_NLANES : NE) { // (every lane of the wave takes part in the prefix)
        const int i = C == 2 ? e >> 1 : e;
        int draws = 0;
        if (e < NE && i >= start && i < end) {
            const int cnt = __builtin_popcount(~(u32)S.cmask_row()[e] & 0xffu);
            draws = cnt * (rom_eband[i + 1] - rom_eband[i]);
            OG_STAT(30, cnt);                                   // cells filled
            OG_STAT(31, cnt != 0);                              // (band, channel) entries renormalised
        }
#ifdef OG_HOST_EMUL
        const u32 before = run;
        run += (u32)draws;
#else
        const u32 before = (u32)(wave_scan_add(draws) - draws);
#endif
        if (e < NE) ent[e] = lcg_skip(seed, before);
    }
    OG_LSYNC();
    OG_FOR_LANES(t, C * PM_GROUPS) {
        const int c = t >= PM_GROUPS, g = t - PM_GROUPS * c;
        const int i = P.binband[g], j = P.binoff[g], e = i * C + c;
        const u32 clr = (i >= start && i < end) ? ~(u32)S.cmask_row()[e] & 0xffu : 0u;
        if (clr) {
            const int N0 = rom_eband[i + 1] - rom_eband[i];
            const i32 r = rrow[c * NBANDS + i];
            const u32 base = ent[e];
            V8 x = ld8(V_X + c * size + 8 * g);
            int at = j;
            i32 ss = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const u32 s = lcg.at(base, at); // (a block that is not filled names the next one's draw: inside the table)
                if ((clr >> k) & 1u) {
                    x.v[k] = (i16)((s & 0x8000) ? r : -r);
                    at += N0;
                }
                ss += mul16(x.v[k], x.v[k]);
            }
            st8(V_X + c * size + 8 * g, x);
            part[t] = ss;
        }
    }
    OG_LSYNC();
    OG_FOR_LANES(e, NE) { // renormalise()'s gain for the entries that had a fill
        const int i = C == 2 ? e >> 1 : e, c = e - i * C;
        u32 w = 0;
        if (i >= start && i < end && (~(u32)S.cmask_row()[e] & 0xffu)) {
            const int g0 = rom_eband[i], g1 = rom_eband[i + 1];
            i32 E = 1;
            for (int g = g0; g < g1; g++) E += part[c * PM_GROUPS + g];
            const int k = ilog2(E) >> 1;
            const i32 t = vshr32(E, 2 * (k - 7));
            const i32 gn = tr16(mul16_p15(rsqrt_norm(t), 32767));
            w = ((u32)gn & 0xffffu) | (u32)((k + 1) & 63) << 16 | 1u << 31;
        }
        ent[e] = w;
    }
    OG_LSYNC();
    OG_FOR_LANES(t, C * PM_GROUPS) {
        const int c = t >= PM_GROUPS, g = t - PM_GROUPS * c;
        const u32 w = ent[P.binband[g] * C + c];
        if (w) {
            const i32 gn = (i32)(i16)(w & 0xffff);
            const int sh = (int)(w >> 16) & 63;
            V8 x = ld8(V_X + c * size + 8 * g);
#pragma unroll
            for (int k = 0; k < 8; k++) x.v[k] = (i16)pshr32(mul16(gn, x.v[k]), sh);
            st8(V_X + c * size + 8 * g, x);
        }
    }
    OG_LSYNC();
}
#endif

} // namespace og
