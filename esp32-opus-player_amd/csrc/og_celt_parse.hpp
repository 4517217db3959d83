// og_celt_parse.hpp -- the split CELT path's first stage: entropy decoding with ONE FRAME PER LANE into a ParseRec per frame
// (og_celt_rec.hpp says why the frame splits there).  The kernel around it: og_parse_kernel.hpp.
#pragma once
#include "og_celt.hpp"
#include "og_celt_rec.hpp"

namespace og {

// Frames per parse wave (= lanes that carry a frame; the [element][lane] arrays below are that wide).  Fewer than the wave's
// 64 lanes means more, smaller waves: less LDS per wave (more of them resident per SIMD) and a shorter divergent union.
#ifndef OG_PL_LANES
#define OG_PL_LANES (OG_NLANES >= 32 ? 32 : OG_NLANES) // measured: 64 / 32 / 16 frames per wave, see DESIGN.md section 6
#endif
// Waves per parse workgroup (they share one copy of the ROM tables, ParseTabLds, 3.3 KB: LDS per wave goes from 13 granules of
// 1280 bytes to 11.5 at two, 10.75 at four).  Measured next to the reconstruction in pipelined steps (opusgpu_set_pipeline), where
// LDS is what the two kernels compete for: 2.74 ms per step at one, 2.73 at two, 2.80 at four (a workgroup's LDS stays
// allocated until its slowest wave is done) -- so one.
#ifndef OG_PL_WAVES
#define OG_PL_WAVES 1
#endif
// a thread's wave within the workgroup and the column of its frame in that wave's [element][column] arrays
#ifdef OG_HOST_EMUL
#define OG_PWAVE 0
#define OG_PCOL OG_LANE
#else
#define OG_PWAVE ((int)(threadIdx.x >> 6))
#define OG_PCOL ((int)(threadIdx.x & 63))
#endif
#define OG_PL_FRAMES (OG_PL_LANES * OG_PL_WAVES) // frames per workgroup
struct ParseLds { // [element][lane]: lanes of a wave touch consecutive addresses, no bank conflicts
    // (from the dynalloc boosts until compute_allocation settles the fine bits, fine_quant holds the bands' BOOST COUNTS -- see LaneArr::boost)
    i8 fine_quant[NBANDS][OG_PL_LANES];
    i8 tf_prio[NBANDS][OG_PL_LANES]; // bits 0-3: tf_res (-3 .. 3, two's complement), bit 4: fine_prio
    // Three tenants, one after the other (next to the reconstruction the kernel's LDS is what keeps that kernel's waves out: 16.1 KB
    // per wave of 32 frames in round 2, 14.0 with the caps computed and tf_res / fine_prio in one byte, 11.3 with the energies resting, 8.6 with OG_PARSE_PULSES_REC):
    union {
        // the band energies while the header's energy stages and energy_finalise work on them (coarse energy .. , fine energy, the
        // finalise pass); in between they rest in the frame's record (LaneArr::energies_rest / energies_back: 21 words each way)
        i16 bandE[2 * NBANDS][OG_PL_LANES];
        struct { // from the dynalloc boosts until compute_allocation returns, i.e. before the first band is parsed
            // (the bands' caps are computed where they are used: celt_band_cap; their dynalloc boosts rest as counts in fine_quant)
            // One word per band: the two allocation vectors' entries (bits1 | bits2 << 16) while compute_allocation interpolates
            // between them, then -- written over them band by band by the pass that settles the interpolation -- the band's bits
            // (32 bits: a frame whose budget went negative carries wrapped values here, as the reference does).  When the allocation
            // is done they move to the frame's record (LaneArr::pulses_rest), where the band walk reads one per band.  Round 5: the
            // bits had an array of their own here, a third of the kernel's LDS -- which is what keeps the reconstruction's waves
            // off the CUs the parse kernel runs on.
            u32 bw[NBANDS][OG_PL_LANES];
        } al;
        i32 stack[4][5][OG_PL_LANES]; // split frames of the partition walk: [depth][word][lane] (every split takes one off LM = 3: four deep at most)
    } u;
};
// One per wave.  The union below is private to a wave only because its lanes reconverge between compute_allocation and the band
// walk; two waves of a workgroup do not, so they must not share rows of it.
// OG_PARSE_DYN_LDS (og_parse64.hip): the parse kernel's LDS as DYNAMIC shared memory, sized at the launch.  The compiler derives
// a kernel's occupancy -- and from it the register budget it allocates to -- from the LDS it can see, and with 46 KB per
// workgroup it saw two waves per SIMD and took 219 of their 256 registers, whatever the kernel was told to aim for; a SIMD that
// holds such a wave has registers left for three of the reconstruction's waves, not for five.
#ifdef OG_PARSE_DYN_LDS
extern __shared__ __attribute__((aligned(16))) unsigned char og_dyn_lds[];
#define PLs (reinterpret_cast<ParseLds *>(og_dyn_lds))
#else
OG_LDS ParseLds PLs[OG_PL_WAVES];
#endif
#define PL PLs[OG_PWAVE]

// LDS copy of the entropy-decoding ROM tables (see RomGlobal, og_celt_bands.hpp), loaded once per workgroup
struct ParseTabLds {
    i16 eband[NBANDS + 1], logn[NBANDS];
    u16 pulse_idx[105];
    u32 pulse_v[392]; // size of the PVQ codebook a leaf's index is decoded against, by pulse-cache index (rom_pulse_v)
    u8 pulse_bits[392], band_alloc[231], pulse_caps[168], log2_frac[24], eprob[336];
};
#ifdef OG_PARSE_DYN_LDS
#define PT (*reinterpret_cast<ParseTabLds *>(og_dyn_lds + sizeof(ParseLds) * OG_PL_WAVES))
#define OG_PARSE_LDS_BYTES (sizeof(ParseLds) * OG_PL_WAVES + sizeof(ParseTabLds))
#else
OG_LDS ParseTabLds PT;
#define OG_PARSE_LDS_BYTES 0
#endif
struct RomLds {
    static OG_MEMBER i32 eband(int i) { return PT.eband[i]; }
    static OG_MEMBER i32 logn(int i) { return PT.logn[i]; }
    static OG_MEMBER i32 pulse_idx(int i) { return PT.pulse_idx[i]; }
    static OG_MEMBER i32 pulse_bits(int i) { return PT.pulse_bits[i]; }
    static OG_MEMBER i32 band_alloc(int i) { return PT.band_alloc[i]; }
    static OG_MEMBER i32 pulse_caps(int i) { return PT.pulse_caps[i]; }
    static OG_MEMBER i32 log2_frac(int i) { return PT.log2_frac[i]; }
    static OG_MEMBER i32 eprob(int i) { return PT.eprob[i]; }
};
// cooperative load by the whole workgroup (call before any lane leaves the kernel); ends with a barrier
OG_DEV void parse_tables_load() {
    OG_FOR_LANES(i, NBANDS + 1) PT.eband[i] = rom_eband[i];
    OG_FOR_LANES(i, NBANDS) PT.logn[i] = rom_logn[i];
    OG_FOR_LANES(i, 105) PT.pulse_idx[i] = rom_pulse_idx[i];
    OG_FOR_LANES(i, 392) PT.pulse_bits[i] = rom_pulse_bits[i];
    OG_FOR_LANES(i, 392) PT.pulse_v[i] = rom_pulse_v[i];
    OG_FOR_LANES(i, 231) PT.band_alloc[i] = rom_band_alloc[i];
    OG_FOR_LANES(i, 168) PT.pulse_caps[i] = rom_pulse_caps[i];
    OG_FOR_LANES(i, 24) PT.log2_frac[i] = rom_log2_frac[i];
    OG_FOR_LANES(i, 336) PT.eprob[i] = rom_eprob[i];
    OG_FULL_SYNC();
}

// tf_res and fine_prio of a band share a byte of the lane's column: what the shared header code sees are these two views of it
struct TfResView {
    i8 *p;
    OG_MEMBER operator int() const { return (int)(i8)((u8)*p << 4) >> 4; }
    OG_MEMBER void operator=(int v) const { *p = (i8)((*p & 0xF0) | (v & 15)); }
};
struct FinePrioView {
    i8 *p;
    OG_MEMBER operator int() const { return (*p >> 4) & 1; }
    OG_MEMBER void operator=(int v) const { *p = (i8)((*p & ~0x10) | ((v & 1) << 4)); }
};
struct LaneArr {
    typedef RomLds Rom;
    i32 *pl;   // the bits-per-band array once compute_allocation is done: in the frame's record (ParseRec::work_pulses)
    i16 *rest; // where the band energies rest while the allocation scratch / the partition stack have their LDS: the record's bandE
    i16 *pk;   // the record's 16-bit copy of the bits per band (ParseRec::pulses: what the reconstruction's anti-collapse reads)
    // (pairs of bands per 32-bit access; every load is requested before the first is used)
    OG_MEMBER void energies_rest() const {
        for (int i = 0; i < 2 * NBANDS; i += 2)
            *reinterpret_cast<u32 *>(&rest[i]) = (u32)(u16)PL.u.bandE[i][OG_PCOL] | (u32)(u16)PL.u.bandE[i + 1][OG_PCOL] << 16;
    }
    OG_MEMBER void energies_back() const {
        u32 w[NBANDS];
        for (int i = 0; i < NBANDS; i++) w[i] = *reinterpret_cast<const u32 *>(&rest[2 * i]);
        for (int i = 0; i < NBANDS; i++) {
            PL.u.bandE[2 * i][OG_PCOL] = (i16)(w[i] & 0xffff);
            PL.u.bandE[2 * i + 1][OG_PCOL] = (i16)(w[i] >> 16);
        }
    }
    typedef u16 __attribute__((may_alias)) u16a;
    typedef i32 __attribute__((may_alias)) i32a;
    OG_MEMBER i32 &pulses(int i) const { return pl[i]; }
    OG_MEMBER i32a &alloc_bits(int i) const { return *reinterpret_cast<i32a *>(&PL.u.al.bw[i][OG_PCOL]); }
    // the allocation is done: bands start .. end - 1 to the record (zero outside), four words per store
    OG_MEMBER void pulses_rest(int start, int end) const {
        i32 v[24];
        for (int i = 0; i < 24; i++) v[i] = (i >= start && i < end) ? (i32)PL.u.al.bw[i < NBANDS ? i : 0][OG_PCOL] : 0;
#ifdef OG_HOST_EMUL
        for (int i = 0; i < NBANDS; i++) pl[i] = v[i];
#else
        typedef i32 i32x4 __attribute__((ext_vector_type(4)));
        for (int i = 0; i < 24; i += 4) *reinterpret_cast<i32x4 *>(&pl[i]) = i32x4{v[i], v[i + 1], v[i + 2], v[i + 3]};
#endif
        for (int i = 0; i < NBANDS; i++) pk[i] = (i16)v[i];
    }
    OG_MEMBER i8 &fine_quant(int i) const { return PL.fine_quant[i][OG_PCOL]; }
    OG_MEMBER FinePrioView fine_prio(int i) const { return FinePrioView{&PL.tf_prio[i][OG_PCOL]}; }
    OG_MEMBER TfResView tf_res(int i) const { return TfResView{&PL.tf_prio[i][OG_PCOL]}; }
    // A band's dynalloc boost is a whole number of the band's quanta, at most 66 of them (dynalloc_quanta), and nothing reads
    // fine_quant between the boosts and the end of compute_allocation, whose last loop writes it after the last boost was read:
    // the count rests in that byte (zero from celt_parse_lane for the bands a frame does not code) and the bits are a multiply
    // away.  An i16 array of the boosts took 2.7 KB of a 64-frame wave's LDS: the workgroup's 20 granules are 16 without it.
    OG_MEMBER void boost_put(int i, int n, int) const {
#ifdef OG_HOST_EMUL
        if (n < 0 || n > 127) __builtin_trap();
#endif
        PL.fine_quant[i][OG_PCOL] = (i8)n;
    }
    OG_MEMBER i32 boost(int i, int C, int LM) const { return (i32)PL.fine_quant[i][OG_PCOL] * dynalloc_quanta<RomLds>(i, LM, C); }
    OG_MEMBER u16a &bits1(int i) const { return reinterpret_cast<u16a *>(&PL.u.al.bw[i][OG_PCOL])[0]; }
    OG_MEMBER u16a &bits2(int i) const { return reinterpret_cast<u16a *>(&PL.u.al.bw[i][OG_PCOL])[1]; }
    OG_MEMBER i16 &bandE(int i) const { return PL.u.bandE[i][OG_PCOL]; }
};

struct RecWriter {
    ParseRec *rec;
    int nw, nl, ncoef = 0;
    int job = 0; // the job whose leaves are being written (2 x band + decode slot)
    OG_MEMBER void word(u32 w) {
        if (nw < REC_MAX_WORDS) rec->words[nw] = w;
        nw++;
    }
    OG_MEMBER int reserve() { return nw++; } // a slot to be filled in later by patch()
    OG_MEMBER void patch(int at, u32 w) {
        if (at < REC_MAX_WORDS) rec->words[at] = w;
    }
    OG_MEMBER void leaf(int x, int N, int K, int B, i32 gain, int off, u32 idx) {
        if (nl < REC_MAX_LEAVES) {
            const u32 geom = (u32)x | (u32)N << 11 | (u32)K << 19 | (u32)(B - 1) << 27;
            const u32 aux = (u32)(gain & 0xffff) | (u32)off << 16 | (u32)job << 20;
#ifdef OG_HOST_EMUL
            rec->leaf[nl].idx = idx; rec->leaf[nl].geom = geom; rec->leaf[nl].aux = aux; rec->leaf[nl].pad = 0;
#else
            typedef u32 u32x4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<u32x4 *>(&rec->leaf[nl]) = u32x4{idx, geom, aux, 0u};
#endif
        }
        nl++;
        ncoef += N;
    }
    // a band's four header words: on a multiple of four (up to three words skipped), one 16-byte store
    OG_MEMBER int band_begin() { return nw = (nw + 3) & ~3; }
    OG_MEMBER void words4(u32 w0, u32 w1, u32 w2, u32 w3) {
        if (nw + 4 <= REC_MAX_WORDS) {
#ifdef OG_HOST_EMUL
            rec->words[nw] = w0; rec->words[nw + 1] = w1; rec->words[nw + 2] = w2; rec->words[nw + 3] = w3;
#else
            typedef u32 u32x4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<u32x4 *>(&rec->words[nw]) = u32x4{w0, w1, w2, w3};
#endif
        }
        nw += 4;
    }
};

// isqrt32 (celt.cpp:3086) for arguments below 2^24, which a float holds exactly: the hardware's root is within one of the integer
// root, and two comparisons settle it.  (The reference's bit-by-bit loop runs as long as the wave's largest argument needs.)
// The root is below 4,096 there and a float's spacing at 4,096 is 2^-11, so any root good to a few units in the last place -- the
// correctly rounded one the compiler emits by default as much as a bare v_sqrt_f32 -- truncates to the integer root or to one
// beside it.  The CPU test walks all of 2^24 with the host's root; the only caller passes at most 8 x 129^2 + 1 = 133,129.
OG_DEV u32 isqrt24(u32 val) {
    u32 g = (u32)__builtin_sqrtf((float)val);
    g -= g * g > val;
    g += (g + 1) * (g + 1) <= val;
    return g;
}

// compute_theta (celt.cpp:1241) as the partition walk calls it -- mono, no fill mask -- for a lane of its own.  The angle has one
// of two models, uniform (ec_dec_uint) where the node still spans several short blocks and triangular where it does not, and a
// parse wave holds frames of both kinds at nearly every split: compute_theta's three decode / update pairs then run one after the
// other with a part of the lanes each.  Here a lane's model only chooses the total it decodes against and how the decoded value
// maps to (itheta, fl, fs): ONE division pair, one update and one renormalisation for the whole wave.
OG_DEV void split_theta_lane(RcLane &rc, int band, Split &sc, int N, i32 &b, int B0, int LM) {
    int itheta = 0;
    const int pulse_cap = RomLds::logn(band) + LM * (1 << BITRES);
    const int offset = (pulse_cap >> 1) - 4;
    const int qn = compute_qn(N, b, offset, pulse_cap, 0);
    const u32 tell = rc_tell_frac(rc);
    if (qn != 1) {
        const bool uni = B0 > 1;
        const int h = qn >> 1;
        const int ftb = uni ? OG_MAX(ilog((u32)qn) - 8, 0) : 0; // ec_dec_uint(qn + 1): raw bits below the eight range-coded ones
        const u32 ft = uni ? (u32)(qn >> ftb) + 1 : (u32)((h + 1) * (h + 1));
        const u32 fm = rc_decode(rc, ft);
        // the triangular model (celt.cpp:1290-1305): rising below the middle, falling above it.  (Lanes of the uniform model run
        // this arithmetic too and drop the result: with fm < ft <= 257 there every value stays small and every shift defined.)
        const bool low = fm < (u32)(h * (h + 1) >> 1);
        const u32 root = isqrt24(8 * (low ? fm : ft - fm - 1) + 1);
        const int it = low ? (int)((root - 1) >> 1) : (int)((2u * (u32)(qn + 1) - root) >> 1);
        const int fs_t = low ? it + 1 : qn + 1 - it;
        const u32 fl_t = low ? (u32)(it * (it + 1) >> 1) : ft - (u32)(fs_t * (fs_t + 1) >> 1);
        const u32 fl = uni ? fm : fl_t, fs = uni ? 1u : (u32)fs_t;
        rc_update(rc, fl, fl + fs, ft);
        itheta = uni ? (int)fm : it;
        if (ftb) {
            const u32 t = fm << ftb | rc_bits(rc, (unsigned)ftb);
            if (t > (u32)qn) rc.error = 1;
            itheta = (int)OG_MIN(t, (u32)qn);
        }
        itheta = (int)udiv((u32)(itheta * 16384), (u32)qn);
    }
    const int qalloc = (int)(rc_tell_frac(rc) - tell);
    b -= qalloc;
    int imid, iside, delta;
    if (itheta == 0) {
        imid = 32767;
        iside = 0;
        delta = -16384;
    } else if (itheta == 16384) {
        imid = 0;
        iside = 32767;
        delta = 16384;
    } else {
        imid = bitexact_cos(itheta);
        iside = bitexact_cos(16384 - itheta);
        delta = frac_mul16((N - 1) << 7, bitexact_log2tan(iside, imid));
    }
    sc.inv = 0;
    sc.imid = imid;
    sc.iside = iside;
    sc.delta = delta;
    sc.itheta = itheta;
    sc.qalloc = qalloc;
}

// quant_partition celt.cpp:1382, range-decoder half: split decisions, angles, pulse counts and PVQ indices.  The
// partition tree itself does not reach the record: the reconstruction only needs its LEAVES in decode order, each with
// what the tree implies for it -- position, size, gain, and how the band's fill / collapse masks map onto the leaf:
//   fill(leaf) = silent ? 0 : (fill(job) >> off) & ((1 << B) - 1)        cm(job) |= cm(leaf) << off
// (`off` sums B0 >> 1 over the splits whose side branch leads to the leaf; a split with angle 0 silences its side
// branch, one with angle 16384 its mid branch: compute_theta's fill masks, celt.cpp:1320-1353.)
// In the word stream a job is one header word (JW_*: how many leaves without pulses follow, which PVQ leaves are its
// own, whether it needs its folding source at all) followed by two words per non-silent leaf without pulses; leaves
// with pulses only exist in the leaf arrays.  Returns 1 when the job needs the folding source.
// `silent`: the whole job's fill mask is known to be empty (the mid of a stereo band split at angle 16384, the side of one
// split at angle 0 -- every band from the intensity band on: celt.cpp:1320-1353 clear that half of the mask), so none of
// its leaves without pulses is ever filled and none is recorded.
OG_DEV int parse_tree(RcLane &rc, RecWriter &out, int band, i32 &remaining_bits, int x, int N, i32 b, int B, int LM, i32 gain,
                      int has_low, int silent) {
    int depth = 0, off = 0, n_fill = 0;
    const int jpos = out.reserve(), first_pvq = out.nl;
    for (;;) {
        OG_MARK(41);
        for (;;) { // descend
            if (!(LM != -1 && b > pulse_cache_max<RomLds>(band, LM) + 12 && N > 2)) break;
            const int B0 = B;
            Split sc;
            N >>= 1;
            LM -= 1;
            B = (B + 1) >> 1;
            split_theta_lane(rc, band, sc, N, b, B0, LM);
            i32 delta = sc.delta;
            const int itheta = sc.itheta;
            if (B0 > 1 && (itheta & 0x3fff)) {
                if (itheta > 8192)
                    delta -= delta >> (4 - LM);
                else
                    delta = OG_MIN(0, delta + (N << BITRES >> (5 - LM)));
            }
            const i32 mbits = OG_MAX(0, OG_MIN(b, (b - delta) / 2));
            const i32 sbits = b - mbits;
            remaining_bits -= sc.qalloc;
            const int mid_first = mbits >= sbits;
            const int off_side = off + (B0 >> 1), silent_mid = silent | (itheta == 16384), silent_side = silent | (itheta == 0);
            const i32 gain_mid = tr16(mul16_p15(gain, sc.imid)), gain_side = tr16(mul16_p15(gain, sc.iside));
            // The frame holds the SECOND child as it will start (celt.cpp:1440-1461): where it lies, its mask offset, whether it is
            // silent, its gain, both children's bits and the budget as of now (for the rebalancing) -- and nothing of the split
            // itself: once the second child has started nothing is left to do here, so it takes the frame with it and the way
            // back from a leaf is ONE pop.  (The frames stayed until both children were done: a loop over the finished ones that
            // the wave ran as often as its deepest lane needed, every lane's LDS reads depending on the word before.)
            // Word 0 has no bit to spare: position < 2^11 (two channels of 960), half size N <= 88 of 8 bits, LM + 1 <= 3 of 3, blocks
            // B <= 16 of 5, mask offset <= 15 of 4 (it sums B0 >> 1 = 8 + 4 + 2 + 1 at most), silence.
#ifdef OG_HOST_EMUL
            if (x + N >= 2048 || N > 255 || LM + 1 > 7 || B > 31 || off_side > 15) __builtin_trap();
#endif
            i32 *F = &PL.u.stack[depth][0][OG_PCOL];
            F[0 * OG_PL_LANES] = (i32)((u32)(mid_first ? x + N : x) | (u32)N << 11 | (u32)(LM + 1) << 19 | (u32)B << 22 |
                                       (u32)(mid_first ? off_side : off) << 27 | (u32)(mid_first ? silent_side : silent_mid) << 31);
            F[1 * OG_PL_LANES] = mid_first ? mbits : sbits;
            F[2 * OG_PL_LANES] = mid_first ? sbits : mbits;
            F[3 * OG_PL_LANES] = remaining_bits;
            // (the side gets nothing back when the angle is 0, the mid nothing when it is 16384)
            F[4 * OG_PL_LANES] = ((mid_first ? gain_side : gain_mid) & 0xffff) | (itheta != (mid_first ? 0 : 16384)) << 16;
            depth++;
            if (mid_first) {
                b = mbits;
                gain = gain_mid;
                silent = silent_mid;
            } else {
                x += N;
                b = sbits;
                gain = gain_side;
                off = off_side;
                silent = silent_side;
            }
        }
        { // leaf: pulse count from the remaining budget, then the codeword index (celt.cpp:1463-1480)
            OG_MARK(42);
            int q = bits2pulses<RomLds>(band, LM, b), curr_bits = pulses2bits<RomLds>(band, LM, q);
            remaining_bits -= curr_bits;
            while (remaining_bits < 0 && q > 0) {
                remaining_bits += curr_bits;
                q--;
                curr_bits = pulses2bits<RomLds>(band, LM, q);
                remaining_bits -= curr_bits;
            }
            const int K = q ? get_pulses(q) : 0;
            OG_MARK(43);
            if (K) // V(N, K) = U(N, K) + U(N, K + 1) (celt.cpp:2622), found next to the cache entry that gave q
                out.leaf(x, N, K, B, gain, off, rc_uint(rc, PT.pulse_v[pulse_cache<RomLds>(band, LM) + q]));
            else if (!silent) { // (a silent leaf stays zero, as the spectrum was initialised: nothing to record)
                out.word((u32)off << LW_OFF_SHIFT | (u32)(B - 1) << LW_B_SHIFT | (u32)N << LW_N_SHIFT);
                out.word((u32)x | (u32)(gain & 0xffff) << 11);
                n_fill++;
            }
        }
        OG_MARK(44);
        if (depth == 0) break;
        { // on to the innermost split's second child, with what the first one left of its bits (celt.cpp:1446-1461)
            depth--;
            const i32 *F = &PL.u.stack[depth][0][OG_PCOL];
            const u32 w0 = (u32)F[0];
            const i32 w4 = F[4 * OG_PL_LANES];
            const i32 rebalance = F[1 * OG_PL_LANES] - (F[3 * OG_PL_LANES] - remaining_bits);
            b = F[2 * OG_PL_LANES] + ((rebalance > 3 << BITRES && (w4 >> 16)) ? rebalance - (3 << BITRES) : 0);
            x = (int)(w0 & 2047);
            N = (int)(w0 >> 11) & 255;
            LM = (int)((w0 >> 19) & 7) - 1;
            B = (int)(w0 >> 22) & 31;
            off = (int)(w0 >> 27) & 15;
            silent = (int)(w0 >> 31);
            gain = (i32)(i16)w4;
        }
    }
    OG_MARK(40);
    const int need_low = has_low && n_fill > 0;
    out.patch(jpos, (u32)n_fill | (u32)(out.nl - first_pvq) << JW_NPVQ_SHIFT | (u32)first_pvq << JW_FIRST_SHIFT | (need_low ? JW_NEED_LOW : 0));
    return need_low;
}

// quant_all_bands celt.cpp:1754: the range-decoder half, plus everything else about a band that is known without the
// decoded spectrum (folding source and mask range, stereo gains, the folding-history scale).
// Returns the set of bands (bit i = band i) whose folding history some later band actually reads.
OG_DEV u32 parse_all_bands(RcLane &rc, RecWriter &out, int start, int end, int C, int N_ch, int shortBlocks, int spread,
                           int dual_stereo, int intensity, i32 total_bits, i32 balance, int LM, int codedBands, int disable_inv) {
    const LaneArr a{out.rec->work_pulses, nullptr, nullptr}; // (pulses and tf_res only: the band energies rest in the record while the bands are parsed)
    const int M = 1 << LM, B = shortBlocks ? M : 1;
    const int norm_offset = M * RomLds::eband(start);
    int lowband_offset = 0, update_lowband = 1;
    u32 need_norm = 0;
    // the bands' bits from the record (LaneArr::pulses_rest), FOUR bands per 16-byte load, requested four bands ahead: one load per
    // band went to HBM every time -- the record's line does not survive in the L2 from one band to the next (21 read requests and
    // 2.7 KB of traffic per frame, round 5's counters)
#ifdef OG_HOST_EMUL
    i32 p4[4] = {0, 0, 0, 0}, n4[4] = {0, 0, 0, 0};
    auto fetch4 = [&](int b, i32 *o) { for (int k = 0; k < 4; k++) o[k] = b + k < NBANDS ? a.pulses(b + k) : 0; };
    fetch4(start & ~3, n4);
#else
    typedef i32 i32x4p __attribute__((ext_vector_type(4)));
    i32x4p p4 = {0, 0, 0, 0}, n4 = *reinterpret_cast<const i32x4p *>(&a.pulses(start & ~3)); // (work_pulses is padded to 32 words)
#endif
    for (int i = start; i < end; i++) {
        if (i == start || (i & 3) == 0) {
#ifdef OG_HOST_EMUL
            for (int k = 0; k < 4; k++) p4[k] = n4[k];
            fetch4((i & ~3) + 4, n4);
#else
            p4 = n4;
            n4 = *reinterpret_cast<const i32x4p *>(&a.pulses((i & ~3) + 4));
#endif
        }
        const i32 pulses_i = (i & 3) == 0 ? p4[0] : (i & 3) == 1 ? p4[1] : (i & 3) == 2 ? p4[2] : p4[3];
        const int eb0 = M * RomLds::eband(i), N = M * RomLds::eband(i + 1) - eb0;
        const int x = eb0, y = C == 2 ? N_ch + eb0 : -1;
        out.rec->band_w[i] = (u16)OG_MIN(out.band_begin(), REC_MAX_WORDS);
        const i32 tell = (i32)rc_tell_frac(rc);
        if (i != start) balance -= tell;
        i32 remaining_bits = total_bits - tell - 1, b;
        if (i <= codedBands - 1) {
            const i32 curr_balance = balance / OG_MIN(3, codedBands - i);
            b = OG_MAX(0, OG_MIN(16383, OG_MIN(remaining_bits + 1, pulses_i + curr_balance)));
        } else
            b = 0;
        const int tf_change = a.tf_res(i);
        // ---- folding source (celt.cpp:1812-1850): offsets into the folding history and the bands whose collapse
        //      masks feed this band's fill mask
        if ((eb0 - N >= M * RomLds::eband(start) || i == start + 1) && (update_lowband || lowband_offset == 0)) lowband_offset = i;
        u32 w0 = (u32)(tf_change + 4) << BW_TF_SHIFT, w1 = (u32)eb0 << 11 | (u32)N << 22;
        int has_low = 0;
        u32 fold_bands = 0; // the bands the folding source overlaps
        if (lowband_offset != 0 && (spread != 3 || B > 1 || tf_change < 0)) {
            const int effective_lowband = OG_MAX(0, M * RomLds::eband(lowband_offset) - norm_offset - N);
            int fold_start = lowband_offset;
            while (M * RomLds::eband(--fold_start) > effective_lowband + norm_offset) {}
            int fold_end = lowband_offset - 1;
            while (++fold_end < i && M * RomLds::eband(fold_end) < effective_lowband + norm_offset + N) {}
            w0 |= BW_HAS_LOW | (u32)fold_start << BW_FOLD0_SHIFT | (u32)fold_end << BW_FOLD1_SHIFT;
            w1 |= (u32)effective_lowband;
            has_low = 1;
            fold_bands = (1u << fold_end) - (1u << fold_start);
        }
        if (dual_stereo) w0 |= BW_DUAL_PRE;
        if (dual_stereo && i == intensity) {
            dual_stereo = 0;
            w0 |= BW_DUAL_END;
        }
        if (dual_stereo) w0 |= BW_DUAL;
        u32 w2 = 0;
        if (N == 1) { // quant_band_n1 celt.cpp:1357
            for (int c = 0; c < (y >= 0 ? 2 : 1); c++) {
                if (remaining_bits >= 1 << BITRES) {
                    if (rc_bits(rc, 1)) w0 |= c ? BW_SIGN1 : BW_SIGN0;
                    remaining_bits -= 1 << BITRES;
                }
            }
            out.words4(w0, w1, 0, 0);
        } else {
            const int stereo = (y >= 0) && !dual_stereo;
            Split sc;
            sc.inv = 0; sc.imid = 0; sc.iside = 0; sc.delta = 0; sc.itheta = 0; sc.qalloc = 0;
            i32 bb = b, fill_unused = 0, mbits = 0, sbits = 0, rebal0 = 0;
            int n2case = 0, swap_c = 0, mid_first = 1, njobs = 1;
            if (stereo) { // quant_band_stereo celt.cpp:1628
                compute_theta<RomLds>(rc, i, intensity, disable_inv, remaining_bits, sc, N, bb, B, B, LM, 1, fill_unused);
                w0 |= BW_STEREO;
                if (sc.itheta == 0) w0 |= BW_THETA0;
                if (sc.itheta == 16384) w0 |= BW_THETA1;
                if (sc.itheta > 8192) w0 |= BW_SWAP;
                if (sc.inv) w0 |= BW_INV;
                w2 = (u32)(sc.imid & 0xffff) | (u32)sc.iside << 16;
                if (N == 2) {
                    n2case = 1;
                    mbits = bb;
                    sbits = 0;
                    if (sc.itheta != 0 && sc.itheta != 16384) sbits = 1 << BITRES;
                    mbits -= sbits;
                    swap_c = sc.itheta > 8192;
                    remaining_bits -= sc.qalloc + sbits;
                    if (sbits && rc_bits(rc, 1)) w0 |= BW_SIGN;
                } else {
                    mbits = OG_MAX(0, OG_MIN(bb, (bb - sc.delta) / 2));
                    sbits = bb - mbits;
                    remaining_bits -= sc.qalloc;
                    rebal0 = remaining_bits;
                    mid_first = mbits >= sbits;
                    njobs = 2;
                }
            } else if (dual_stereo)
                njobs = 2;
            if (mid_first) w0 |= BW_MID_FIRST;
            out.words4(w0, w1, w2, (u32)(u16)tr16(celt_sqrt(shl32(N, 22)))); // (w3: scale of the folding history, celt.cpp:1617)
            for (int jb = 0; jb < njobs; jb++) {
                int jx, jlow = has_low, jsilent = 0;
                i32 jbits, jgain = 32767;
                if (dual_stereo) {
                    jx = jb ? y : x;
                    jbits = b / 2;
                } else if (!stereo) {
                    jx = x;
                    jbits = b;
                } else if (n2case) {
                    jx = swap_c ? y : x;
                    jbits = mbits;
                } else {
                    const int is_mid = (jb == 0) == (mid_first != 0);
                    if (jb == 1) { // rebalance between the two halves (celt.cpp:1711-1724)
                        const i32 rebalance = (mid_first ? mbits : sbits) - (rebal0 - remaining_bits);
                        if (mid_first) {
                            if (rebalance > 3 << BITRES && sc.itheta != 0) sbits += rebalance - (3 << BITRES);
                        } else {
                            if (rebalance > 3 << BITRES && sc.itheta != 16384) mbits += rebalance - (3 << BITRES);
                        }
                    }
                    jx = is_mid ? x : y;
                    jbits = is_mid ? mbits : sbits;
                    jsilent = is_mid ? sc.itheta == 16384 : sc.itheta == 0;
                    if (!is_mid) {
                        jgain = sc.iside;
                        jlow = 0; // the side never folds (celt.cpp:1709)
                    }
                }
                // quant_band celt.cpp:1526: only the block count reaches the partition walk's decisions
                int Bj = B, N_B = (int)udiv((u32)N, (u32)B), tfc = tf_change;
                const int recombine = tfc > 0 ? tfc : 0;
                Bj >>= recombine;
                N_B <<= recombine;
                while ((N_B & 1) == 0 && tfc < 0) {
                    Bj <<= 1;
                    N_B >>= 1;
                    tfc++;
                }
                out.job = 2 * i + jb;
                if (parse_tree(rc, out, i, remaining_bits, jx, N, jbits, Bj, LM, jgain, jlow, jsilent)) need_norm |= fold_bands;
            }
        }
        balance += pulses_i + tell;
        update_lowband = b > (N << BITRES);
    }
    return need_norm;
}

// One CELT-only frame, lane-private.  `payload`/`len`: the frame's bytes; `ch`: channels coded in the packet,
// CC: decoder channels.  Mirrors decode_frame_wave + celt_decode_frame up to (not including) every vector operation.
// `handoff` (hybrid frames): resume the range decoder where the SILK half left it and start at band 17.
// The stream's band energies (CeltState::bandE) are carried from frame to frame HERE, not by the reconstruction: they are the only
// stream state this half reads, so the parse of a stream's next frame depends on nothing but the parse of this one and may run
// while this frame is still being reconstructed (opusgpu_set_pipeline, og_api.hip).
OG_DEV void celt_parse_lane(StreamState *st, const u8 *payload, int len, int ch, ParseRec *rec, const SilkHandoff *handoff) {
    const LaneArr a{rec->work_pulses, rec->bandE, rec->pulses};
    const int CC = st->channels, C = ch, LM = 3, frame_size = 960, start = handoff ? 17 : 0, end = NBANDS;
    rec->start = start;
    rec->n_leaves = 0;
    rec->n_words = 0;
    if (len < 0 || len > 1275 || (handoff && !handoff->valid)) {
        rec->ret = BAD_ARG;
        rec->flags = RF_SKIP;
        return;
    }
    RcLane rc;
    rc_lane_attach(rc, payload, (u32)len);
    if (handoff) {
        rc.storage = handoff->storage; rc.end_offs = handoff->end_offs; rc.end_window = handoff->end_window;
        rc.nend_bits = handoff->nend_bits; rc.nbits_total = handoff->nbits_total; rc.offs = handoff->offs; rc.rng = handoff->rng;
        rc.val = handoff->val; rc.ext = handoff->ext; rc.rem = handoff->rem; rc.error = handoff->error;
        rc_lane_resume(rc);
    } else
        rc_init(rc, (u32)len);
    if (rc.storage <= 1) { // celt_decode_frame's early exit (celt.cpp:2225)
        rec->ret = CELT_BAD_ARG;
        rec->flags = RF_BAD_CELT;
        rec->rng_final = rc.rng;
        return;
    }
    const int disable_inv = CC == 1;
    for (int i = 0; i < 2 * NBANDS; i++) a.bandE(i) = st->celt.bandE[i];
    if (C == 1)
        for (int i = 0; i < NBANDS; i++) a.bandE(i) = (i16)OG_MAX((i32)a.bandE(i), (i32)a.bandE(NBANDS + i));
    for (int i = 0; i < NBANDS; i++) { // (this also clears the dynalloc boosts, which rest in fine_quant: LaneArr::boost;
                                       // the bits per band outside start .. end where they leave the allocation scratch: pulses_rest)
        a.fine_quant(i) = 0;
        a.fine_prio(i) = 0;
    }
    CeltHeader h;
    OG_MARK(20);
    celt_parse_header(a, rc, start, end, C, LM, h);
    a.energies_rest(); // the partition walk's stack takes their place
    RecWriter out;
    out.rec = rec;
    out.nw = 0;
    out.nl = 0;
    const int M = 1 << LM, N = M * 120;
    // tf_res and pulses are needed by the reconstruction (pulses_rest wrote those; they change meaning nowhere after the header)
    for (int i = 0; i < NBANDS; i++) rec->tf_res[i] = a.tf_res(i);
    OG_MARK(26);
    rec->need_norm = parse_all_bands(rc, out, start, end, C, N, h.transient ? M : 0, h.spread, h.dual_stereo, h.intensity,
                                     (i32)rc.storage * (8 << BITRES) - h.anti_collapse_rsv, h.balance, LM, h.codedBands, disable_inv);
    OG_MARK(27);
    int anti_collapse_on = 0;
    if (h.anti_collapse_rsv > 0) anti_collapse_on = (int)rc_bits(rc, 1);
    a.energies_back();
    energy_finalise(a, rc, start, end, (i32)rc.storage * 8 - rc_tell(rc), C);
    for (int i = 0; i < 2 * NBANDS; i++) rec->bandE[i] = a.bandE(i);
    u32 flags = (u32)LM << RF_LM_SHIFT | (u32)h.spread << RF_SPREAD_SHIFT;
    if (h.silence) flags |= RF_SILENCE;
    if (h.transient) flags |= RF_TRANSIENT;
    if (C == 2) flags |= RF_STEREO;
    if (h.dual_stereo) flags |= RF_DUAL;
    if (anti_collapse_on) flags |= RF_ANTI_COLLAPSE;
    if (rc.error || out.nw > REC_MAX_WORDS || out.nl > REC_MAX_LEAVES) flags |= RF_RC_ERROR;
    if (rc_tell(rc) > 8 * (i32)rc.storage) flags |= RF_TELL_OVERFLOW;
    rec->flags = flags;
    rec->ret = frame_size;
    rec->rng_final = rc.rng;
    rec->intensity = h.intensity;
    rec->pf_pitch = h.pf_pitch;
    rec->pf_gain = h.pf_gain;
    rec->pf_tapset = h.pf_tapset;
    rec->n_leaves = OG_MIN(out.nl, REC_MAX_LEAVES);
    rec->n_coef = out.ncoef;
    rec->n_words = OG_MIN(out.nw, REC_MAX_WORDS);
    // the energies the next frame predicts from, as celt_synthesis leaves them (celt.cpp:2404-2436): -28 dB in a silent frame,
    // a mono frame's in both channels, zero outside start .. end.  Two bands per store.
    for (int i = 0; i < 2 * NBANDS; i += 2) {
        i32 e[2];
        for (int k = 0; k < 2; k++) {
            const int band = i + k >= NBANDS ? i + k - NBANDS : i + k;
            e[k] = h.silence ? -28 * 1024 : (i32)a.bandE(C == 1 ? band : i + k);
            if (band < start || band >= end) e[k] = 0;
        }
        *reinterpret_cast<u32 *>(&st->celt.bandE[i]) = (u32)(u16)e[0] | (u32)(u16)e[1] << 16;
    }
}

} // namespace og
