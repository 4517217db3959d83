// og_celt_rec.hpp -- the records the kernels of the split CELT path hand each other (ParseRec, SilkHandoff, ReconOut) and the layout
// of their words; nothing here executes a stage.  The stages: og_celt_parse.hpp (k_celt_parse), og_celt_recon.hpp with
// og_celt_recon_pm.hpp (k_celt_recon, k_celt_recon_fb: og_recon.hip), and k_celt_post (og_api.hip).
//
// The split CELT path: entropy decoding with ONE FRAME PER LANE, then vector reconstruction with
// one frame per wave, then de-emphasis with one (frame, channel) per lane.
//
// Why: everything the range decoder touches is a serial dependency chain over wave-uniform values.  Run one frame
// per wave it occupies a whole 64-lane SIMD for scalar work (measured on the single-kernel path: ~140 k vector +
// ~43 k scalar instructions per frame, half of them walking the PVQ codebook).  None of that work depends on the
// decoded spectrum: the bits a CELT frame reads are fully determined by the bit budget bookkeeping, never by the
// pulse vectors, collapse masks or the noise seed (src/celt.cpp:1382-1741: `fill`, `cm` and `seed` only steer the
// folding).  So the frame splits cleanly:
//
//   parse  (k_celt_parse, one frame per LANE, 64 frames per wave): header, energies, allocation, the band loop's
//          budget logic, split angles and PVQ codeword indices -- and every other wave-uniform quantity of the band
//          loop that does not depend on decoded data (folding offsets, gains, scale factors).  Output: a ParseRec
//          per frame in HBM: a header, a word stream in decode order (4 words per band, 1 per split / leaf) and an
//          array of PVQ leaves (index, position, N, K, blocks, gain).
//   recon  (k_celt_recon, one frame per WAVE): all PVQ leaves of the frame at once, one leaf per lane (index ->
//          pulses -> scaled, de-rotated coefficients + collapse mask: serial per leaf, independent across leaves);
//          then the band loop's vector half (folding / noise fill, Haar / Hadamard, stereo merge, collapse-mask
//          bookkeeping, anti-collapse) interpreting the word stream; then the synthesis half (og_celt.hpp).
//   post   (k_celt_post, one (frame, channel) per lane): the de-emphasis IIR (rounding => serial) and int16 PCM.
//
// All halves restate the same reference functions as og_celt_bands.hpp (file:line cited there); the single-kernel
// path remains for frames whose CELT part follows SILK data in the same range coder (hybrid) and for the SILK-only
// transition frame (Q4).
#pragma once
#include <stddef.h>
#include "og_state.hpp"

namespace og {

// ---- the record ------------------------------------------------------------------------------------
constexpr int REC_BAND_WORDS = 4;
constexpr int REC_MAX_LEAVES = NBANDS * 2 * 16;                   // <= 16 leaves per band and channel (4 split levels)
constexpr int REC_MAX_WORDS = NBANDS * (REC_BAND_WORDS + 2 * 33) + 3 * NBANDS + 1; // band words + per job: header + <= 16 leaves x 2 words (+ up to 3 words of padding before a band's header)

enum { // ParseRec.flags
    RF_SILENCE = 1, RF_TRANSIENT = 2, RF_LM_SHIFT = 2 /* 2 bits */, RF_STEREO = 16, RF_SPREAD_SHIFT = 5 /* 2 bits */,
    RF_DUAL = 128, RF_ANTI_COLLAPSE = 256, RF_RC_ERROR = 512, RF_TELL_OVERFLOW = 1024,
    RF_SKIP = 2048,    // descriptor rejected before any state change (decode_frame_wave's BAD_ARG), or (hybrid) the
                       // single-kernel path already reported the frame's error: nothing to do, result untouched
    RF_BAD_CELT = 4096 // celt_decode_frame's early CELT_BAD_ARG: bookkeeping only
};
// Band words.  W0: flags below; W1: eff_low | x << 11 | N << 22 (positions relative to their arena rows);
// W2: imid | iside << 16 (stereo split gains, Q15); W3: lowband_out scale sqrt(N) (Q?) in the low 16 bits.
enum {
    BW_SIGN0 = 1, BW_SIGN1 = 2, BW_INV = 4, BW_SIGN = 8, BW_MID_FIRST = 16, BW_SWAP = 32,
    BW_THETA0 = 64, BW_THETA1 = 128,   // the stereo angle is exactly 0 / exactly 16384 (fill mask halves)
    BW_TF_SHIFT = 8 /* tf_change + 4, 3 bits */, BW_FOLD0_SHIFT = 11 /* 5 bits */, BW_FOLD1_SHIFT = 16 /* 5 bits */,
    BW_HAS_LOW = 1 << 21, BW_DUAL = 1 << 22, BW_DUAL_END = 1 << 23, BW_STEREO = 1 << 24,
    BW_DUAL_PRE = 1 << 25 // dual stereo still on when the band starts (before a switch-off at the intensity band)
};
// Job words (a "job" = one band of one channel, or the mid / side part of a stereo band).  Header: number of leaves
// without pulses that follow | number of PVQ leaves << 5 | index of its first PVQ leaf << 10 | JW_NEED_LOW.  Then,
// per (non-silent) leaf without pulses, in decode order: L0 = off | B-1 | N (LW_* shifts), L1 = x | gain << 11.
enum {
    JW_NPVQ_SHIFT = 5 /* 5 bits */, JW_FIRST_SHIFT = 10 /* 10 bits */, JW_NEED_LOW = 1 << 20,
    LW_OFF_SHIFT = 8 /* 4 bits */, LW_B_SHIFT = 12 /* 4 bits */, LW_N_SHIFT = 16 /* 8 bits */
};

// Hybrid frames: the single-kernel path decodes the SILK half (wave per frame), then hands the live range decoder and
// the SILK PCM over to the split path, which decodes the CELT half (bands 17..20) and mixes the two in k_celt_post.
struct SilkHandoff {
    // SILK output at 48 kHz, interleaved over the packet's channels; first and on a line boundary of the memory system: the
    // synthesis kernel writes it and k_celt_post reads it in 128-byte pieces (at offset 48 of a 3,888-byte record every piece was two lines)
    alignas(128) i16 pcm[1920];
    u32 valid; // 1: SILK half decoded, coder state below is live
    u32 storage, end_offs, end_window;
    i32 nend_bits, nbits_total;
    u32 offs, rng, val, ext;
    i32 rem, error;
};
static_assert(sizeof(SilkHandoff) % 128 == 0 && offsetof(SilkHandoff, pcm) == 0, "handoff alignment");

struct ParseRec {
    i32 ret;       // samples per channel (960) -- or the negative code the frame ends with
    u32 rng_final; // range decoder's rng after the frame
    u32 flags;
    i32 intensity, pf_pitch, pf_gain, pf_tapset, start;
    i32 n_leaves, n_words;
    u32 need_norm; // bands whose folding history is read by a later band
    i32 n_coef;    // coefficients in PVQ leaves (the sum of their N)
    i32 reserved[4];
    i16 bandE[2 * NBANDS]; // final band energies (coarse + fine + finalise)
    i16 pulses[NBANDS];
    u16 band_w[NBANDS];    // where each band's four header words start in words[] (its job words follow them)
    i8 tf_res[NBANDS];
    i8 pad[256 - 64 - 4 * NBANDS - 2 * NBANDS - 2 * NBANDS - NBANDS];
    // A PVQ leaf is 16 bytes -- written by the parse lane with ONE store and fetched by the reconstruction's lane with one load
    // (round 3 kept three arrays of words: three scattered 4-byte stores per leaf from every lane, each into a record of its own).
    struct Leaf {
        u32 idx;  // PVQ codeword index
        u32 geom; // x | N << 11 | K << 19 | (B - 1) << 27   (x: offset into S.v[V_X..])
        u32 aux;  // gain (product of the split gains above the leaf, Q15) | mask offset << 16 (4 bits) | the leaf's job << 20
                  // (2 x band + decode slot: whose collapse mask the leaf's mask goes into, S.job_mask_row())
        u32 pad;
    } leaf[REC_MAX_LEAVES];
    u32 words[(REC_MAX_WORDS + 64) / 64 * 64]; // read in windows of 64 (REC_WORDS_CAP); a band's four header words start on a multiple of four
    // the parse lane's bits per band (32 bits: see ParseLds) from the end of its allocation on -- written once (LaneArr::pulses_rest,
    // 16-byte stores: the pad below is written too), read once per band by the band walk.  (Round 4 measured the array here for the
    // allocation's passes as well: 2.9 KB more HBM traffic per frame; those passes work in LDS, on the words of the two vectors.)
    i32 work_pulses[NBANDS];
    i32 work_pad[32 - NBANDS];
};
static_assert(offsetof(ParseRec, leaf) % 16 == 0 && offsetof(ParseRec, words) % 16 == 0 && offsetof(ParseRec, work_pulses) % 16 == 0 &&
              offsetof(ParseRec, work_pad) == offsetof(ParseRec, work_pulses) + 4 * NBANDS && NBANDS + 3 <= 32, "16-byte stores into the record");
static_assert(sizeof(ParseRec) % 16 == 0, "record alignment");

constexpr int FAST_MAX_LEAVES = 416; // (og_state.hpp: the most a 20 ms frame can have)

// What a reconstruction kernel reports per frame, read by the de-emphasis kernel (k_celt_post), which passes `ret` on to the
// caller's result array: the frame's result code and where in the stream's history ring its first sample went.  (The ring
// position is taken from here, not from the stream state: in pipelined steps the next step's reconstruction may already have
// advanced it when this step's de-emphasis runs.)
struct ReconOut {
    i32 ret, pos;
};

} // namespace og
