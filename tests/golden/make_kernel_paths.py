#!/usr/bin/env python3
"""Regenerates tests/golden/kernel_paths.json: directed packets for the branch sides of the KERNEL source (in host emulation) that
nothing the suite decodes takes.  CPU only, deterministic for a seed.

    python tests/golden/make_kernel_paths.py [--seed N] [--rounds N] [--batch N] [--baseline]

The coverage-guided search of tests/golden/make_rare_paths.py pointed at tools/kernel_branches.py: the frame writers of
tests/rc_craft.py pin a frame's leading symbols, random bytes fill the rest, the tool says which sides of the baseline list a batch
of candidate sequences took; a sequence that takes a side nothing before it took is found by bisection, shrunk (packets dropped
from the front while the side stays taken) and kept.  A sequence is one stream's packets from a fresh decoder, at most 8; in RFC
mode an empty packet is a loss and "fec" lists the packets before which decode_fec is asked for.  The tool compares every
candidate with the oracle on every entry point while it decodes; a candidate that differs stops the search and is printed: it is
a bug to fix, not a corpus entry.

The baseline list (the tool's report for everything the suite already decodes, kernel_branches.baseline_sequences) is kept in the
fixture; --baseline measures it again (minutes), otherwise the one in the existing fixture is reused.  Every side of it ends up
in exactly one of "reached" (named by an entry's keys), "emulation" (EMULATION below: the side exists only because a wave is one
lane here; the reason names the device form and the GPU test that runs it), "unreachable" (UNREACHABLE: the invariant) or "open"
(with what was tried).  Functions never entered are listed under "never_entered" with a reason of the same kinds.
"""
import argparse
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_branches as kb  # noqa: E402
import make_rare_paths as mrp  # noqa: E402
import rc_craft as rcc  # noqa: E402

OUT = os.path.join(HERE, "kernel_paths.json")

# (substring of the key -- or a tuple of substrings that must all occur --, reason).  The first match counts.
# ---- why a side is not the corpus's to take ---------------------------------------------------------------------------------------
G_SYNTH = "tests/test_gpu_synth_stages.py and tests/test_gpu_transient_frames.py run the device form against the oracle"
G_FORMS = "tests/test_gpu_device_forms.py with tests/gpu_kat runs the device form against known answers"
G_RFC = "tests/test_gpu_rfc.py (test_rfc_celt_loss_bursts_pitch_then_noise, test_rfc_loss_path) runs the device form against the oracle"
E_IMDCT = ("a wave is one lane here, so a block takes N4 passes and every pass is in range; on the device the 64 lanes take the 60 butterflies of a "
           "short block in ONE pass (ppb == 1) and the lanes at or past N4, and the passes past the last block, idle.  " + G_SYNTH)
E_NLANES = ("a reduction over the wave's lanes (OG_NLANES partial results): with one lane the loop over the other lanes never runs and no two "
            "partial results ever tie.  On the device 64 lanes scan lags side by side.  " + G_RFC)
E_GROUPS = ("the wave walks its items in strides of OG_NLANES and the lanes past the last item idle; with one lane every pass has an item.  "
            "tests/test_gpu_fill_windows.py and tests/test_gpu_transient_frames.py run the device form (k_celt_recon_fb) against the oracle")
E_PRE = ("the 20 ms kernel (og_recon.hip) fetches a frame's first record words, leaves and energies ahead of their use and passes them in (pre, "
         "bw_staged, booked); the emulation's celt_recon_wave passes none.  tests/test_gpu_celt.py, tests/test_gpu_fill_windows.py and "
         "tests/test_gpu_bench_shapes.py run that kernel against the oracle")
E_DEFER = ("the deferred rotation is the device form of the 20 ms kernel's leaf pass (og_recon.hip: pvq_leaf_lane describes the rotation, "
           "pvq_rotate_wave does it with the whole wave); the emulation rotates in the leaf.  " + G_FORMS + " (og_gpu_kat_tight.hip)")
E_HOSTPCM = ("a block under #if OG_HOST_EMUL: the emulation's de-emphasis writes PCM through a pointer that celt_post leaves null for a frame that "
             "failed, and no frame with a synthesis fails (see the tell-overflow reason); the device form stores unconditionally.  "
             "tests/test_gpu_celt.py runs it against the oracle")
EMULATION = [
    ("|imdct_channel|", E_IMDCT),
    ("|plc_shift_for|for (int t = 1; t < OG_NLANES", E_NLANES), ("|plc_search|if (LB.part[0][t] >= 0 && plc_better", E_NLANES),
    ("|plc_better|", E_NLANES),
    ("|pm_tf_undo|if (g < 2 * PM_GROUPS)", E_GROUPS),
    (("og_celt_recon_pm.hpp|anti_collapse_pm|", "e < NE", "|b1"), E_GROUPS),
    ("|recon_leaves_own|", E_PRE), ("|recon_begin|if (rx.pre", E_PRE), ("|recon_finish|if (rx.pre)", E_PRE),
    ("|recon_finish|if (!rx.booked)", E_PRE), ("|pm_setup_jobs|const int bw = !coded", E_PRE),
    ("|pvq_leaf_lane|if (defer)", E_DEFER),
    ("|celt_post4|if (pcm)", E_HOSTPCM),
]

R_FRAMING = ("every frame comes out of the packet layer (og_packet.hpp / opus_packet_parse, tests/test_host_framing.py): a frame of more than 1275 "
             "bytes is an invalid packet before a descriptor exists, and a length is never negative")
R_FSIZE = ("the frame size is 120 << LM for the LM the TOC names (RFC mode: og_packet.hpp; reference mode: always 960, or 120 for the 2.5 ms frame "
           "behind a hybrid one), so the loop always leaves through its break with LM <= 3")
R_STORAGE = ("celt_decode_frame is called with 2 <= storage <= 1275: a frame of at most one byte is concealed (decode_frame_rfc: len <= 1) or answered "
             "by the early CELT_BAD_ARG of the split path, the packet layer caps a frame at 1275 bytes; the silence frame of the hybrid fade-out is 2 bytes")
R_TELL = ("every symbol is read behind a check that its worst case fits what is left (flags, post-filter 16 bits, coarse energy 15 / 2 / 1, tf, "
          "spread, dynalloc, trim; the allocation hands out at most the bits left; quant_band_n1, fine energy and the final bits count theirs "
          "down), and a frame that starts past its budget is made silent with tell set to exactly 8 * storage: tell never passes the budget "
          "(the oracle's twin side: tests/golden/rare_paths.json)")
R_CELT_RET = ("the CELT layer never fails here: celt_decode_frame's three error returns (frame size, storage, tell overflow) and celt_conceal's "
              "BAD_ARG are unreachable -- the frame size is 120 << LM, the storage 2 .. 1275 bytes, the tell never passes the budget -- so celt_ret "
              "is the frame size and no error is passed on")
R_SILK_RET = ("silk_decode_packet fails only for a sampling rate other than 8 / 12 / 16 kHz, and internal_hz is 8000, 12000 or 16000 from the "
              "TOC's bandwidth (a concealment: the rate of the last frame); the concealment chunks pass the same errors on, so none arrives")
R_LIMITS = ("the record's limits cannot be exceeded: celt_parse_lane parses at LM 3, where a band of width w splits at most min(4, "
            "log2(8 w) - 1) times, so a job has at most 16 leaves, a frame at most FAST_MAX_LEAVES = 416 <= REC_MAX_LEAVES and at most 1021 words "
            "< REC_MAX_WORDS, whatever its bytes (tests/test_kernel_paths.py test_no_frame_exceeds_the_record_limits derives the counts from "
            "the band table in the ROM and reads the three constants from og_celt_rec.hpp)")
R_LM3 = ("celt_parse_lane decodes 20 ms frames only (LM = 3 is a constant there, written to every record's flags): the split path is "
         "reference mode's, where every frame is 20 ms")
R_NOT_FAST = ("the general band walk runs for a frame with leaves whose record is not fast, i.e. LM != 3 or a record past its limits; "
              "celt_parse_lane writes LM 3 and cannot exceed the limits (test_no_frame_exceeds_the_record_limits), so every frame with leaves "
              "takes the phase-major loop; recon_all_bands is the only caller that passes a folding scratch or a lowband_out")
R_REST_FILTER = ("k_celt_recon in its role RECON_REST_ONLY calls celt_recon_wave only for the frames its lanes find not fast, by recon_fast_eligible's "
                 "conditions written out on the record's words (og_api.hip; tests/test_kernel_paths.py "
                 "test_the_rest_kernels_lane_filter_is_recon_fast_eligible holds the two texts together), so a fast frame never arrives in that role")
R_SKIP = ("RF_SKIP marks a frame over 1275 bytes or a hybrid frame whose SILK half failed: the packet layer caps a frame at 1275 bytes and the SILK "
          "half fails only for an impossible sampling rate, so celt_parse_lane never writes the flag")
R_TRAP = "the five conditions of a __builtin_trap() that guards the bit fields of the partition stack in host emulation: none may ever hold"
R_20MS = ("the lane-per-frame SILK parse (og_silk_parse.hpp) is reference mode's: every SILK frame decodes as 20 ms there (one internal frame of "
          "four subframes, independently coded: condCoding 0, the lag coded absolutely, frame_length = 20 * fs_kHz a multiple of 16); RFC mode's "
          "10 / 40 / 60 ms frames go through silk_decode_packet's own entropy half, where the baseline takes these sides")
R_RATE = ("internal_hz is 8000 / 12000 / 16000 from the TOC's bandwidth, or (concealment) the channel's own rate, which was one of the three "
          "when it was set: the last comparison of the chain is never reached with another value")
R_REC = ("a record is handed only to the REC_ONLY instantiation (decode_frame_wave<false>, the synthesis kernel's): decode_frame_wave<true> with a "
         "record is the Q4 resume, which takes the SILK PCM from the handoff and does not call silk_decode_20ms again (og_decode.hpp: "
         "`mode != MODE_CELT && !q4_resume`), and RFC mode has no records")
R_LOSS_INST = ("the synthesis lambda is compiled once per caller of silk_decode_packet: in reference mode's instance (silk_decode_20ms) there is no "
               "loss state, in decode_frame_rfc's and conceal_chunk_rfc's there always is one, and a concealment chunk conceals every coded "
               "channel (lost == 1 sets conceal[n] for all n)")
R_ORACLE = "the oracle's twin side is unreachable for the same reason (tests/golden/rare_paths.json, tests/golden/make_rare_paths.py): "
UNREACHABLE = [
    ("|celt_decode_frame|for (LM = 0", R_FSIZE), ("|celt_decode_frame|if (LM > 3)", R_FSIZE),
    ("|celt_decode_lost|for (LM = 0", R_FSIZE), ("|celt_decode_lost|if (LM > 3)", R_FSIZE),
    ("|celt_conceal|(frame_size == 120", R_FSIZE),
    ("|celt_decode_frame|if (rc.storage > 1275", R_STORAGE),
    ("|celt_decode_frame|if (rc_tell(rc) > 8", R_TELL), ("|celt_parse_lane|if (rc_tell(rc) > 8", R_TELL),
    ("|recon_finish|if (flags & RF_TELL_OVERFLOW)", R_TELL),
    ("|celt_post|celt_post_lane(", R_TELL + "; so a frame that was synthesised has result >= 0"),
    ("|celt_decode_lost|const int N = 120 << LM, effEnd", "end is the band count of the last decoded frame's bandwidth, 13 .. 21, and start is 0 or 17 "
     "with end 19 or 21 for hybrid: OG_MIN(end, NBANDS) is end and not below start (og_decode.hpp end_band, loss.celt_end_band)"),
    ("|comb_filter|const int chunk_fade", "OG_MIN evaluates the chosen operand a second time: the side where that operand is the 1 << 20 of a filter "
     "with zero gain.  T0, T1 <= 1022, so such an operand is chosen only when both gains are zero, and comb_filter has returned by then (g0 == 0 && g1 == 0)"),
    ("og_celt_bands.hpp|compute_theta|} else if (stereo) {", R_ORACLE + "a mono split never has qn == 1 (tests/test_rare_paths.py test_a_mono_split_never_has_qn_1 walks the ROM tables)"),
    ("|split_theta_lane|if (qn != 1)", R_ORACLE + "split_theta_lane is compute_theta for mono splits, and a mono split never has qn == 1 "
     "(tests/test_rare_paths.py test_a_mono_split_never_has_qn_1 walks the ROM tables)"),
    ("|decode_all_bands|if (out1 >= 0)", "N == 1 only for the bands of width 1 at LM 0 (bands 0 .. 7), and lowband_out is absent only for the last band, "
     "20, whose width is 22: out1 is never negative here (the oracle's quant_band_n1 side, tests/golden/rare_paths.json)"),
    ("|decode_all_bands|if (dual_stereo && out2 >= 0)", "as for out1: a band of width 1 is never the last band, so with dual stereo out2 is a real offset"),
    ("|ordery|", "the Hadamard order is used with long blocks only, where the block count comes from time-splitting alone: 1 << -tf_change <= 8 for LM <= 3; "
     "a stride of 16 arises only in transient frames (8 short blocks split once more), which interleave in natural order: the table of 16 is never read"),
    ("|stereo_merge|if (k", R_ORACLE + "the function has returned unless both energies are at least 161061 > 2^17, so kl and kr are at least 8"),
    ("|pm_stereo_merge|if (k", R_ORACLE + "the merge has been skipped unless both energies are at least 161061 > 2^17, so kl and kr are at least 8"),
    ("|celt_exp2|if (integer > 14)", R_ORACLE + "anti-collapse passes a value <= 0 and the denormalisation clamps its argument first"),
    ("|celt_sqrt|", R_ORACLE + "the only caller passes N << 22 with a band width 1 <= N <= 176: neither 0 nor 2^30 and above"),
    ("|cos_norm|", R_ORACLE + "exp_rotation's theta lies in (0, 16384), so both arguments lie in (0, 32768) and none has its low 15 bits clear"),
    ("|celt_parse_lane|if (band < start || band >= end)", "end is NBANDS in celt_parse_lane (reference mode decodes all 21 bands, Q1), so `band >= end` never holds"),
    ("|celt_parse_lane|if (len < 0 || len > 1275 ||", R_FRAMING + "; and a hybrid frame's handoff is invalid only when its SILK half failed, which needs an impossible sampling rate"),
    ("|celt_parse_lane|if (rc.error || out.nw > REC_MAX_WORDS", R_LIMITS), ("|celt_parse_lane|rec->n_leaves = OG_MIN", R_LIMITS),
    ("|celt_parse_lane|rec->n_words = OG_MIN", R_LIMITS), ("og_celt_parse.hpp|leaf|", R_LIMITS), ("og_celt_parse.hpp|word|", R_LIMITS),
    ("og_celt_parse.hpp|words4|", R_LIMITS), ("og_celt_parse.hpp|patch|", R_LIMITS), ("|parse_all_bands|out.rec->band_w[i] =", R_LIMITS),
    (("|recon_fast_eligible|", "|b1"), R_LM3), ("|recon_fast_eligible|", R_LIMITS),
    ("|parse_all_bands|if (N == 1)", R_LM3 + ": the narrowest band is 8 coefficients wide at LM 3"),
    ("|parse_all_bands|if (N == 2)", R_LM3 + ": the narrowest band is 8 coefficients wide at LM 3"),
    ("|parse_all_bands|} else if (n2case)", R_LM3 + ": the narrowest band is 8 coefficients wide at LM 3, so no stereo band has N == 2"),
    ("|anti_collapse_r|if (LM == 3)", "anti_collapse_r serves the records of celt_parse_lane, all LM 3 (the oracle's twin side in reference mode: R_TRANS of make_rare_paths.py)"),
    ("|anti_collapse_r|if (i >= start && i < end)", "end is NBANDS and the loop runs over the 21 bands of each channel: i < end always holds"),
    ("|parse_tree|if (x + N >= 2048", R_TRAP),
    ("|pulses_rest|", "the loop pads the 21 bands to 24 words and guards the table index with i < NBANDS; `i >= start && i < end` is false for the pad "
     "(end = 21), so the guarded index is only evaluated for i < 21 and its other arm never runs"),
    ("|pvq_block_mul|", "a leaf's block count divides its size: quant_band doubles B only while N / B is even and a split halves both (parse_all_bands, "
     "parse_tree), so blen = N >> logB is at least 1"),
    (("|pvq_leaf_lane|if (k <= 13 && n > k && n > 3)", "|b1"), "no codebook has more dimensions than pulses with K > 13: V(N, K) must fit 32 bits, and the pulse "
     "cache ends below K = 14 for every N >= 15 (tests/test_kernel_paths.py test_sparse_leaves_have_at_most_13_pulses walks the cache in the ROM)"),
    (("|pvq_leaf_lane|if (k <= 13 && n > k && n > 3)", "|b3"), "the line sits inside `if (sparse)`, and sparse is n > k: the second condition always holds"),
    ("|pvq_leaf_lane|if (p0 <= i && s == 0)", "a codeword index is below V(n, k) = U(n, k) + U(n, k + 1) = p0 + p1: when the sign test fired (i >= p1, s = -1) "
     "what is left, i - p1, is below p0, so `p0 <= i` holds only with s == 0"),
    ("|plc_pitch_search|const int p = OG_MIN(PLC_PMAX", "both rounds of the search answer a lag inside their bounds or the fallback: round one's lies in PLC_PMIN / 2 .. "
     "PLC_PMAX / 2 = 50 .. 360, round two searches max(PLC_PMIN, 2 best - 1) .. min(PLC_PMAX, 2 best + 1) with the fallback 2 best, all inside 100 .. 720: the clamp never acts"),
    ("|plc_ratio_q15|if (b <= 0", "both callers pass a sum of squares plus one, and the common shift leaves the divisor at 2^29 or more when it acts: b is never 0 or negative"),
    ("|recon_band_mono|", R_NOT_FAST), ("|recon_finish|if (!pm)", R_NOT_FAST), ("|recon_finish|if (pm)", R_NOT_FAST),
    ("|recon_begin|if ((role == RECON_FAST_ONLY", R_REST_FILTER), ("|recon_begin|if (rx.flags & RF_SKIP)", R_SKIP),
    ("og_common.hpp|ilog|", "every caller passes a non-zero value: the range decoder's rng is above 2^23, an ec_dec_uint total is at least 2, qn >= 2 where "
     "it is logged, celt's isqrt and log2tan take positive arguments"),
    ("og_common.hpp|rshift_round64|", "the shifts passed are 31, 16 and inverse_pred_gain's mult2Q = 32 - clz(1 - rc^2 in Q30): the stability guard lets through "
     "|rc| <= 0.99975 only, so 1 - rc^2 >= 2^19 in Q30 and mult2Q is 20 .. 31: s == 1 never occurs"),
    ("|conceal_chunk_rfc|if (ret) return INTERNAL_ERROR;", R_SILK_RET), ("|decode_frame_rfc|if (ret) return INTERNAL_ERROR;", R_SILK_RET),
    ("|decode_frame_wave|if (ret) return INTERNAL_ERROR;", R_SILK_RET), ("|decode_frame_wave|if (r0 < 0) return r0;", R_SILK_RET + " (the record's ret)"),
    ("|silk_params_channel|if (t.skip) return;", R_SILK_RET + " (the record's ret)"), ("|silk_params_shadow|if (t.skip || !shadow)", R_SILK_RET + " (the record's ret)"),
    ("|conceal_chunk_rfc|OG_FOR_LANES(i, audiosize * CC) (hold ? hold : pcm)[i] = 0;",
     "the side is `hold` set while nothing has been decoded yet (mode 0): decode_frame_rfc asks for a held concealment only for a transition, and "
     "a transition needs prev_mode > 0 (og_decode.hpp: `transition = prev_mode > 0 && ...`)"),
    ("|conceal_chunk_rfc|", R_CELT_RET), ("|conceal_frame_rfc|if (r < 0)", R_CELT_RET),
    ("|decode_frame_rfc|if (len < 0 || len > 1275)", R_FRAMING), ("|decode_frame_wave|if (len < 0 || len > 1275)", R_FRAMING),
    ("|silk_parse_lane|if (len < 0 || len > 1275)", R_FRAMING),
    ("|decode_frame_rfc|celt_ret = celt_conceal(", "gcov's sides of `mode == MODE_CELT ? 0 : 17` on this line: a frame recovered from forward error "
     "correction data is SILK-only or hybrid (fec_plan: CELT-only packets are concealed, not recovered), and a lost CELT layer inside "
     "decode_frame_rfc is a hybrid frame's, so the concealment here always starts at band 17"),
    ("|decode_frame_rfc|pcm[i] = (i16)(i < nmix", "the fade-out frame is added to a SILK-only frame, which is at least 10 ms long: nmix >= 480 exceeds the "
     "120 * CC <= 240 entries of the fade, so `i < nmix` always holds"),
    ("|decode_frame_rfc|", R_CELT_RET),
    ("|decode_frame_wave|if (WITH_CELT && mode == MODE_SILK && prev_mode == MODE_HYBRID)", R_REC + "; WITH_CELT is a template constant: gcov's sides for "
     "it on the instantiation that has a record are those of the Q4 resume alone"),
    ("|decode_frame_wave|if (q4_resume)", R_REC + ": inside `if (srec)` with WITH_CELT the call IS the Q4 resume"),
    ("|decode_frame_wave|if (mode != MODE_SILK) return INTERNAL_ERROR;", "decode_frame_wave<false> returns CONTINUE_SPLIT for a hybrid frame before this "
     "line and is never called for a CELT-only one (the split path sends those to celt_parse_lane)"),
    ("|silk_decode_packet|if (fs_kHz != 8", R_RATE), ("|silk_parse_lane|if (fs_kHz != 8", R_RATE),
    ("|silk_decode_packet|const int nF =", R_REC), ("|silk_decode_packet|const int nb_subfr =", R_REC),
    ("|silk_decode_packet|if (!rec && !lost && channels == 2)", R_REC), ("|silk_decode_packet|if (REC_ONLY || rec)", R_REC),
    ("|silk_decode_packet|pulse_row[", R_REC),
    ("|silk_decode_packet|if (channels == 2 && (s->nChannelsAPI == 1 || s->nChannelsInternal == 1))", R_ORACLE + "nChannelsAPI and nChannelsInternal are "
     "always assigned together: when the first is not 1 the second is not either"),
    ("|silk_decode_packet|if (loss) {", R_LOSS_INST), ("|silk_decode_packet|if (conceal[n])", R_LOSS_INST),
    ("|silk_decode_parameters|k.Gains_Q16[j] = silk_log2lin(OG_MIN(", R_ORACLE + "smulwb(1907825, 63) + 2090 = 3924 < 3967: the clamp never acts"),
    ("|silk_log2lin|", R_ORACLE + "the only caller passes 2090 .. 3924: never negative, never below 2048, never 3967 or more"),
    ("|silk_div32_varQ|", R_ORACLE + "the only caller divides two gains of 2^16.3 .. 2^30.7: lshift <= 27"),
    ("|silk_inverse32_varQ|", R_ORACLE + "lshift is 0 from inverse_pred_gain and 14 - b_headrm from the core: always below 32"),
    ("|silk_nlsf2a|for (int i = 0; silk_inverse_pred_gain", R_ORACLE + "in round 15 the chirp is 0, every coefficient becomes zero and the all-zero "
     "filter is stable: `i < 16` is never evaluated as false"),
    ("|silk_params_channel|if (n == 1 && channels == 2 && dom == 0 && prev_dom == 1)", "the function returns above for a channel that is not coded "
     "(t.coded = n < channels && !(n == 1 && dom)): channel 1 arrives here only with channels == 2 and dom == 0, so the second and the "
     "third condition always hold when they are reached"),
    ("|silk_parse_indices|", R_20MS), ("|silk_parse_pulses|if (iter * 16 < frame_length)", R_20MS), ("|silk_skip_pulses|if (iter * 16 < frame_length)", R_20MS),
    ("|silk_sum_sqr_shift|", "both callers pass a subframe length 5 * fs_kHz (40, 60 or 80) or a frame length, a multiple of it: always even, so the loop "
     "over pairs covers every sample and the odd tail never runs (kept as the reference has it, silk.cpp:3839)"),
]

T_SUBSAT = ("as for the oracle's twin side (tests/golden/saturation_paths.json, open): the step-down recursion's subtraction clamps only when two "
            "Q24 coefficients sum past 128.0, and in everything tried the guard on the next line ends the recursion first -- no proof that it must; "
            "tried here: all families of make_kernel_paths.py and, through the baseline, the saturation corpus and the exhaustive NLSF corners")
TRIED = [
    ("og_celt_recon_pm.hpp|anti_collapse_pm|", "a limit of the drive, not of the code: the sides are a band outside start .. end (end is NBANDS always), and the phase-major anti-collapse is compiled only "
     "in the tight library, which has no SILK half and so is fed CELT-only streams (start 0).  On the device k_celt_recon_fb takes the CELT "
     "layer of hybrid frames (start 17) through this code: the hybrid batches of tests/test_gpu_transient_frames.py and "
     "tests/test_gpu_fill_windows.py compare it with the oracle; an emulation entry that hands a hybrid frame's record to the tight layout "
     "would take them"),
    ("|pm_fill_jobs|if ((w0 & BW_HAS_LOW) && want_low && (jw & JW_NEED_LOW))", "believed unreachable, not proven: the side is a job that runs in pm_fill_jobs with a "
     "folding source on offer (BW_HAS_LOW, not a side job) whose record says it needs none, i.e. a job without fill leaves that still has pulses "
     "and a non-empty fill mask; tried: all families of make_kernel_paths.py, CELT frames of 2 .. 1275 bytes with loud, quiet and mixed energies"),
    ("og_common.hpp|sub_sat32|", T_SUBSAT),
    ("og_common.hpp|limit32|", "the arm for bounds given in the other order (l1 > l2): the gain index, the NLSF decode, the pitch lag and the shift "
     "saturation pass constant bounds in order; silk_nlsf_stabilize's min_center and max_center could cross where the minimum distances do not "
     "fit -- silk_LIMIT takes either order for that reason -- and nothing decoded makes them: the baseline with the exhaustive NLSF corners of "
     "the rare-paths corpus, and all families of make_kernel_paths.py"),
]
NEVER_ENTERED = [
    ("|recon_all_bands", "unreachable: " + R_NOT_FAST), ("|rec_word4", "unreachable: only recon_all_bands reads the record this way; " + R_NOT_FAST),
    ("|stream_reset", "open: a limit of the drive: the host resets streams through k_stream_reset (og_api.hip), the tool starts every stream with emu_stream_init and never resets one; "
     "tests/test_gpu_rfc.py test_rfc_loss_before_any_packet_and_after_reset and tests/test_gpu_pipeline.py run the kernel"),
]


def reason_in(table, key):
    for sub, why in table:
        if all(s in key for s in (sub if isinstance(sub, tuple) else (sub,))):
            return why
    return None


# ---- candidate families: (channels, [packet bytes], rfc, [fec indices]) ------------------------------------------------------------------
def _noise(r, n):
    return bytes(r.randrange(256) for _ in range(n))


def _reference(fam):
    def f(r):
        c = fam(r)
        return c and (c[0], c[1], False, [])
    f.__doc__ = fam.__doc__
    return f


def family_ref_walk(r):
    """reference mode: random TOC walks (every configuration as a 20 ms frame), mono and stereo packets in either decoder, payloads of
    0, 1, 2 bytes among ordinary ones -- the frames the split path hands back (a CELT frame of at most one byte) among them"""
    ch = r.choice([1, 2])
    cfg = r.randrange(32)
    pkts = []
    for _ in range(r.choice([1, 2, 3, 5, 8])):
        if r.random() < 0.4:
            cfg = r.randrange(32)
        stereo = (ch == 2) if r.random() < 0.75 else bool(r.randrange(2))
        n = r.choice([0, 1, 1, 2, 3, 5, 9, 17, 40, 100, 160, 300, 700, 1275])
        kind = r.randrange(8)
        body = bytes(n) if kind == 0 else (b"\xff" * n if kind == 1 else _noise(r, n))
        pkts.append(bytes([cfg << 3 | (4 if stereo else 0)]) + body)
    return ch, pkts, False, []


def _rfc_packet(r, cfg, stereo, body_of):
    """one packet with frame-count code 0..3; body_of(n) -> n payload bytes"""
    code = r.choice([0, 0, 0, 1, 2, 3])
    toc = cfg << 3 | (4 if stereo else 0) | code
    L = r.choice([3, 8, 20, 40, 80, 120, 160, 300]) if r.random() >= 0.1 else r.randrange(2)
    if code == 0:
        return bytes([toc]) + body_of(L)
    if code == 1:
        return bytes([toc]) + body_of(L) + body_of(L)
    if code == 2:
        L = min(L, 250)
        return bytes([toc, L]) + body_of(L) + body_of(L + r.randrange(120))
    import rfc_common as rc
    cnt = r.randrange(1, 5)
    while rc.dur(toc) * cnt > 5760:
        cnt -= 1
    return bytes([toc, cnt]) + b"".join(body_of(L) for _ in range(cnt))


def family_rfc_walk(r, cfgs=range(32), p_loss=0.25, p_fec=0.15):
    """RFC mode: configuration walks over all 32 TOC configurations and the four frame-count codes, losses (bursts), DTX frames and
    decode_fec marks, mono and stereo packets in either decoder"""
    cfgs = list(cfgs)
    ch = r.choice([1, 2])
    cfg = r.choice(cfgs)
    pkts, fec = [], []
    for k in range(r.choice([2, 3, 5, 8])):
        if k and r.random() < p_loss:
            pkts.append(b"")
            continue
        if r.random() < 0.35:
            cfg = r.choice(cfgs)
        stereo = (ch == 2) if r.random() < 0.8 else bool(r.randrange(2))
        kind = r.randrange(10)
        pkts.append(_rfc_packet(r, cfg, stereo, lambda n: bytes(n) if kind == 0 else (b"\xff" * n if kind == 1 else _noise(r, n))))
        if r.random() < p_fec:
            fec.append(k)
    return ch, pkts, True, fec


def family_rfc_celt_loss(r):
    """RFC mode, CELT-only: crafted frames (post-filter on or off, loud or quiet or mixed energies, at every LM) and then bursts of losses:
    the pitch search of the concealment on periodic, silent and clipped histories, the decaying noise behind it"""
    ch = r.choice([1, 2])
    pkts = []
    LM = r.randrange(4)
    for k in range(r.choice([3, 5, 8])):
        if k >= 1 and r.random() < 0.5:
            pkts.append(b"")
            continue
        stereo = (ch == 2) if r.random() < 0.8 else bool(r.randrange(2))
        n = r.choice([2, 3, 8, 20, 60, 160, 400, 1275])
        try:
            body = _celt_lm_payload(r, 2 if stereo else 1, n, LM)
        except rcc.CraftError:
            body = _noise(r, n)
        pkts.append(bytes([0x80 | r.randrange(4) << 5 | LM << 3 | (4 if stereo else 0)]) + body)
    return ch, pkts, True, []


def _celt_lm_payload(r, C, n, LM):
    kind = r.choice(["loud", "quiet", "mixed", "none", "silence"])
    if kind == "silence":
        return rcc.celt_frame(n, C, silence=1, fill=_noise(r, n), LM=LM)
    coarse = None
    if kind != "none":
        v = {"loud": lambda: r.choice([3, 5, 8]), "quiet": lambda: r.choice([-3, -5, -8]), "mixed": lambda: r.choice([-6, 0, 6])}[kind]
        coarse = [[v(), v()] for _ in range(r.choice([3, 8, 21]))]
    pf = None
    if r.random() < 0.5:
        octave = r.randrange(6)
        pf = (octave, r.randrange(16 << octave), r.randrange(8), r.randrange(3))
    return rcc.celt_frame(n, C, postfilter=pf, transient=r.randrange(2) if LM else 0, intra=r.randrange(2), coarse=coarse,
                          fill=_noise(r, n), LM=LM)


def family_rfc_silk(r):
    """RFC mode, SILK-only and hybrid 20 ms frames with pinned side information (extreme NLSF residuals, pulse heads), with losses and
    decode_fec marks around them: the concealment's piecewise chunks on voiced and unvoiced pasts"""
    stereo = r.random() < 0.4
    ch = 2 if stereo else r.choice([1, 1, 2])
    pkts, fec = [], []
    for k in range(r.choice([2, 3, 5, 8])):
        if k and r.random() < 0.35:
            pkts.append(b"")
            continue
        fs = r.choice([8, 12, 16])
        hybrid = r.random() < 0.3
        n = r.choice([30, 60, 120, 250])
        try:
            body = mrp._silk_payload(r, 16 if hybrid else fs, stereo, n)
        except rcc.CraftError:
            body = _noise(r, n)
        toc = (r.choice([0x68, 0x78]) if hybrid else mrp.SILK_TOC[fs]) | (4 if stereo else 0)
        pkts.append(bytes([toc]) + body)
        if r.random() < 0.2:
            fec.append(k)
    return ch, pkts, True, fec


_SWEEP = {}


def family_q4_tail(r):
    """reference mode: a hybrid frame, then a SILK-only frame cut at every length in turn -- the 2.5 ms CELT frame behind it (Q4) starts on
    what SILK left of the coder, from band 0, so some length leaves it exactly the 16 bits that let the post-filter in and none
    for its tapset"""
    if not _SWEEP.get("left"):
        stereo = r.random() < 0.3
        _SWEEP.update(ch=2 if stereo else 1, first=bytes([0x78 | (4 if stereo else 0)]) + _noise(r, r.choice([30, 60])),
                      toc=mrp.SILK_TOC[r.choice([8, 12, 16])] | (4 if stereo else 0), body=_noise(r, 70), left=list(range(8, 70)))
    n = _SWEEP["left"].pop()
    return _SWEEP["ch"], [_SWEEP["first"], bytes([_SWEEP["toc"]]) + _SWEEP["body"][:n]], False, []


FAMILIES = [_reference(mrp.family_silk), _reference(mrp.family_celt), _reference(mrp.family_q4), _reference(mrp.family_hybrid),
            family_ref_walk, family_rfc_walk, family_rfc_celt_loss, family_rfc_silk,
            lambda r: family_rfc_walk(r, range(16, 32), 0.5, 0.0), lambda r: family_rfc_walk(r, range(0, 16), 0.3, 0.4)]


def tried(key):
    return reason_in(TRIED, key) or ("all families of make_kernel_paths.py (reference and RFC walks, crafted CELT frames at every LM with "
                                     "loss bursts, crafted SILK frames with losses and decode_fec), none aimed at this side in particular")


def _as_seq(c):
    s = {"channels": c[0], "packets": [p.hex() for p in c[1]], "rfc": c[2]}
    if c[3]:
        s["fec"] = [k for k in c[3] if k < len(c[1])]
    return s


def _drop_front(seq):
    s = dict(seq, packets=seq["packets"][1:])
    if seq.get("fec"):
        s["fec"] = [k - 1 for k in seq["fec"] if k >= 1]
    return s


def search(cov, targets, seed, rounds, batch, families=None):
    families = families or FAMILIES
    r = random.Random(seed)
    entries, left = [], set(targets)
    for rnd in range(rounds):
        if not left:
            break
        cands = []
        while len(cands) < batch:
            c = families[rnd % len(families)](r)
            if c and c[1] and (c[2] or all(c[1])):
                cands.append(_as_seq(c))

        def new_sides(seqs):
            try:
                cov.decode(seqs)
            except RuntimeError:
                if len(seqs) == 1:
                    print("A CANDIDATE THE EMULATION DECODES DIFFERENTLY FROM THE ORACLE:\n" + json.dumps(seqs[0]), file=sys.stderr)
                    raise
                new_sides(seqs[:len(seqs) // 2])
                new_sides(seqs[len(seqs) // 2:])
                raise
            return left & cov.untaken()[1]

        pool = cands
        while True:
            got = new_sides(pool)
            if not got:
                break
            key = sorted(got)[0]
            lo = pool
            while len(lo) > 1:
                half = lo[:len(lo) // 2]
                lo = half if key in new_sides(half) else lo[len(lo) // 2:]
            seq = first = lo[0]
            while len(seq["packets"]) > 1:  # shrink: drop packets from the front while the side stays taken
                shorter = _drop_front(seq)
                if (shorter["rfc"] or all(shorter["packets"])) and key in new_sides([shorter]):
                    seq = shorter
                else:
                    break
            keys = sorted(new_sides([seq]))
            assert key in keys
            expect = cov.decode([seq])[0]
            entries.append(dict(seq, keys=keys, expect=expect))
            left -= set(keys)
            print(f"round {rnd}: +{len(keys)} ({len(left)} left)  {keys[0]}", file=sys.stderr)
            pool = [c for c in pool if c is not first]
    return entries, left


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20251)
    ap.add_argument("--rounds", type=int, default=22)
    ap.add_argument("--batch", type=int, default=300)
    ap.add_argument("--baseline", action="store_true", help="measure the baseline list again instead of reusing the fixture's")
    a = ap.parse_args()
    with kb.CoverageBuild() as cov:
        if a.baseline or not os.path.exists(OUT):
            kb.decode_in_chunks(cov, kb.baseline_sequences())
            baseline, never = sorted(cov.untaken()[0]), cov.never_entered()
        else:
            old = json.load(open(OUT))
            baseline, never = old["baseline"], sorted(old["never_entered"])
        reasons, emulation, unreachable = [], {}, {}  # the fixture holds every reason once: key -> index into "reasons"

        def ref(why):
            if why not in reasons:
                reasons.append(why)
            return reasons.index(why)

        for k in baseline:
            why = reason_in(EMULATION, k)
            if why:
                emulation[k] = ref(why)
                continue
            why = reason_in(UNREACHABLE, k)
            if why:
                unreachable[k] = ref(why)
        targets = [k for k in baseline if k not in unreachable and k not in emulation]
        # the directed stage: the tapset side needs the 2.5 ms CELT frame behind a hybrid frame to start with 16 bits left, one length in
        # some thousands (family_q4_tail sweeps them)
        entries, _ = search(cov, [k for k in targets if "tapset_icdf" in k], 7, 12, 1240, [family_q4_tail])
        more, left = search(cov, [k for k in targets if not any(k in e["keys"] for e in entries)], a.seed, a.rounds, a.batch)
        entries += more
    fx = {"about": "directed packets for rarely taken branch sides of the kernel source in host emulation; made by "
                   "tests/golden/make_kernel_paths.py, read by tests/test_kernel_paths.py, tests/test_gpu_kernel_paths.py and "
                   "tools/kernel_branches.py --corpus.  expect: per packet [return code, final range, crc32 of the PCM] of the oracle "
                   "(reference mode, or RFC mode for the entries marked rfc: an empty packet is a loss, fec lists the packets before "
                   "which decode_fec is asked for)",
          "gcc": kb.gcc_version(), "seed": a.seed, "rounds": a.rounds, "batch": a.batch, "baseline": baseline, "reasons": reasons,
          "emulation": emulation, "unreachable": unreachable, "open": {k: tried(k) for k in sorted(left)},
          "never_entered": {k: (reason_in(NEVER_ENTERED, k) or "") for k in never}, "entries": entries}
    with open(OUT, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print(f"baseline {len(baseline)}: reached {len(targets) - len(left)}, emulation {len(emulation)}, unreachable {len(unreachable)}, "
          f"open {len(left)}; {len(entries)} entries, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
