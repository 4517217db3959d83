#!/usr/bin/env python3
"""Which branch sides of the KERNEL source, in host emulation, does a set of packet sequences leave untaken?  CPU only.

The twin of tools/oracle_branches.py for the device source.  The tool builds tests/emul/og_emul.cpp and
tests/emul/og_emul_tight.cpp with `g++ -O0 --coverage -fno-exceptions` and the flags of csrc/BUILD_FLAGS into a temporary
directory of its own (never in-tree; tests/emul/Makefile is not used), decodes the sequences in a child process, reads
`gcov --json-format --branch-probabilities` and reports every EXECUTED line of an in-scope header that has a branch side with
count 0, and every in-scope function that was compiled but never entered.  A side is keyed by

    file | function | stripped source text of the line [@n for the n-th line with that text in the function] | b<k>

The function is its demangled unqualified name, template arguments and parameter list dropped; counts are summed over
instantiations and over the two libraries (a line whose instantiations differ in their number of branches is left out: the
ordinals would not line up).  k is the ordinal of the branch on that line in gcov's order.  Line numbers are not
part of a key: they move.

A sequence is one stream from emu_stream_init: {"channels": c, "packets": [hex, ...], "rfc": bool, "fec": [packet indices]}.
  * Reference mode (rfc false): every packet is one 20 ms frame; an empty packet is a frame of no bytes in the mode of the last
    packet (mode 0 before the first: what the reference's empty-packet branch does, tests/test_empty_packets.py).  The stream is
    decoded through emu_decode_frame, emu_decode_frame_single and emu_decode_frame_shadowed (CELT-only frames of the shadowed run go the ordinary way and end the
    copy's epoch, as the host does), each from a fresh state; a stream with CELT-only packets once more with those through
    emu_decode_frame_roles (the two reconstruction kernels of a pipelined CELT window in their roles RECON_FAST_ONLY and
    RECON_REST_ONLY); a stream of CELT-only packets also through the tight library, where it ends at the first frame that
    library answers -999.
  * RFC mode: packets are framed with the oracle's oc_packet_parse (rfc_common.frame_payloads) and go frame by frame through
    emu_decode_frame_rfc.  An empty packet is a loss: concealed for the duration of the stream's last packet, cut into device
    frames by rfc_common.conceal_pieces.  A packet index listed under "fec" asks for decode_fec before that packet
    (emu_decode_frame_rfc_fec, planned by rfc_common.fec_plan), after which the packet is decoded normally.
While it decodes, the child decodes every sequence with the oracle too (reference or RFC mode) and compares return codes and PCM
(RFC mode: over the domain rfc_common.same_pcm defines).  A difference ends the run: a census over a wrong decode is worthless.

Scope: SCOPE_FILES below, under esp32-opus-player_amd/csrc/.  og_output.hpp, the stage taps (OG_TAP) and whatever sits under
OG_STATS / OG_PROF (not compiled here) are out of scope.

    python tools/kernel_branches.py --baseline            # everything the suite already decodes (baseline_sequences; minutes)
    python tools/kernel_branches.py --corpus [--entry N]  # tests/golden/kernel_paths.json, or one entry of it alone:
                                                          # prints the claimed keys and whether each is taken
    python tools/kernel_branches.py --json FILE           # sequences from FILE

BASELINE -- what the suite decodes already (baseline_sequences):
  1. the families of oracle_branches.baseline_sequences at their full counts;
  2. tests/golden/rare_paths.json and tests/golden/saturation_paths.json, the rfc entries of the latter in RFC mode;
  3. the crafted batches of tests/test_gpu_comb_history.py, test_gpu_fill_windows.py, test_gpu_synth_stages.py,
     test_gpu_transient_frames.py and test_anti_collapse_cells.py, through their own builders;
  4. the three payload shapes of tests/test_gpu_bench_shapes.py at 256 streams;
  5. the RFC walks of the five plans of tests/test_gpu_rfc.py (rfc_common.rfc_plan / draw_step, which that test walks too);
  6. reference-mode walks with empty packets as tests/test_empty_packets.py decodes them, the mode-0 frame of a stream that has
     had no packet yet among them (empty_packet_sequences).
The report over it is data in tests/golden/kernel_paths.json under "baseline" (regenerate: tests/golden/make_kernel_paths.py
--baseline), with the four sets every side belongs to.  tests/test_kernel_paths.py checks the corpus against them.  The 193 sides
(g++ 11.4.0; functions never entered: og_celt_recon.hpp|rec_word4, og_celt_recon.hpp|recon_all_bands, og_decode.hpp|stream_reset):

    og_celt.hpp|celt_decode_frame|for (LM = 0; LM <= 3; LM++)|b1
    og_celt.hpp|celt_decode_frame|if (LM > 3) return CELT_BAD_ARG; // celt.cpp:2211|b0
    og_celt.hpp|celt_decode_frame|if (rc.storage > 1275 || rc.storage <= 1) return CELT_BAD_ARG; // :2216, :2225|b1
    og_celt.hpp|celt_decode_frame|if (rc_tell(rc) > 8 * (i32)rc.storage) return INTERNAL_ERROR;|b0
    og_celt.hpp|celt_decode_lost|const int N = 120 << LM, effEnd = OG_MAX(start, OG_MIN(end, NBANDS));|b2
    og_celt.hpp|celt_decode_lost|for (LM = 0; LM <= 3; LM++)|b1
    og_celt.hpp|celt_decode_lost|if (LM > 3) return BAD_ARG;|b0
    og_celt.hpp|celt_parse_header|if (rc_tell(rc) + 2 <= total_bits) { // tapset_icdf {2,1,0}, ftb 2|b1
    og_celt.hpp|celt_post4|if (pcm) {|b1
    og_celt.hpp|comb_filter|const int chunk_fade = OG_MIN(use0 ? T0 : 1 << 20, use1 ? T1 : 1 << 20) - 2, chunk_rest = T1 - 2;|b7
    og_celt.hpp|comb_filter|const int chunk_fade = OG_MIN(use0 ? T0 : 1 << 20, use1 ? T1 : 1 << 20) - 2, chunk_rest = T1 - 2;|b9
    og_celt.hpp|imdct_channel|const int b = ppb == 1 ? it : it / ppb, i = OG_LANE + (it - b * ppb) * OG_NLANES;@2|b1
    og_celt.hpp|imdct_channel|const int b = ppb == 1 ? it : it / ppb, i = OG_LANE + (it - b * ppb) * OG_NLANES;|b1
    og_celt.hpp|imdct_channel|if (i < N4 && b < B) {@2|b1
    og_celt.hpp|imdct_channel|if (i < N4 && b < B) {@2|b3
    og_celt.hpp|imdct_channel|if (i < N4 && b < B) {|b1
    og_celt.hpp|imdct_channel|if (i < N4 && b < B) {|b3
    og_celt_bands.hpp|compute_theta|} else if (stereo) {|b1
    og_celt_bands.hpp|decode_all_bands|if (dual_stereo && out2 >= 0) S.v[out2] = (i16)(S.v[y] >> 4);|b3
    og_celt_bands.hpp|decode_all_bands|if (out1 >= 0) S.v[out1] = (i16)(S.v[x] >> 4);|b1
    og_celt_bands.hpp|ordery|u64 t = stride == 2 ? t2 : (stride == 4 ? t4 : (stride == 8 ? t8 : t16));|b5
    og_celt_bands.hpp|stereo_merge|if (kl < 7) kl = 7;|b0
    og_celt_bands.hpp|stereo_merge|if (kr < 7) kr = 7;|b0
    og_celt_math.hpp|celt_exp2|if (integer > 14) return 0x7f000000;|b0
    og_celt_math.hpp|celt_sqrt|if (x == 0) return 0;|b0
    og_celt_math.hpp|celt_sqrt|if (x >= 1073741824) return 32767;|b0
    og_celt_math.hpp|cos_norm|if (x & 0x7fff) {|b1
    og_celt_math.hpp|cos_norm|if (x < (1 << 15)) return cos_quarter(tr16(x));|b1
    og_celt_math.hpp|cos_norm|if (x > (1 << 16)) x = (1 << 17) - x;|b0
    og_celt_parse.hpp|celt_parse_lane|if (band < start || band >= end) e[k] = 0;|b2
    og_celt_parse.hpp|celt_parse_lane|if (len < 0 || len > 1275 || (handoff && !handoff->valid)) {|b1
    og_celt_parse.hpp|celt_parse_lane|if (len < 0 || len > 1275 || (handoff && !handoff->valid)) {|b3
    og_celt_parse.hpp|celt_parse_lane|if (len < 0 || len > 1275 || (handoff && !handoff->valid)) {|b6
    og_celt_parse.hpp|celt_parse_lane|if (rc.error || out.nw > REC_MAX_WORDS || out.nl > REC_MAX_LEAVES) flags |= RF_RC_ERROR;|b3
    og_celt_parse.hpp|celt_parse_lane|if (rc.error || out.nw > REC_MAX_WORDS || out.nl > REC_MAX_LEAVES) flags |= RF_RC_ERROR;|b4
    og_celt_parse.hpp|celt_parse_lane|if (rc_tell(rc) > 8 * (i32)rc.storage) flags |= RF_TELL_OVERFLOW;|b0
    og_celt_parse.hpp|celt_parse_lane|rec->n_leaves = OG_MIN(out.nl, REC_MAX_LEAVES);|b1
    og_celt_parse.hpp|celt_parse_lane|rec->n_words = OG_MIN(out.nw, REC_MAX_WORDS);|b1
    og_celt_parse.hpp|leaf|if (nl < REC_MAX_LEAVES) {|b1
    og_celt_parse.hpp|parse_all_bands|if (N == 1) { // quant_band_n1 celt.cpp:1357|b0
    og_celt_parse.hpp|parse_all_bands|if (N == 2) {|b0
    og_celt_parse.hpp|parse_all_bands|out.rec->band_w[i] = (u16)OG_MIN(out.band_begin(), REC_MAX_WORDS);|b1
    og_celt_parse.hpp|parse_all_bands|} else if (n2case) {|b0
    og_celt_parse.hpp|parse_tree|if (x + N >= 2048 || N > 255 || LM + 1 > 7 || B > 31 || off_side > 15) __builtin_trap();|b1
    og_celt_parse.hpp|parse_tree|if (x + N >= 2048 || N > 255 || LM + 1 > 7 || B > 31 || off_side > 15) __builtin_trap();|b3
    og_celt_parse.hpp|parse_tree|if (x + N >= 2048 || N > 255 || LM + 1 > 7 || B > 31 || off_side > 15) __builtin_trap();|b5
    og_celt_parse.hpp|parse_tree|if (x + N >= 2048 || N > 255 || LM + 1 > 7 || B > 31 || off_side > 15) __builtin_trap();|b7
    og_celt_parse.hpp|parse_tree|if (x + N >= 2048 || N > 255 || LM + 1 > 7 || B > 31 || off_side > 15) __builtin_trap();|b8
    og_celt_parse.hpp|patch|if (at < REC_MAX_WORDS) rec->words[at] = w;|b1
    og_celt_parse.hpp|pulses_rest|for (int i = 0; i < 24; i++) v[i] = (i >= start && i < end) ? (i32)PL.u.al.bw[i < NBANDS ? i : 0][OG_PCOL] : 0;|b5
    og_celt_parse.hpp|split_theta_lane|if (qn != 1) {|b1
    og_celt_parse.hpp|words4|if (nw + 4 <= REC_MAX_WORDS) {|b1
    og_celt_parse.hpp|word|if (nw < REC_MAX_WORDS) rec->words[nw] = w;|b1
    og_celt_recon.hpp|anti_collapse_r|if (LM == 3) r = tr16(mul16_q14(23170, OG_MIN(23169, r)));|b1
    og_celt_recon.hpp|anti_collapse_r|if (i >= start && i < end) {|b3
    og_celt_recon.hpp|celt_post|celt_post_lane(&st->celt, c, st->channels, 960, (st->celt.ring_pos - 960) & RING_MASK, result >= 0 ? pcm : nullptr, silk, 960 * ch);|b1
    og_celt_recon.hpp|pvq_block_mul|OG_DEV u32 pvq_block_mul(int blen) { return blen > 0 ? 65536u / (u32)blen + 1u : 0u; }|b1
    og_celt_recon.hpp|pvq_leaf_lane|if (defer) {|b0
    og_celt_recon.hpp|pvq_leaf_lane|if (k <= 13 && n > k && n > 3) {|b1
    og_celt_recon.hpp|pvq_leaf_lane|if (k <= 13 && n > k && n > 3) {|b3
    og_celt_recon.hpp|pvq_leaf_lane|if (p0 <= i && s == 0) {|b3
    og_celt_recon.hpp|recon_band_mono|if (low_out >= 0) {|b0
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b0
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b10
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b11
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b2
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b3
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b4
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b5
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b6
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b7
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b8
    og_celt_recon.hpp|recon_band_mono|if (low_scratch >= 0 && low >= 0 && (recombine || ((N_B & 1) == 0 && tf_change < 0) || B > 1)) {|b9
    og_celt_recon.hpp|recon_begin|if ((role == RECON_FAST_ONLY && !rx.fast) || (role == RECON_REST_ONLY && rx.fast)) {|b6
    og_celt_recon.hpp|recon_begin|if (rx.flags & RF_SKIP) {|b0
    og_celt_recon.hpp|recon_begin|if (rx.pre && OG_LANE < NBANDS) S.band_w_row()[OG_LANE] = (u16)rx.pre_band_w;|b0
    og_celt_recon.hpp|recon_fast_eligible|return ((h.flags >> RF_LM_SHIFT) & 3) == 3 && h.n_words < REC_MAX_WORDS && h.n_leaves <= FAST_MAX_LEAVES;|b1
    og_celt_recon.hpp|recon_fast_eligible|return ((h.flags >> RF_LM_SHIFT) & 3) == 3 && h.n_words < REC_MAX_WORDS && h.n_leaves <= FAST_MAX_LEAVES;|b3
    og_celt_recon.hpp|recon_fast_eligible|return ((h.flags >> RF_LM_SHIFT) & 3) == 3 && h.n_words < REC_MAX_WORDS && h.n_leaves <= FAST_MAX_LEAVES;|b5
    og_celt_recon.hpp|recon_finish|if (!pm) { // the band walk starts from an empty folding history (the PVQ table that was there is no longer needed)|b0
    og_celt_recon.hpp|recon_finish|if (!rx.booked) recon_bookkeeping(st, rx);|b1
    og_celt_recon.hpp|recon_finish|if (flags & RF_TELL_OVERFLOW) result = INTERNAL_ERROR;|b0
    og_celt_recon.hpp|recon_finish|if (pm)|b1
    og_celt_recon.hpp|recon_finish|if (rx.pre) {|b0
    og_celt_recon.hpp|recon_leaves_own|const bool first = pre && t < OG_NLANES;|b0
    og_celt_recon.hpp|recon_leaves_own|const bool first = pre && t < OG_NLANES;|b2
    og_celt_recon.hpp|recon_leaves_own|const bool first = pre && t < OG_NLANES;|b3
    og_celt_recon.hpp|recon_leaves_own|const u32 aux = first ? aux0 : rec->leaf[t].aux;|b0
    og_celt_recon.hpp|recon_leaves_own|const u32 g = first ? g0 : rec->leaf[t].geom;|b0
    og_celt_recon.hpp|recon_leaves_own|const u32 idx = first ? idx0 : rec->leaf[t].idx;|b0
    og_celt_recon_pm.hpp|anti_collapse_pm|const u32 clr = (i >= start && i < end) ? ~(u32)S.cmask_row()[e] & 0xffu : 0u;|b1
    og_celt_recon_pm.hpp|anti_collapse_pm|const u32 clr = (i >= start && i < end) ? ~(u32)S.cmask_row()[e] & 0xffu : 0u;|b3
    og_celt_recon_pm.hpp|anti_collapse_pm|if (e < NE && i >= start && i < end) {|b1
    og_celt_recon_pm.hpp|anti_collapse_pm|if (e < NE && i >= start && i < end) {|b3
    og_celt_recon_pm.hpp|anti_collapse_pm|if (e < NE && i >= start && i < end) {|b5
    og_celt_recon_pm.hpp|anti_collapse_pm|if (e < NE) ent[e] = lcg_skip(seed, before);|b1
    og_celt_recon_pm.hpp|anti_collapse_pm|if (i >= start && i < end && (~(u32)S.cmask_row()[e] & 0xffu)) {|b1
    og_celt_recon_pm.hpp|anti_collapse_pm|if (i >= start && i < end && (~(u32)S.cmask_row()[e] & 0xffu)) {|b3
    og_celt_recon_pm.hpp|pm_fill_jobs|if ((w0 & BW_HAS_LOW) && want_low && (jw & JW_NEED_LOW)) {|b5
    og_celt_recon_pm.hpp|pm_setup_jobs|const int bw = !coded ? 0 : bw_staged ? (int)S.band_w_row()[band] : (int)rec->band_w[band];|b1
    og_celt_recon_pm.hpp|pm_setup_jobs|const int bw = !coded ? 0 : bw_staged ? (int)S.band_w_row()[band] : (int)rec->band_w[band];|b2
    og_celt_recon_pm.hpp|pm_stereo_merge|if (kl < 7) kl = 7;|b0
    og_celt_recon_pm.hpp|pm_stereo_merge|if (kr < 7) kr = 7;|b0
    og_celt_recon_pm.hpp|pm_tf_undo|if (g < 2 * PM_GROUPS) {@2|b1
    og_celt_recon_pm.hpp|pm_tf_undo|if (g < 2 * PM_GROUPS) {@3|b1
    og_celt_recon_pm.hpp|pm_tf_undo|if (g < 2 * PM_GROUPS) {|b1
    og_common.hpp|ilog|OG_DEV int ilog(u32 x) { return x ? 32 - OG_CLZ(x) : 0; } // EC_ILOG :250|b1
    og_common.hpp|limit32|return l1 > l2 ? (a > l1 ? l1 : (a < l2 ? l2 : a)) : (a > l2 ? l2 : (a < l1 ? l1 : a));|b0
    og_common.hpp|limit32|return l1 > l2 ? (a > l1 ? l1 : (a < l2 ? l2 : a)) : (a > l2 ? l2 : (a < l1 ? l1 : a));|b2
    og_common.hpp|limit32|return l1 > l2 ? (a > l1 ? l1 : (a < l2 ? l2 : a)) : (a > l2 ? l2 : (a < l1 ? l1 : a));|b3
    og_common.hpp|limit32|return l1 > l2 ? (a > l1 ? l1 : (a < l2 ? l2 : a)) : (a > l2 ? l2 : (a < l1 ? l1 : a));|b4
    og_common.hpp|limit32|return l1 > l2 ? (a > l1 ? l1 : (a < l2 ? l2 : a)) : (a > l2 ? l2 : (a < l1 ? l1 : a));|b5
    og_common.hpp|rshift_round64|OG_DEV i64 rshift_round64(i64 a, int s) { return s == 1 ? (a >> 1) + (a & 1) : ((a >> (s - 1)) + 1) >> 1; }|b0
    og_common.hpp|sub_sat32|return s > 2147483647LL ? 2147483647 : (s < -2147483648LL ? (i32)(-2147483647 - 1) : (i32)s);|b1
    og_common.hpp|sub_sat32|return s > 2147483647LL ? 2147483647 : (s < -2147483648LL ? (i32)(-2147483647 - 1) : (i32)s);|b3
    og_decode.hpp|conceal_chunk_rfc|OG_FOR_LANES(i, audiosize * CC) (hold ? hold : pcm)[i] = 0;|b0
    og_decode.hpp|conceal_chunk_rfc|if (celt_ret >= 0) {|b1
    og_decode.hpp|conceal_chunk_rfc|if (mode == MODE_HYBRID && celt_ret >= 0) {|b3
    og_decode.hpp|conceal_chunk_rfc|if (ret) return INTERNAL_ERROR;|b0
    og_decode.hpp|conceal_chunk_rfc|return celt_ret < 0 ? celt_ret : audiosize;|b0
    og_decode.hpp|conceal_frame_rfc|if (r < 0) return r;|b0
    og_decode.hpp|decode_frame_rfc|celt_ret = celt_conceal(&st->celt, &st->loss, audiosize, CC, mode == MODE_CELT ? 0 : 17, end_band);|b0
    og_decode.hpp|decode_frame_rfc|if (celt_ret >= 0) {@2|b1
    og_decode.hpp|decode_frame_rfc|if (celt_ret >= 0) {|b1
    og_decode.hpp|decode_frame_rfc|if (len < 0 || len > 1275) return BAD_ARG;|b1
    og_decode.hpp|decode_frame_rfc|if (len < 0 || len > 1275) return BAD_ARG;|b2
    og_decode.hpp|decode_frame_rfc|if (mode == MODE_HYBRID && celt_ret >= 0) {|b3
    og_decode.hpp|decode_frame_rfc|if (r < 0) return r;@2|b0
    og_decode.hpp|decode_frame_rfc|if (r < 0) return r;|b0
    og_decode.hpp|decode_frame_rfc|if (ret) return INTERNAL_ERROR;|b0
    og_decode.hpp|decode_frame_rfc|if (transition && celt_ret >= 0) { // 2.5 ms of the concealment as it is, then 2.5 ms of cross-fade (a 2.5 ms frame: from its start)|b3
    og_decode.hpp|decode_frame_rfc|pcm[i] = (i16)(i < nmix ? sat16(v + (i32)pcm[i]) : v);|b1
    og_decode.hpp|decode_frame_rfc|return celt_ret < 0 ? celt_ret : audiosize;|b0
    og_decode.hpp|decode_frame_rfc|} else if (redundancy && celt_ret >= 0) { // CELT -> SILK|b3
    og_decode.hpp|decode_frame_wave|if (WITH_CELT && mode == MODE_SILK && prev_mode == MODE_HYBRID) {|b1
    og_decode.hpp|decode_frame_wave|if (WITH_CELT && mode == MODE_SILK && prev_mode == MODE_HYBRID) {|b3
    og_decode.hpp|decode_frame_wave|if (len < 0 || len > 1275) return BAD_ARG;|b1
    og_decode.hpp|decode_frame_wave|if (len < 0 || len > 1275) return BAD_ARG;|b2
    og_decode.hpp|decode_frame_wave|if (mode != MODE_SILK) return INTERNAL_ERROR;|b0
    og_decode.hpp|decode_frame_wave|if (q4_resume) { // the SILK half ran in the synthesis kernel: take its PCM back|b1
    og_decode.hpp|decode_frame_wave|if (r0 < 0) return r0;|b0
    og_decode.hpp|decode_frame_wave|if (ret) return INTERNAL_ERROR;|b0
    og_plc.hpp|celt_conceal|(frame_size == 120 || frame_size == 240 || frame_size == 480 || frame_size == 960))|b5
    og_plc.hpp|plc_better|return a > b || (a == b && l < bl);|b4
    og_plc.hpp|plc_pitch_search|const int p = OG_MIN(PLC_PMAX, OG_MAX(PLC_PMIN, L.scal[0]));|b1
    og_plc.hpp|plc_pitch_search|const int p = OG_MIN(PLC_PMAX, OG_MAX(PLC_PMIN, L.scal[0]));|b3
    og_plc.hpp|plc_pitch_search|const int p = OG_MIN(PLC_PMAX, OG_MAX(PLC_PMIN, L.scal[0]));|b5
    og_plc.hpp|plc_ratio_q15|if (b <= 0 || a >= b) return 32767;|b1
    og_plc.hpp|plc_search|if (LB.part[0][t] >= 0 && plc_better(LB.part[0][t], LB.part[1][t], LB.best_l[t], bnum, bden, bl)) {|b3
    og_plc.hpp|plc_shift_for|for (int t = 1; t < OG_NLANES; t++) mx = OG_MAX(mx, LB.best_l[t]);|b0
    og_plc.hpp|plc_shift_for|for (int t = 1; t < OG_NLANES; t++) mx = OG_MAX(mx, LB.best_l[t]);|b1
    og_plc.hpp|plc_shift_for|for (int t = 1; t < OG_NLANES; t++) mx = OG_MAX(mx, LB.best_l[t]);|b2
    og_silk.hpp|silk_decode_packet|const int nF = (REC_ONLY || rec) ? 1 : payload_ms == 40 ? 2 : payload_ms == 60 ? 3 : 1;|b1
    og_silk.hpp|silk_decode_packet|const int nb_subfr = (REC_ONLY || rec) ? 4 : payload_ms == 10 ? 2 : 4;|b1
    og_silk.hpp|silk_decode_packet|if (!rec && !lost && channels == 2) {|b1
    og_silk.hpp|silk_decode_packet|if (REC_ONLY || rec) { // parameters + indices (68 words laid out like SilkCtrl) from the record|b0
    og_silk.hpp|silk_decode_packet|if (REC_ONLY || rec) { // the entropy half was done by the lane-per-frame parse kernel (og_silk_parse.hpp)|b0
    og_silk.hpp|silk_decode_packet|if (channels == 2 && (s->nChannelsAPI == 1 || s->nChannelsInternal == 1)) {|b4
    og_silk.hpp|silk_decode_packet|if (conceal[n])|b0
    og_silk.hpp|silk_decode_packet|if (conceal[n])|b1
    og_silk.hpp|silk_decode_packet|if (conceal[n])|b5
    og_silk.hpp|silk_decode_packet|if (fs_kHz != 8 && fs_kHz != 12 && fs_kHz != 16) return -200;|b4
    og_silk.hpp|silk_decode_packet|if (loss) {|b0
    og_silk.hpp|silk_decode_packet|if (loss) {|b3
    og_silk.hpp|silk_decode_packet|if (loss) {|b5
    og_silk.hpp|silk_decode_packet|pulse_row[0] = rec ? rec->ch[0].pulses : PW().pulses[0];|b0
    og_silk.hpp|silk_decode_packet|pulse_row[1] = rec ? rec->ch[1].pulses : PW().pulses[1];|b0
    og_silk.hpp|silk_decode_parameters|k.Gains_Q16[j] = silk_log2lin(OG_MIN(smulwb(1907825, prev) + 2090, 3967));|b1
    og_silk.hpp|silk_div32_varQ|return lshift < 32 ? result >> lshift : 0;|b1
    og_silk.hpp|silk_inverse32_varQ|return lshift < 32 ? result >> lshift : 0;|b1
    og_silk.hpp|silk_log2lin|if (inLog_Q7 < 0) return 0;|b0
    og_silk.hpp|silk_log2lin|if (inLog_Q7 < 2048) return out + ((out * t) >> 7);|b0
    og_silk.hpp|silk_log2lin|if (inLog_Q7 >= 3967) return 2147483647;|b0
    og_silk.hpp|silk_nlsf2a|for (int i = 0; silk_inverse_pred_gain<W>(a_Q12, d) == 0 && i < 16; i++) {|b3
    og_silk.hpp|silk_params_channel|if (n == 1 && channels == 2 && dom == 0 && prev_dom == 1) {|b3
    og_silk.hpp|silk_params_channel|if (n == 1 && channels == 2 && dom == 0 && prev_dom == 1) {|b5
    og_silk.hpp|silk_params_channel|if (t.skip) return;|b0
    og_silk.hpp|silk_params_shadow|if (t.skip || !shadow) return;|b1
    og_silk_loss.hpp|silk_sum_sqr_shift|if (i < len) nrg += (u32)smulbb(x[i], x[i]) >> shft;@2|b0
    og_silk_loss.hpp|silk_sum_sqr_shift|if (i < len) nrg += (u32)smulbb(x[i], x[i]) >> shft;|b0
    og_silk_parse.hpp|silk_parse_indices|OG_KEEP(LTP_scaleIndex, condCoding == 0 ? rc_icdf_tab(rc, SILK_BLOB_ltpscale_icdf, 3) : 0);|b1
    og_silk_parse.hpp|silk_parse_indices|if (condCoding == 2 && ec_prevSignalType == 2) {|b0
    og_silk_parse.hpp|silk_parse_indices|if (condCoding == 2 && ec_prevSignalType == 2) {|b2
    og_silk_parse.hpp|silk_parse_indices|if (condCoding == 2 && ec_prevSignalType == 2) {|b3
    og_silk_parse.hpp|silk_parse_indices|if (condCoding == 2)|b0
    og_silk_parse.hpp|silk_parse_indices|if (decode_abs) {|b1
    og_silk_parse.hpp|silk_parse_lane|if (fs_kHz != 8 && fs_kHz != 12 && fs_kHz != 16) {|b4
    og_silk_parse.hpp|silk_parse_lane|if (len < 0 || len > 1275) {|b1
    og_silk_parse.hpp|silk_parse_lane|if (len < 0 || len > 1275) {|b2
    og_silk_parse.hpp|silk_parse_pulses|if (iter * 16 < frame_length) iter++;|b0
    og_silk_parse.hpp|silk_skip_pulses|if (iter * 16 < frame_length) iter++;|b0
    og_silk_parse.hpp|silk_skip_pulses|sp = rc_icdf_tab(rc, SILK_BLOB_pulses_per_block_icdf + 18 * 9 + (nl == 10), 18 - (nl == 10));|b0
    og_silk_parse.hpp|silk_skip_pulses|sp = rc_icdf_tab(rc, SILK_BLOB_pulses_per_block_icdf + 18 * 9 + (nl == 10), 18 - (nl == 10));|b2
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
EMUL = os.path.join(ROOT, "tests", "emul")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_paths.json")
SCOPE_FILES = ["og_range.hpp", "og_celt.hpp", "og_celt_math.hpp", "og_celt_bands.hpp", "og_celt_parse.hpp", "og_celt_recon.hpp",
               "og_celt_recon_pm.hpp", "og_silk.hpp", "og_silk_parse.hpp", "og_silk_loss.hpp", "og_plc.hpp", "og_decode.hpp",
               "og_common.hpp"]
LIBS = {"main": "og_emul.cpp", "tight": "og_emul_tight.cpp"}
MODE_SILK, MODE_HYBRID, MODE_CELT = 1000, 1001, 1002


def gcc_version():
    return subprocess.check_output(["g++", "-dumpfullversion"]).decode().strip()


def function_name(demangled):
    """`int og::decode_frame_wave<true>(og::StreamState*, ...)` -> decode_frame_wave; `og::RecWriter::word(unsigned int)` -> word"""
    s = demangled.replace("(anonymous namespace)::", "")
    while True:  # template arguments, innermost first
        t = re.sub(r"<[^<>]*>", "", s)
        if t == s:
            break
        s = t
    s = s.split("(")[0].strip()
    s = s.split(" ")[-1]
    return s.split("::")[-1] or demangled


class CoverageBuild:
    """Both emulation libraries with coverage counters, in a temporary directory of the tool's own."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="kernel_cov_")
        flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
        self.libs = {}
        for name, src in LIBS.items():
            d = os.path.join(self.dir, name)
            os.mkdir(d)
            obj = os.path.join(d, src[:-4] + ".o")
            subprocess.check_call(["g++", "-std=c++17", "-O0", "--coverage", "-fno-exceptions", "-fPIC", "-fwrapv", "-w", *flags,
                                   "-I", CSRC, "-c", os.path.join(EMUL, src), "-o", obj], cwd=d)
            self.libs[name] = os.path.join(d, "lib" + src[:-4] + "_cov.so")
            subprocess.check_call(["g++", "-shared", "--coverage", "-o", self.libs[name], obj], cwd=d)

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        for name in LIBS:
            d = os.path.join(self.dir, name)
            for f in os.listdir(d):
                if f.endswith(".gcda"):
                    os.remove(os.path.join(d, f))

    def decode(self, sequences, accumulate=False):
        """Decode in a child (its exit writes the counters) -> per sequence [[return code, final range, crc32 of the PCM], ...]
        of the ORACLE.  Raises when an emulation entry point differs from the oracle."""
        if not accumulate:
            self.reset()
        job = os.path.join(self.dir, "job.json")
        with open(job, "w") as f:
            json.dump(sequences, f)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", self.libs["main"], self.libs["tight"], job],
                           stdout=subprocess.PIPE)
        if p.returncode:
            raise RuntimeError("the emulation differs from the oracle (or the child failed): no census")
        return json.loads(p.stdout)

    def _gcov(self):
        """{(file, function, line number): [summed branch counts]}, {(file, function, line number): executions},
        {(file, function): entries}"""
        br, ex, fn_calls = {}, {}, {}
        self.disagree = set()
        for name, src in LIBS.items():
            d = os.path.join(self.dir, name)
            out = subprocess.check_output(["gcov", "--json-format", "--stdout", "--branch-probabilities", "--demangled-names",
                                           src[:-4] + ".o"], cwd=d, stderr=subprocess.DEVNULL)
            for fil in json.loads(out)["files"]:
                base = os.path.basename(fil["file"])
                if base not in SCOPE_FILES:
                    continue
                names, spans = {}, []  # (a line names its function by the mangled name, or not at all)
                for f in fil["functions"]:
                    names[f["name"]] = function_name(f["demangled_name"])
                    spans.append((f["start_line"], f["end_line"], names[f["name"]]))
                    k = (base, names[f["name"]])
                    fn_calls[k] = fn_calls.get(k, 0) + f["execution_count"]
                for ln in fil["lines"]:
                    n = ln["line_number"]
                    fn = names.get(ln.get("function_name")) or next((s[2] for s in spans if s[0] <= n <= s[1]), "?")
                    k = (base, fn, n)
                    ex[k] = ex.get(k, 0) + ln["count"]
                    b = [x["count"] for x in ln.get("branches") or []]
                    if not b:
                        continue
                    have = br.get(k)
                    if have is not None and len(have) != len(b):  # an instantiation folded a condition away: the ordinals do not line up
                        self.disagree.add(k)
                        continue
                    br[k] = b if have is None else [v + w for v, w in zip(have, b)]
        for k in self.disagree:  # (not summed and not reported: DISAGREE in the report's last line counts them)
            br.pop(k, None)
        return br, ex, fn_calls

    def untaken(self):
        """{key: source line number} of every untaken side on an executed in-scope line, and the set of all taken sides"""
        br, ex, _ = self._gcov()
        untaken, taken, seen = {}, set(), {}
        text = {f: open(os.path.join(CSRC, f)).read().split("\n") for f in SCOPE_FILES}
        for (f, fn, n) in sorted(br):
            line = " ".join(text[f][n - 1].split())
            if "OG_TAP" in line:
                continue
            c = seen[(f, fn, line)] = seen.get((f, fn, line), 0) + 1
            base = f"{f}|{fn}|{line}" + (f"@{c}" if c > 1 else "")
            for k, v in enumerate(br[(f, fn, n)]):
                key = f"{base}|b{k}"
                if v > 0:
                    taken.add(key)
                elif ex[(f, fn, n)] > 0:
                    untaken[key] = n
        return untaken, taken

    def never_entered(self):
        """in-scope functions that were compiled but never entered: ["file|function", ...]"""
        return sorted(f"{f}|{fn}" for (f, fn), n in self._gcov()[2].items() if n == 0)


# ---- the child: decode, and compare with the oracle -----------------------------------------------------------------------------------
def _mode_bw(toc):
    if toc & 0x80:
        bw = 1102 + ((toc >> 5) & 3)
        return MODE_CELT, (1101 if bw == 1102 else bw)
    if (toc & 0x60) == 0x60:
        return MODE_HYBRID, (1105 if toc & 0x10 else 1104)
    return MODE_SILK, 1101 + ((toc >> 5) & 3)


class Mismatch(Exception):
    """an emulation entry point and the oracle differ"""


def check_sequences(main_path, tight_path, seqs):
    """Decode every sequence with the oracle and through every emulation entry point that applies (the module's docstring), compare,
    -> per sequence [[return code, final range, crc32 of the PCM], ...] of the oracle.  Raises Mismatch."""
    import zlib
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_py
    import rfc_common as rc
    o = oracle_py.load()
    o.lib.oc_decode_fec.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int]
    main, tight = C.CDLL(main_path), C.CDLL(tight_path)
    sig = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    for lib in (main, tight):
        lib.emu_state_size.restype = C.c_int
        lib.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
        lib.emu_decode_frame.argtypes = sig
    main.emu_decode_frame_single.argtypes = main.emu_decode_frame_roles.argtypes = sig
    main.emu_decode_frame_shadowed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint] + sig[1:]
    main.emu_shadow_vs_state.argtypes = [C.c_void_p, C.c_void_p]
    main.emu_decode_frame_rfc.argtypes = main.emu_decode_frame_rfc_fec.argtypes = sig + [C.c_int]
    st = C.create_string_buffer(max(main.emu_state_size(), tight.emu_state_size()))

    def fail(*what):
        raise Mismatch(" ".join(str(w) for w in what))

    def reference_mode(i, seq):
        ch = seq["channels"]
        pkts = [bytes.fromhex(h) for h in seq["packets"]]
        d = o.decoder(ch)
        d.init()
        rows, refs = [], []
        for p in pkts:
            ref, r = d.decode(p) if p else d.conceal(960)  # (an empty packet: one pass of the reference's empty-packet branch)
            rows.append([r, o.lib.oc_decoder_final_range(d.h), zlib.crc32(ref[:max(r, 0)].tobytes())])
            refs.append((r, ref[:960].reshape(-1).copy()))
        routes = ["split", "single", "shadowed"] + (["roles"] if any(p and p[0] & 0x80 for p in pkts) else [])
        routes += ["tight"] if pkts and all(p and p[0] & 0x80 for p in pkts) else []
        for route in routes:
            lib = tight if route == "tight" else main
            lib.emu_stream_init(st, ch)
            shadow, epoch = C.create_string_buffer(128), 1
            last = (0, 1104, ch)  # (mode 0: the empty frame of a stream that has had no packet yet)
            for f, p in enumerate(pkts):
                if p:
                    (m, bw), pch, body = _mode_bw(p[0]), 2 if p[0] & 4 else 1, p[1:]
                    last = (m, bw, pch)
                else:  # a frame of no bytes with the last accepted packet's mode, bandwidth and channels
                    (m, bw, pch), body = last, b""
                buf = np.zeros((960, ch), dtype=np.int16)
                if route == "single":
                    r2 = main.emu_decode_frame_single(st, body, len(body), m, bw, pch, buf.ctypes.data)
                elif route == "roles" and m == MODE_CELT:
                    r2 = main.emu_decode_frame_roles(st, body, len(body), m, bw, pch, buf.ctypes.data)
                    epoch += 1
                elif route == "shadowed" and m != MODE_CELT:
                    r2 = main.emu_decode_frame_shadowed(st, shadow, epoch, body, len(body), m, bw, pch, buf.ctypes.data)
                    if r2 > 0 and main.emu_shadow_vs_state(st, shadow) != 0:
                        fail("shadow differs from the state", i, f)
                else:
                    r2 = lib.emu_decode_frame(st, body, len(body), m, bw, pch, buf.ctypes.data)
                    epoch += 1
                if route == "tight" and r2 == -999:
                    break
                r, ref = refs[f]
                if r2 != r:
                    fail(route, "return code", i, f, p[:1].hex(), r, r2)
                if r > 0:
                    ncmp = 960 * pch if (m == MODE_SILK and pch < ch) else 960 * ch
                    if not np.array_equal(buf.reshape(-1)[:ncmp], ref[:ncmp]):
                        fail(route, "PCM", i, f, p[:1].hex())
        return rows

    def rfc_mode(i, seq):
        ch = seq["channels"]
        pkts = [bytes.fromhex(h) for h in seq["packets"]]
        fec = set(seq.get("fec") or ())
        d = o.decoder(ch)
        d.init()
        d.set_rfc(True)
        main.emu_stream_init(st, ch)
        last, rows = None, []  # last: (frame count, frame duration, mode, bandwidth, packet channels) of the last packet framed

        def frames(pays, fs, m, bw, pch):
            got = np.zeros((len(pays) * fs, ch), dtype=np.int16)
            total = 0
            for k, pay in enumerate(pays):
                buf = np.zeros((fs, ch), dtype=np.int16)
                rr = main.emu_decode_frame_rfc(st, pay, len(pay), m, bw, pch, buf.ctypes.data, fs)
                if rr < 0:
                    return rr, got
                got[k * fs:(k + 1) * fs] = buf
                total += rr
            return total, got

        for f, p in enumerate(pkts):
            if p and f in fec and rc.frame_payloads(o, p) is not None:
                total, pieces, use = rc.fec_plan((last[0], last[1], last[2]) if last else None, p[0], ch)
                lfs, lm, lbw, lpch = (last[1], last[2], last[3], last[4]) if last else (960, MODE_CELT, 1105, ch)
                mode_now = d.prev_mode()
                ref = np.zeros((5760, ch), dtype=np.int16)
                r = o.lib.oc_decode_fec(d.h, p, len(p), ref.ctypes.data, total)
                at, spans, r2 = 0, [], 0
                got = np.zeros((total, ch), dtype=np.int16)
                for w in pieces:
                    buf = np.zeros((w, ch), dtype=np.int16)
                    rr = main.emu_decode_frame_rfc(st, b"", 0, lm, lbw, lpch, buf.ctypes.data, w)
                    if rr != w:
                        fail("fec: concealment piece", i, f, rr, w)
                    got[at:at + w] = buf
                    spans.append((at, w, 0, lm, lpch))
                    at += w
                r2 = at
                if use:
                    (m, bw), fs, pch = _mode_bw(p[0]), rc.dur(p[0]), 2 if p[0] & 4 else 1
                    pay = rc.frame_payloads(o, p)[0]
                    buf = np.zeros((fs, ch), dtype=np.int16)
                    rr = main.emu_decode_frame_rfc_fec(st, pay, len(pay), m, bw, pch, buf.ctypes.data, fs)
                    got[at:at + fs] = buf
                    spans.append((at, fs, len(pay), m, pch))
                    at += fs
                    r2 = rr if rr < 0 else at
                if r != r2:
                    fail("fec: return code", i, f, hex(p[0]), r, r2)
                for (a0, w, ln, mm, pc) in spans if r > 0 else []:
                    if not rc.same_pcm(got[a0:a0 + w], ref[a0:a0 + w], w, [ln], mode_now, mm, pc, ch)[0]:
                        fail("fec: PCM", i, f, hex(p[0]), a0)
                    if ln > 1:
                        mode_now = mm
            before = d.prev_mode()
            if not p:
                cnt, fs, m, bw, pch = last if last else (1, 960, MODE_CELT, 1105, ch)
                pays, label = None, "lost"
                ref, r = d.conceal(cnt * fs)
                ref = ref[:max(r, 0)].copy()
                got, r2 = np.zeros((cnt * fs, ch), dtype=np.int16), 0
                for w in rc.conceal_pieces(cnt * fs, fs):
                    buf = np.zeros((w, ch), dtype=np.int16)
                    rr = main.emu_decode_frame_rfc(st, b"", 0, m, bw, pch, buf.ctypes.data, w)
                    if rr < 0:
                        r2 = rr
                        break
                    got[r2:r2 + w] = buf
                    r2 += rr
                lens = [0] * cnt
            else:
                ref, r = d.decode(p)
                ref = ref[:max(r, 0)].copy()
                pays, label = rc.frame_payloads(o, p), hex(p[0])
                if pays is None:
                    if r >= 0:
                        fail("framing disagrees", i, f, label, r)
                    rows.append([r, o.lib.oc_decoder_final_range(d.h), 0])
                    continue
                (m, bw), fs, pch = _mode_bw(p[0]), rc.dur(p[0]), 2 if p[0] & 4 else 1
                last = (len(pays), fs, m, bw, pch)
                r2, got = frames(pays, fs, m, bw, pch)
                lens = [len(x) for x in pays]
            rows.append([r, o.lib.oc_decoder_final_range(d.h), zlib.crc32(ref.tobytes())])
            if r != r2:
                fail("rfc: return code", i, f, label, r, r2)
            if r > 0 and not rc.same_pcm(got, ref, fs, lens, before, m, pch, ch)[0]:
                fail("rfc: PCM", i, f, label)
        return rows

    return [rfc_mode(i, seq) if seq.get("rfc") else reference_mode(i, seq) for i, seq in enumerate(seqs)]


def worker(main_path, tight_path, job):
    try:
        res = check_sequences(main_path, tight_path, json.load(open(job)))
    except Mismatch as e:
        print("MISMATCH", e, file=sys.stderr)
        sys.exit(3)
    json.dump(res, sys.stdout)


# ---- the baseline: everything the suite already decodes ----------------------------------------------------------------------------
def _seq(channels, packets, rfc=False, fec=None):
    s = {"channels": channels, "packets": [bytes(p).hex() for p in packets], "rfc": rfc}
    if fec:
        s["fec"] = sorted(fec)
    return s


def corpus_sequences(names=("rare_paths.json", "saturation_paths.json")):
    seqs = []
    for name in names:
        for e in json.load(open(os.path.join(ROOT, "tests", "golden", name)))["entries"]:
            s = {"channels": e["channels"], "packets": e["packets"], "rfc": bool(e.get("rfc"))}
            if e.get("fec"):
                s["fec"] = e["fec"]
            seqs.append(s)
    return seqs


def crafted_sequences():
    """the crafted batches of the five directed test modules, through the modules' own builders"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_anti_collapse_cells as ac
    import test_fill_windows_emul as fw
    import test_gpu_comb_history as cbh
    import test_gpu_fill_windows as gfw
    import test_gpu_synth_stages as ss
    seqs = []
    for name in cbh.BATCHES:  # packets[frame][stream], a stereo decoder
        pk = cbh._reference(name)[0]
        seqs += [_seq(2, [pk[f][s] for f in range(len(pk))]) for s in range(len(pk[0]))]
    for L in fw.SIZES:  # payloads [frames, n, L]
        pay = fw.reference(L)[0]
        seqs += [_seq(2, [bytes([fw.TOC]) + pay[f, s].tobytes() for f in range(pay.shape[0])]) for s in range(pay.shape[1])]
    pay = gfw._hybrid_reference()[0]
    seqs += [_seq(2, [bytes([gfw.HYBRID[1]]) + pay[f, s].tobytes() for f in range(pay.shape[0])]) for s in range(pay.shape[1])]
    for name, (n, channels, toc) in ss.BATCHES.items():
        pk = ss._reference(name)[0]
        seqs += [_seq(channels, [pk[f][s] for f in range(len(pk))]) for s in range(n)]
    for name, (n, channels, toc, L, _) in ac.BATCHES.items():  # (test_gpu_transient_frames.py runs these very batches)
        pay = ac.reference(name)[0]
        seqs += [_seq(channels, [bytes([toc]) + pay[f, s].tobytes() for f in range(pay.shape[0])]) for s in range(n)]
    return seqs


def bench_shape_sequences(streams=256):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    import test_gpu_bench_shapes as bs
    from conftest import load_pkg
    pkg = load_pkg()
    seqs = []
    for name in ("celt_fb_stereo_64k", "silk_nb_stereo_64k", "hybrid_fb_stereo_256k"):
        toc, L = bench.WORKLOADS[name][:2]
        pay = pkg.lcg_payloads(streams, bs.STEPS, L, seed_base=0xBE4C0000 + toc)
        seqs += [_seq(2, [bytes([toc]) + pay[f, s].tobytes() for f in range(bs.STEPS)]) for s in range(streams)]
    return seqs


def rfc_plan_sequences():
    """Every stream of every plan of tests/test_gpu_rfc.py, both channel counts: rfc_common.rfc_plan and draw_step are what that test
    walks too, so the packets are the ones it decodes."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_py
    import rfc_common as rc
    o = oracle_py.load()
    seqs = []
    for name in rc.RFC_PLANS:
        for channels in (2, 1):
            plan = rc.rfc_plan(name)
            rng = np.random.default_rng(plan["seed"] + channels)
            n = plan["streams"]
            pks, fec = [[] for _ in range(n)], [set() for _ in range(n)]
            for f in range(plan["steps"]):
                pk, who = rc.draw_step(o, plan, rng, f, channels)
                for s in range(n):
                    pks[s].append(pk[s])
                for s in who:
                    fec[s].add(f)
            seqs += [_seq(channels, pks[s], rfc=True, fec=fec[s]) for s in range(n)]
    return seqs


def empty_packet_sequences(streams=80, frames=12, seed=5):
    """reference-mode walks with empty packets, the kind tests/test_empty_packets.py decodes on every entry point: an empty packet
    first in half of the streams (the mode-0 frame), later with probability 0.3, once or twice in a row; the configurations and
    payload lengths of that test"""
    import numpy as np
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(streams):
        channels, pkts = int(rng.integers(1, 3)), []
        for f in range(frames):
            if rng.random() < (0.5 if f == 0 else 0.3):
                pkts += [b""] * int(rng.integers(1, 3))
            else:
                toc = int(rng.choice([1, 5, 9, 13, 15, 19, 23, 31])) << 3 | (4 if rng.random() < 0.7 else 0)
                pkts.append(bytes([toc]) + rng.integers(0, 256, int(rng.choice([0, 1, 2, 30, 80, 200])), dtype=np.uint8).tobytes())
        seqs.append(_seq(channels, pkts))
    return seqs


def baseline_sequences():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_branches as ob
    seqs = [dict(s, rfc=False) for s in ob.baseline_sequences()]
    return seqs + corpus_sequences() + crafted_sequences() + bench_shape_sequences() + rfc_plan_sequences() + empty_packet_sequences()


def fixture_sequences(entries):
    out = []
    for e in entries:
        s = {"channels": e["channels"], "packets": e["packets"], "rfc": bool(e.get("rfc"))}
        if e.get("fec"):
            s["fec"] = e["fec"]
        out.append(s)
    return out


def decode_in_chunks(cov, seqs, chunk=4000):
    """one child per chunk (a job file and a result stay small), the counters accumulate"""
    cov.reset()
    res = []
    for k in range(0, len(seqs), chunk):
        res += cov.decode(seqs[k:k + chunk], accumulate=True)
    return res


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3], sys.argv[4])
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--baseline", action="store_true")
    g.add_argument("--corpus", action="store_true")
    g.add_argument("--json")
    ap.add_argument("--entry", type=int, help="with --corpus: this entry alone")
    a = ap.parse_args()
    claimed = None
    if a.baseline:
        seqs = baseline_sequences()
    elif a.json:
        seqs = json.load(open(a.json))
    else:
        fx = json.load(open(FIXTURE))
        ents = fx["entries"] if a.entry is None else [fx["entries"][a.entry]]
        seqs = fixture_sequences(ents)
        claimed = sorted({k for e in ents for k in e["keys"]})
    with CoverageBuild() as cov:
        decode_in_chunks(cov, seqs)
        untaken, taken = cov.untaken()
        never = cov.never_entered()
    if claimed is not None and a.entry is not None:
        for k in claimed:
            print(("TAKEN    " if k in taken else "NOT TAKEN") + " " + k)
        return 0 if all(k in taken for k in claimed) else 1
    for k in sorted(untaken):
        print(f"{untaken[k]:5d}  {k}")
    for k in never:
        print(f"never  {k}")
    print(f"{len(untaken)} untaken sides on executed lines, {len(taken)} taken, {len(never)} functions never entered, "
          f"{len(cov.disagree)} lines left out because their instantiations differ in branch count; g++ {gcc_version()}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
