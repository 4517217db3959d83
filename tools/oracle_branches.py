#!/usr/bin/env python3
"""Which branch sides of the CPU oracle's reference-mode decode does a set of packet sequences leave untaken?  CPU only.

The tool builds oracle/*.c with `gcc -O0 --coverage` into a temporary directory (never into oracle/; oracle/Makefile is not
used), decodes the sequences in a child process (a fresh decoder per sequence, packets in order, reference mode), reads
`gcov --json-format --branch-probabilities` and reports every EXECUTED line of an in-scope function that has a branch side with
count 0.  A side is keyed by

    file | function | stripped source text of the line [@n for the n-th line with that text in the function] | b<k>

with k the ordinal of the branch on that line in gcov's order (-O0: two per condition, in source order: b0 / b1 are the first
condition's jump and fall-through, b2 / b3 the second's, ...).  Line numbers are not part of a key: they move.

Scope: the functions of the reference-mode decode in oc_celt.c, oc_celt_math.c, oc_silk.c and oc_range.c.  RFC mode, both
concealments, the oc_test_* entry points and the stage taps are out of scope: EXCLUDED_FUNCTIONS below, plus any line whose text
names `taps`.

    python tools/oracle_branches.py --baseline            # the suite's random payload families (BASELINE below)
    python tools/oracle_branches.py --corpus [--entry N]  # tests/golden/rare_paths.json, or one entry of it alone:
                                                          # prints the claimed keys and whether each is taken
    python tools/oracle_branches.py --json FILE           # sequences from FILE: [{"channels": c, "packets": [hex, ...]}, ...]

BASELINE -- the report at the commit before the corpus existed, for the suite's random payloads: 512 streams x 6 frames of
lcg_payloads for each (TOC, length) of tests/test_gpu_stage_taps.py, tests/test_gpu_modes.py and tests/test_gpu_celt.py
(BASELINE_SETS below) and make_walk walks (tests/test_gpu_pipeline.py) of 1024 streams x 14 packets, mono and stereo.
The same list is data in tests/golden/rare_paths.json under "baseline" (regenerate: tests/golden/make_rare_paths.py
--baseline), together with the three sets every side of it belongs to: "reached" by the corpus, "unreachable" in reference
mode (with the reason), "open".  tests/test_rare_paths.py checks the report over the corpus against them, and this list
against the fixture's.  The 102 sides:

    oc_celt.c|anti_collapse|if (LM == 3) r = (i16)m16_q14(23170, OC_MIN(23169, r));|b1
    oc_celt.c|compute_theta|if (*b > 2 << BITRES && cx->remaining_bits > 2 << BITRES)|b3
    oc_celt.c|compute_theta|} else if (stereo) {|b1
    oc_celt.c|denormalise|i16 lg = (i16)(lg32 > 32767 ? 32767 : (lg32 < -32768 ? -32768 : lg32)), g;|b3
    oc_celt.c|oc_celt_decode|anti_collapse_rsv = transient && LM >= 2 && bits >= ((LM + 2) << BITRES) ? (1 << BITRES) : 0;|b3
    oc_celt.c|oc_celt_decode|const i16 inc = st->loss_count < 10 ? (i16)(M * 1) : 1024; /* M * QCONST16(0.001f, DB_SHIFT), QCONST16(1.f, DB_SHIFT) */|b1
    oc_celt.c|oc_celt_decode|for (LM = 0; LM <= 3; LM++)|b1
    oc_celt.c|oc_celt_decode|for (i = end; i < NB; i++) {|b0
    oc_celt.c|oc_celt_decode|if (LM > 3) return OC_CELT_BAD_ARG; /* celt.cpp:2211 */|b0
    oc_celt.c|oc_celt_decode|if (oc_rc_tell(rc) > 8 * (i32)rc->storage) return OC_INTERNAL_ERROR;|b0
    oc_celt.c|oc_celt_decode|if (rc->storage > 1275 || pcm == NULL) return OC_CELT_BAD_ARG; /* :2216 */|b1
    oc_celt.c|oc_celt_decode|if (rc->storage > 1275 || pcm == NULL) return OC_CELT_BAD_ARG; /* :2216 */|b2
    oc_celt.c|oc_celt_decode|int c, i, N, LM, M, start = st->start_band, end = (st->end_band > 0 && st->end_band <= NB) ? st->end_band : NB, effEnd = end;|b1
    oc_celt.c|oc_celt_decode|int c, i, N, LM, M, start = st->start_band, end = (st->end_band > 0 && st->end_band <= NB) ? st->end_band : NB, effEnd = end;|b3
    oc_celt.c|quant_band_n1|if (lowband_out) lowband_out[0] = X[0] >> 4;|b1
    oc_celt.c|stereo_merge|if (kl < 7) kl = 7;|b0
    oc_celt.c|stereo_merge|if (kr < 7) kr = 7;|b0
    oc_celt_math.c|oc_comb_filter|if (x != y) memmove(y + overlap, x + overlap, (N - overlap) * sizeof(*y));|b0
    oc_celt_math.c|oc_comb_filter|if (x != y) memmove(y, x, N * sizeof(*y));|b0
    oc_celt_math.c|oc_cos_norm|if (x & 0x7fff) {|b1
    oc_celt_math.c|oc_cos_norm|if (x < (1 << 15)) return cos_pi_2((i16)x);|b1
    oc_celt_math.c|oc_cos_norm|if (x > (1 << 16)) x = (1 << 17) - x;|b0
    oc_celt_math.c|oc_exp2|if (integer > 14) return 0x7f000000;|b0
    oc_celt_math.c|oc_exp_rotation|if (dir < 0) {|b1
    oc_celt_math.c|oc_fft|switch (fac[2 * i]) {|b4
    oc_celt_math.c|oc_sqrt|if (x == 0) return 0;|b0
    oc_celt_math.c|oc_sqrt|if (x >= 1073741824) return 32767;|b0
    oc_silk.c|cng|if (c->lossCnt == 0 && c->prevSignalType == 0) {|b1
    oc_silk.c|cng|if (c->lossCnt) {|b0
    oc_silk.c|decode_core|if (c->lossCnt && c->prevSignalType == 2 && c->idx.signalType != 2 && k < 2) {|b0
    oc_silk.c|decode_core|if (c->lossCnt && c->prevSignalType == 2 && c->idx.signalType != 2 && k < 2) {|b2
    oc_silk.c|decode_core|if (c->lossCnt && c->prevSignalType == 2 && c->idx.signalType != 2 && k < 2) {|b3
    oc_silk.c|decode_core|if (c->lossCnt && c->prevSignalType == 2 && c->idx.signalType != 2 && k < 2) {|b4
    oc_silk.c|decode_core|if (c->lossCnt && c->prevSignalType == 2 && c->idx.signalType != 2 && k < 2) {|b5
    oc_silk.c|decode_core|if (c->lossCnt && c->prevSignalType == 2 && c->idx.signalType != 2 && k < 2) {|b6
    oc_silk.c|decode_core|if (c->lossCnt && c->prevSignalType == 2 && c->idx.signalType != 2 && k < 2) {|b7
    oc_silk.c|decode_frame|if (lostFlag == 0 || (lostFlag == 2 && c->LBRR_flags[c->nFramesDecoded] == 1)) {|b0
    oc_silk.c|decode_frame|if (lostFlag == 0 || (lostFlag == 2 && c->LBRR_flags[c->nFramesDecoded] == 1)) {|b2
    oc_silk.c|decode_frame|if (lostFlag == 0 || (lostFlag == 2 && c->LBRR_flags[c->nFramesDecoded] == 1)) {|b3
    oc_silk.c|decode_frame|if (lostFlag == 0 || (lostFlag == 2 && c->LBRR_flags[c->nFramesDecoded] == 1)) {|b4
    oc_silk.c|decode_frame|if (lostFlag == 0 || (lostFlag == 2 && c->LBRR_flags[c->nFramesDecoded] == 1)) {|b5
    oc_silk.c|decode_indices|contour = c->nb_subfr == 4 ? rom_silk_pitch_contour_icdf : rom_silk_pitch_contour_10ms_icdf;|b1
    oc_silk.c|decode_indices|contour = c->nb_subfr == 4 ? rom_silk_pitch_contour_nb_icdf : rom_silk_pitch_contour_10ms_nb_icdf;|b1
    oc_silk.c|decode_indices|if (c->nb_subfr == 4)|b1
    oc_silk.c|decode_indices|if (condCoding == 0)|b1
    oc_silk.c|decode_indices|if (condCoding == 2 && c->ec_prevSignalType == 2) {|b0
    oc_silk.c|decode_indices|if (condCoding == 2 && c->ec_prevSignalType == 2) {|b2
    oc_silk.c|decode_indices|if (condCoding == 2 && c->ec_prevSignalType == 2) {|b3
    oc_silk.c|decode_indices|if (condCoding == 2)|b0
    oc_silk.c|decode_indices|if (decode_abs) {|b1
    oc_silk.c|decode_parameters|ct->Gains_Q16[k] = log2lin(OC_MIN(smulwb(1907825, c->LastGainIndex) + 2090, 3967));|b1
    oc_silk.c|decode_parameters|if (c->lossCnt) { /* silk.cpp:860-864: after a packet loss do BWE of the LPC coefficients (BWE_AFTER_LOSS_Q16) */|b0
    oc_silk.c|decode_parameters|if (k == 0 && condCoding != 2)|b3
    oc_silk.c|decode_pitch|if (nb_subfr == 4) { cbk = (const signed char *)rom_silk_lags_stage2; cbk_size = 11; }|b1
    oc_silk.c|decode_pitch|if (nb_subfr == 4) { cbk = (const signed char *)rom_silk_lags_stage3; cbk_size = 34; }|b1
    oc_silk.c|decode_pulses|if (iter * 16 < frame_length) iter++;|b0
    oc_silk.c|decode_pulses|sum_pulses[i] = oc_rc_icdf(rc, rom_silk_pulses_per_block_icdf + 18 * 9 + (nLshifts[i] == 10), 8);|b0
    oc_silk.c|div32_varQ|return lshift < 32 ? result >> lshift : 0;|b1
    oc_silk.c|inverse32_varQ|return lshift < 32 ? result >> lshift : 0;|b1
    oc_silk.c|inverse_pred_gain|if (tmp64 > INT32_MAX || tmp64 < INT32_MIN) return 0;@2|b1
    oc_silk.c|inverse_pred_gain|if (tmp64 > INT32_MAX || tmp64 < INT32_MIN) return 0;@2|b2
    oc_silk.c|inverse_pred_gain|if (tmp64 > INT32_MAX || tmp64 < INT32_MIN) return 0;|b1
    oc_silk.c|inverse_pred_gain|if (tmp64 > INT32_MAX || tmp64 < INT32_MIN) return 0;|b2
    oc_silk.c|log2lin|if (inLog_Q7 < 0) return 0;|b0
    oc_silk.c|log2lin|if (inLog_Q7 < 2048)|b0
    oc_silk.c|log2lin|if (inLog_Q7 >= 3967) return INT32_MAX;|b0
    oc_silk.c|lpc_fit|for (i = 0; i < 10; i++) {|b1
    oc_silk.c|lpc_fit|if (i == 10) {|b0
    oc_silk.c|nlsf2a|for (i = 0; inverse_pred_gain(a_Q12, d) == 0 && i < 16; i++) {|b3
    oc_silk.c|nlsf_stabilize|NLSF_Q15[0] = (i16)OC_MAX((i32)NLSF_Q15[0], (i32)NDeltaMin_Q15[0]);|b1
    oc_silk.c|oc_silk_decode_ex|condCoding = (i > 0 && s->ch[n].LBRR_flags[i - 1]) ? 2 : 0;|b0
    oc_silk.c|oc_silk_decode_ex|condCoding = (i > 0 && s->ch[n].LBRR_flags[i - 1]) ? 2 : 0;|b2
    oc_silk.c|oc_silk_decode_ex|condCoding = (i > 0 && s->ch[n].LBRR_flags[i - 1]) ? 2 : 0;|b3
    oc_silk.c|oc_silk_decode_ex|if ((lostFlag == 0 && s->ch[1].VAD_flags[s->ch[0].nFramesDecoded] == 0) |||b1
    oc_silk.c|oc_silk_decode_ex|if ((lostFlag == 0 && s->ch[1].VAD_flags[s->ch[0].nFramesDecoded] == 0) |||b4
    oc_silk.c|oc_silk_decode_ex|if (FrameIndex <= 0)|b1
    oc_silk.c|oc_silk_decode_ex|if (channels == 2 && (s->nChannelsAPI == 1 || s->nChannelsInternal == 1)) {|b4
    oc_silk.c|oc_silk_decode_ex|if (first)|b1
    oc_silk.c|oc_silk_decode_ex|if (fs_kHz_dec != 8 && fs_kHz_dec != 12 && fs_kHz_dec != 16) return -200;|b4
    oc_silk.c|oc_silk_decode_ex|if (lostFlag != 1 && s->ch[0].nFramesDecoded == 0) {|b1
    oc_silk.c|oc_silk_decode_ex|if (lostFlag != 1 && s->ch[0].nFramesDecoded == 0) {|b3
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 0 || (lostFlag == 2 && s->ch[0].LBRR_flags[s->ch[0].nFramesDecoded] == 1)) {|b0
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 0 || (lostFlag == 2 && s->ch[0].LBRR_flags[s->ch[0].nFramesDecoded] == 1)) {|b2
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 0 || (lostFlag == 2 && s->ch[0].LBRR_flags[s->ch[0].nFramesDecoded] == 1)) {|b3
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 0 || (lostFlag == 2 && s->ch[0].LBRR_flags[s->ch[0].nFramesDecoded] == 1)) {|b4
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 0 || (lostFlag == 2 && s->ch[0].LBRR_flags[s->ch[0].nFramesDecoded] == 1)) {|b5
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 0)@2|b1
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 0)|b1
    oc_silk.c|oc_silk_decode_ex|if (lostFlag == 1) /* silk.cpp:1772-1776: no gain clamping across a loss */|b0
    oc_silk.c|oc_silk_decode_ex|if (s->ch[0].nFramesDecoded == 0) {|b1
    oc_silk.c|oc_silk_decode_ex|if (s->ch[n].nFramesPerPacket == 1)|b1
    oc_silk.c|oc_silk_decode_ex|int fs_kHz_dec = internal_hz ? (internal_hz >> 10) + 1 : s->ch[0].fs_kHz;|b1
    oc_silk.c|oc_silk_decode_ex|s->ch[n].nFramesPerPacket = payload_ms == 40 ? 2 : payload_ms == 60 ? 3 : 1;|b1
    oc_silk.c|oc_silk_decode_ex|s->ch[n].nFramesPerPacket = payload_ms == 40 ? 2 : payload_ms == 60 ? 3 : 1;|b2
    oc_silk.c|oc_silk_decode_ex|s->ch[n].nb_subfr = payload_ms == 10 ? 2 : 4;|b0
    oc_silk.c|plc_glue_frames|if (c->lossCnt) {|b0
    oc_silk.c|plc_glue_frames|if (c->plc.last_frame_lost) {|b0
    oc_silk.c|plc_update|if (j == c->nb_subfr) break;|b0
    oc_silk.c|plc|if (lost) {|b0
    oc_silk.c|set_fs|if (c->fs_kHz != fs_kHz || c->fs_API_hz != 48000) {|b2
    oc_silk.c|set_fs|if (c->fs_kHz != fs_kHz || frame_length != c->frame_length) {|b2
    oc_silk.c|set_fs|if (c->fs_kHz != fs_kHz) {|b1
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
ALL_SRCS = ["oc_range.c", "oc_celt_math.c", "oc_celt.c", "oc_packet.c", "oc_silk.c", "oc_batch.c", "oc_output.c"]
SCOPE_FILES = ["oc_celt.c", "oc_celt_math.c", "oc_silk.c", "oc_range.c"]
CFLAGS = ["-O0", "--coverage", "-fPIC", "-fwrapv", "-fno-strict-aliasing", "-w"]

# Out of scope: RFC mode only, the two concealments (CELT: pitch-based and noise-based; SILK: PLC and what only a loss runs),
# test-only entry points, stage taps.
EXCLUDED_FUNCTIONS = [
    # oc_celt.c: concealment of lost frames (RFC mode) and its helpers
    "oc_celt_decode_lost", "celt_decode_lost_pitch", "plc_pitch_search", "plc_lpc", "plc_ratio_q15", "ilog64", "isqrt64",
    "mul32_q31", "sat16_64",
    # entry points for unit tests of single stages: every oc_test_* function (is_excluded)
    # oc_silk.c: packet-loss concealment (RFC mode: lostFlag is never 1 in reference mode), taps
    "plc_conceal", "oc_silk_taps_enable", "oc_silk_taps_copy", "cng_reset", "plc_reset",
]

BASELINE_SETS = [  # (TOC, payload length); the decoder has the TOC's channel count
    (0xFC, 160), (0xFC, 60), (0xFC, 400),                                    # test_gpu_stage_taps.py, test_gpu_celt.py: CELT FB stereo
    (0x0C, 40), (0x4C, 70), (0x48, 60), (0x7C, 120), (0x78, 90),             # test_gpu_stage_taps.py: SILK NB / WB, hybrid FB
    (0x2C, 60), (0x4C, 80), (0x48, 70), (0x6C, 100), (0x08, 30),             # test_gpu_modes.py: SILK MB / WB, hybrid SWB, NB mono
]


def is_excluded(function):
    return function in EXCLUDED_FUNCTIONS or function.startswith("oc_test_")


class CoverageBuild:
    """The oracle with coverage counters, in a temporary directory of its own."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="oracle_cov_")
        for src in ALL_SRCS:
            subprocess.check_call(["gcc", *CFLAGS, "-I", ORACLE, "-c", os.path.join(ORACLE, src), "-o",
                                   os.path.join(self.dir, src[:-2] + ".o")], cwd=self.dir)
        self.lib = os.path.join(self.dir, "liboc_cov.so")
        subprocess.check_call(["gcc", "-shared", "--coverage", "-o", self.lib] + [src[:-2] + ".o" for src in ALL_SRCS], cwd=self.dir)

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        for f in os.listdir(self.dir):
            if f.endswith(".gcda"):
                os.remove(os.path.join(self.dir, f))

    def decode(self, sequences, accumulate=False):
        """Decode in a child (its exit writes the counters) -> per sequence [[return code, final range, crc32 of the PCM], ...]"""
        if not accumulate:
            self.reset()
        job = os.path.join(self.dir, "job.json")
        with open(job, "w") as f:
            json.dump(sequences, f)
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--worker", self.lib, job])
        return json.loads(out)

    def untaken(self):
        """{key: source line number} of every untaken side on an executed in-scope line, and the set of all taken sides"""
        untaken, taken = {}, set()
        for src in SCOPE_FILES:
            out = subprocess.check_output(["gcov", "--json-format", "--stdout", "--branch-probabilities", src[:-2] + ".o"],
                                          cwd=self.dir, stderr=subprocess.DEVNULL)
            text = open(os.path.join(ORACLE, src)).read().split("\n")
            for fil in json.loads(out)["files"]:
                if os.path.basename(fil["file"]) != src:
                    continue
                seen = {}
                for ln in sorted(fil["lines"], key=lambda l: l["line_number"]):
                    br = ln.get("branches") or []
                    fn = ln.get("function_name", "?")
                    if not br or is_excluded(fn):
                        continue
                    line = " ".join(text[ln["line_number"] - 1].split())
                    if "taps" in line:
                        continue
                    n = seen[(fn, line)] = seen.get((fn, line), 0) + 1
                    base = f"{src}|{fn}|{line}" + (f"@{n}" if n > 1 else "")
                    for k, b in enumerate(br):
                        key = f"{base}|b{k}"
                        if b["count"] > 0:
                            taken.add(key)
                        elif ln["count"] > 0:
                            untaken[key] = ln["line_number"]
        return untaken, taken


def worker(lib_path, job):
    import zlib
    lib = C.CDLL(lib_path)
    lib.oc_decoder_create.restype = C.c_void_p
    lib.oc_decoder_create.argtypes = [C.c_int]
    lib.oc_decoder_destroy.argtypes = [C.c_void_p]
    lib.oc_decode.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int]
    lib.oc_decoder_final_range.argtypes = [C.c_void_p]
    lib.oc_decoder_final_range.restype = C.c_uint32
    res = []
    for seq in json.load(open(job)):
        ch = seq["channels"]
        d = lib.oc_decoder_create(ch)
        buf = C.create_string_buffer((5760 + 960) * ch * 2)
        rows = []
        for hx in seq["packets"]:
            p = bytes.fromhex(hx)
            r = lib.oc_decode(d, p, len(p), buf, 5760)
            rows.append([r, lib.oc_decoder_final_range(d), zlib.crc32(buf.raw[:max(r, 0) * ch * 2])])
        lib.oc_decoder_destroy(d)
        res.append(rows)
    json.dump(res, sys.stdout)


def baseline_sequences(streams=512, frames=6, walk_streams=1024, walk_frames=14):
    """The suite's random payload families as sequences (needs numpy and the package's lcg_payloads; no GPU)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_pkg
    from test_gpu_pipeline import make_walk
    pkg = load_pkg()
    seqs = []
    for toc, L in BASELINE_SETS:
        pay = pkg.lcg_payloads(streams, frames, L, seed_base=0x7A95 + L + toc)
        for s in range(streams):
            seqs.append({"channels": 2 if toc & 4 else 1, "packets": [(bytes([toc]) + pay[f, s].tobytes()).hex() for f in range(frames)]})
    for channels in (1, 2):
        arena, offs, plen, _, _ = make_walk(np.random.default_rng(0xC0FFEE + channels), walk_streams, walk_frames, channels)
        for s in range(walk_streams):
            seqs.append({"channels": channels,
                         "packets": [arena[offs[f, s]:offs[f, s] + plen[f, s]].tobytes().hex() for f in range(walk_frames)]})
    return seqs


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3])
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
        fx = json.load(open(os.path.join(ROOT, "tests", "golden", "rare_paths.json")))
        ents = fx["entries"] if a.entry is None else [fx["entries"][a.entry]]
        seqs = [{"channels": e["channels"], "packets": e["packets"]} for e in ents]
        claimed = sorted({k for e in ents for k in e["keys"]})
    with CoverageBuild() as cov:
        cov.decode(seqs)
        untaken, taken = cov.untaken()
    if claimed is not None and a.entry is not None:
        for k in claimed:
            print(("TAKEN    " if k in taken else "NOT TAKEN") + " " + k)
        return 0 if all(k in taken for k in claimed) else 1
    for k in sorted(untaken):
        print(f"{untaken[k]:5d}  {k}")
    print(f"{len(untaken)} untaken sides on executed lines, {len(taken)} taken", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
