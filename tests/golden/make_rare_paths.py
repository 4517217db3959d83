#!/usr/bin/env python3
"""Regenerates tests/golden/rare_paths.json: directed packets for the branch sides of the oracle's reference-mode decode that the
suite's random payloads never take.  CPU only, deterministic for a seed.

    python tests/golden/make_rare_paths.py [--seed N] [--rounds N] [--baseline]

A coverage-guided search: the frame writers of tests/rc_craft.py pin a frame's leading symbols (the families below), random bytes
fill the rest, tools/oracle_branches.py says which sides of the baseline list a batch of candidate sequences took; a sequence
that takes a side nothing before it took is found by bisection, shrunk (packets dropped from the front while the side stays
taken) and kept.  A sequence is one stream's packets from a fresh decoder, at most 8.

The baseline list (the tool's report for the suite's random payload families) is kept in the fixture; --baseline measures it
again (half a minute), otherwise the one in the existing fixture is reused.  Every side of it ends up in exactly one of
"reached" (named by an entry's keys), "unreachable" (UNREACHABLE below: why reference mode cannot take it) or "open".
"""
import argparse
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_branches as ob  # noqa: E402
import rc_craft as rcc  # noqa: E402

OUT = os.path.join(HERE, "rare_paths.json")

# Why reference mode cannot take a side: (substring of the key, reason).  The first match counts.  Lines are oracle/<file> : reference.
R_LOSS = ("reference mode never conceals or recovers: oc_decode passes lostFlag 0 (oc_packet.c oc_decode_frame, `fec ? 2 : 0` with fec "
          "only in RFC mode; src/opus_decoder.cpp:203 calls silk_Decode with lostFlag 0), so lossCnt / loss_count stay 0")
R_20MS = ("every SILK frame decodes as 20 ms in reference mode (oc_opus.h Q6; src/silk.cpp:1522-1540 pins payloadSize_ms to 20): one "
          "internal frame of four subframes per packet, frame_length = 20 * fs_kHz, a multiple of 16")
R_COND = ("one SILK frame per packet: nFramesDecoded is reset by every call (`first` is always 1, oc_packet.c) so FrameIndex <= 0 and "
          "condCoding is 0 (src/silk.cpp:1691-1705)")
R_TRANS = ("LM is 3 (frame_size 960) or, for the 2.5 ms frame that follows a hybrid frame into SILK-only (Q4, oc_packet.c:377-378), 0; the "
           "transient flag is read only when LM > 0 (oc_celt.c:1127; src/celt.cpp:2268), anti-collapse needs a transient (:2330), so "
           "wherever a transient or anti-collapse is under way LM is 3")
R_FSIZE = ("oc_decode_frame asks for 960 samples, or 120 for the Q4 frame (oc_packet.c:367, :378; src/opus_decoder.cpp:262-275): both are "
           "120 << LM, so the loop always leaves through its break with LM <= 3")
R_ARGS = ("the packet layer never calls with such arguments: the payload is at most 1275 bytes (oc_packet_parse), pcm is the caller's "
          "buffer, end_band stays 21 (oc_celt_init; Q1: src/celt.cpp ignores CELT_SET_END_BAND)")
UNREACHABLE = [
    ("lostFlag", R_LOSS), ("lossCnt", R_LOSS), ("loss_count", R_LOSS), ("|plc|if (lost)", R_LOSS), ("last_frame_lost", R_LOSS),
    ("nb_subfr == 4", R_20MS), ("payload_ms", R_20MS), ("nFramesPerPacket", R_20MS), ("iter * 16 < frame_length", R_20MS),
    ("frame_length != c->frame_length", R_20MS + "; the length changes only together with fs_kHz"),
    ("set_fs|if (c->fs_kHz != fs_kHz) {", R_20MS + "; inside, fs_kHz is the only thing that can have changed"),
    ("c->fs_API_hz != 48000", "fs_API_hz is 0 only while fs_kHz is 0 too (chan_init), so the first condition already holds then; afterwards it is "
                              "48000 for good (oc_silk.c set_fs; src/silk.cpp:1541-1545)"),
    ("condCoding", R_COND), ("if (decode_abs)", R_COND + ": the lag is always coded absolutely"), ("FrameIndex <= 0", R_COND), ("if (first)", R_COND), ("s->ch[0].nFramesDecoded == 0", R_COND),
    ("(i > 0 && s->ch[n].LBRR_flags[i - 1])", R_COND),
    ("internal_hz ?", "internal_hz is 8000 / 12000 / 16000 in every decoding call; 0 comes only with a lost packet (oc_packet.c)"),
    ("fs_kHz_dec != 8 &&", "internal_hz is one of 8000 / 12000 / 16000 (oc_packet.c, from the TOC's bandwidth; src/opus_decoder.cpp:183-196)"),
    ("nChannelsInternal == 1)", "nChannelsAPI and nChannelsInternal are always assigned together (oc_silk.c:1265-1266; src/silk.cpp:1547-1548): "
                                "when the first is not 1 the second is not either"),
    ("j == c->nb_subfr", "j * subfr_length < pitchL <= 18 * fs_kHz < 4 * 5 * fs_kHz: the loop ends before j reaches nb_subfr = 4 "
                         "(decode_pitch clamps the lag to max_lag, src/silk.cpp:2075)"),
    ("log2lin", "the only caller in scope passes smulwb(1907825, idx) + 2090 with idx in 0..63, i.e. 2090..3924: never negative, never "
                "below 2048, never 3967 or more (oc_silk.c decode_parameters; src/silk.cpp:2163-2172)"),
    ("3967", "smulwb(1907825, 63) + 2090 = 3924 < 3967: the clamp never acts (src/silk.cpp:2171)"),
    ("inverse32_varQ|return lshift < 32", "lshift is 61 - b_headrm - Qres: 0 from inverse_pred_gain (Qres = mult2Q + 30 = 62 - clz), 14 - b_headrm from "
                                          "decode_core (Qres 47): always below 32"),
    ("div32_varQ|return lshift < 32", "the only caller divides two gains of 2^16.3 .. 2^30.7 (log2lin of 2090..3924): lshift = 13 + a_headrm - "
                                      "b_headrm <= 27"),
    ("LM == 3", R_TRANS), ("transient && LM >= 2 &&", R_TRANS), ("for (LM = 0", R_FSIZE), ("LM > 3", R_FSIZE),
    ("rc->storage > 1275", R_ARGS), ("st->end_band > 0", R_ARGS), ("for (i = end; i < NB", R_ARGS),
    ("quant_band_n1|if (lowband_out)", "N == 1 only for the bands of width 1 at LM 0 (bands 0..7 of the Q4 frame; quant_partition never splits below "
                                       "N > 2 and calls itself, not quant_band): lowband_out is NULL only for the last band, 20, whose width is 22 "
                                       "(oc_celt.c quant_all_bands `last ? NULL`; src/celt.cpp:1810-1830)"),
    ("stereo_merge|if (k", "the function has returned already unless El and Er are at least 161061 > 2^17 (oc_celt.c:451; src/celt.cpp:1126): "
                           "ilog2 >= 17, so kl and kr are at least 8"),
    ("oc_rc_tell(rc) > 8 *", "every symbol is read behind a check that its worst case fits what is left (oc_celt.c:1117-1162 flags, post-filter 16 "
                             "bits, coarse energy 15 / 2 / 1, tf, spread, dynalloc, trim; the allocation hands out at most the bits left, and "
                             "quant_band_n1, fine energy and the final bits count theirs down); a frame that starts past its budget (after SILK, "
                             "Q4 or hybrid) is made silent with tell set to exactly 8 * storage (:1107-1116; src/celt.cpp:2241-2252) and reads "
                             "nothing more"),
    ("nlsf2a|for (i = 0; inverse_pred_gain", "the side where i reaches 16 with the filter still unstable: in round i = 15 the chirp is 65536 - (2 << 15) = 0 "
                                             "(oc_silk.c nlsf2a; src/silk.cpp:686-692), bwexpander_32 then zeroes every coefficient, and "
                                             "inverse_pred_gain of an all-zero filter is 1 << 30, not 0: `i < 16` is never evaluated as false"),
    ("compute_theta|} else if (stereo) {", "a mono split with qn == 1 does not exist: quant_partition splits only for b > cache max + 12 (oc_celt.c:626; "
                                           "src/celt.cpp:1400) and compute_qn gives 1 only for qb < 4 (:521; src/celt.cpp:1229); over every band, "
                                           "LM 0 and 3 and every split depth the smallest b that splits gives qb >= 19 "
                                           "(tests/test_rare_paths.py test_a_mono_split_never_has_qn_1 walks the ROM tables)"),
    ("lg32 < -32768", "bandLogE is at least -28 * 1024 after coarse_energy's clamp (src/celt.cpp:3655), fine energy and the final bits take off less "
                      "than 1024 more, and eMeans is not negative: lg32 > -32768 (src/celt.cpp:958-962)"),
    ("if (x != y) memmove", "oc_celt_decode filters in place (x == y, src/celt.cpp:2381-2389); only the concealment passes two buffers"),
    ("oc_cos_norm", "the only caller is exp_rotation with theta = gain^2 / 2 and 32767 - theta, gain = len / (len + factor * K) in Q15 with "
                    "2 K < len and factor <= 15 (src/celt.cpp:707-735): 0 < theta < 16384, so both arguments lie in (0, 32768) and none has its "
                    "low 15 bits clear"),
    ("oc_exp2|if (integer > 14)", "both callers (anti_collapse) pass a value <= 0 (src/celt.cpp:1027, :1053)"),
    ("oc_sqrt", "the only caller passes N0 << 22 with a band width 1 <= N0 <= 176: neither 0 nor 2^30 and above (src/celt.cpp:1616)"),
    ("oc_exp_rotation|if (dir < 0)", "the decoder always rotates backwards, dir = -1 (oc_celt.c alg_unquant; src/celt.cpp:2616)"),
    ("oc_fft|switch", "the side gcov adds for `no case matches`: the factors of the four transforms are 2, 3, 4 and 5 only (src/celt.cpp:170-175)"),
]


def unreachable_reason(key):
    for sub, why in UNREACHABLE:
        if sub in key:
            return why
    return None


# ---- candidate families --------------------------------------------------------------------------------------------------------
def _noise(r, n):
    return [r.randrange(256) for _ in range(n)]


def _silk_chan(r, order, extreme):
    sig = r.choice([0, 1, 2, 2])
    vad = 1 if sig else r.randrange(2)
    if not vad:
        sig = 0
    t = sig * 2 + r.randrange(2)
    if extreme == "nlsf":
        pat = r.choice(["alt", "hi", "lo", "rand", "ramp"])
        res = {"alt": [10 if i & 1 else -10 for i in range(order)],
               "hi": [r.choice([10, 9, 8]) for _ in range(order)],
               "lo": [r.choice([-10, -9, -8]) for _ in range(order)],
               "rand": [r.choice([-10, -6, 0, 6, 10]) for _ in range(order)],
               "ramp": [max(-10, min(10, (i - order // 2) * r.choice([-3, -2, 2, 3]))) for i in range(order)]}[pat]
        if r.random() < 0.5:
            res = [-v for v in res]
    else:
        res = [r.randint(-3, 3) for _ in range(order)]
    ch = {"vad": vad, "type": t, "gains": [r.randrange(64)] + [r.choice([0, 4, 4, 40, r.randrange(41)]) for _ in range(3)],
          "nlsf1": r.randrange(32), "nlsf_res": res, "interp": r.randrange(5), "seed": r.randrange(4)}
    if sig == 2:
        ch.update(lag=(r.randrange(32), r.randrange(4)), contour=r.randrange(11), per=r.randrange(3), ltp_scale=r.randrange(3))
        ch["ltp"] = [r.randrange([8, 16, 32][ch["per"]]) for _ in range(4)]
    return ch


NPK = [1, 1, 2, 3, 5, 8]
SILK_TOC = {8: 0x08, 12: 0x28, 16: 0x48}


def _silk_payload(r, fs, stereo, n):
    """a SILK frame: pinned side information (extreme NLSF residuals or a pulse head with ten LSB shifts), then noise"""
    extreme = r.choice(["nlsf", "nlsf", "pulses"])
    ch = _silk_chan(r, 16 if fs == 16 else 10, extreme)
    pulses = None
    if extreme == "pulses":
        pulses = {"rate_level": r.randrange(9),
                  "blocks": [[17] * r.choice([10, 10, 3, 9]) + [r.randrange(1, 17)] for _ in range(r.choice([1, 2]))]}
    if not stereo:
        return rcc.silk_frame(n, 1, fs, chans=[ch], pulses=pulses, fill=_noise(r, n))
    # stereo: the side channel without VAD and `mid only`, so that the pinned channel is the whole SILK frame
    pred = (r.randrange(25), [r.randrange(3), r.randrange(5)], [r.randrange(3), r.randrange(5)])
    return rcc.silk_frame(n, 2, fs, chans=[ch, {"vad": 0}], stereo_pred=pred, mid_only=1, pulses=pulses, fill=_noise(r, n))


def family_silk(r):
    """SILK-only NB / MB / WB, mono and stereo"""
    fs, stereo = r.choice([8, 12, 16]), r.random() < 0.4
    pkts = []
    try:
        for _ in range(r.choice(NPK)):
            n = r.choice([30, 60, 120, 250])
            pkts.append(bytes([SILK_TOC[fs] | (4 if stereo else 0)]) + _silk_payload(r, fs, stereo, n))
    except rcc.CraftError:
        return None
    return (2 if stereo else 1), pkts


def _celt_payload(r, C, n):
    kind = r.choice(["loud", "quiet", "mixed", "none"])
    coarse = None
    if kind != "none":
        v = {"loud": lambda: r.choice([3, 5, 8]), "quiet": lambda: r.choice([-3, -5, -8]), "mixed": lambda: r.choice([-6, 0, 6])}[kind]
        coarse = [[v(), v()] for _ in range(r.choice([3, 8, 21]))]
    pf = None
    if r.random() < 0.4:
        octave = r.randrange(6)
        pf = (octave, r.randrange(16 << octave), r.randrange(8), r.randrange(3))
    try:
        return rcc.celt_frame(n, C, postfilter=pf, transient=r.randrange(2), intra=r.randrange(2), coarse=coarse, fill=_noise(r, n))
    except rcc.CraftError:
        return rcc.celt_frame(n, C, postfilter=pf, transient=r.randrange(2), fill=_noise(r, n))


def family_celt(r):
    """CELT-only FB, mono and stereo, 2 .. 1275 bytes"""
    stereo = r.random() < 0.7
    pkts = []
    try:
        for _ in range(r.choice(NPK)):
            n = r.choice([2, 3, 4, 5, 6, 8, 10, 14, 20, 40, 80, 200, 600, 1275])
            pkts.append(bytes([0xFC if stereo else 0xF8]) + _celt_payload(r, 2 if stereo else 1, n))
    except rcc.CraftError:
        return None
    return (2 if stereo else 1), pkts


def family_hybrid(r):
    """hybrid SWB / FB: the SILK layer's side information pinned, the CELT layer (bands 17..20) read off the noise behind it"""
    stereo, toc = r.random() < 0.5, r.choice([0x68, 0x78])
    pkts = []
    try:
        for _ in range(r.choice(NPK)):
            n = r.choice([40, 80, 160, 300])
            pkts.append(bytes([toc | (4 if stereo else 0)]) + _silk_payload(r, 16, stereo, n))
    except rcc.CraftError:
        return None
    return (2 if stereo else 1), pkts


def family_q4(r):
    """hybrid frames followed by SILK-only ones: each SILK-only frame behind a hybrid one also runs a 2.5 ms CELT frame (LM 0, all 21
    bands, no transient) off what SILK left of the coder (Q4) -- the only LM 0 decode reference mode has"""
    stereo = r.random() < 0.5
    flag = 4 if stereo else 0
    pkts = []
    try:
        for k in range(r.choice([2, 2, 4, 6, 8])):
            n = r.choice([12, 20, 30, 45, 60, 120, 250, 600])
            if k % 2 == 0:
                body = bytes(_noise(r, n)) if r.random() < 0.5 else _silk_payload(r, 16, stereo, n)
                pkts.append(bytes([r.choice([0x68, 0x78]) | flag]) + body)
            else:
                fs = r.choice([8, 12, 16])
                pkts.append(bytes([SILK_TOC[fs] | flag]) + _silk_payload(r, fs, stereo, n))
    except rcc.CraftError:
        return None
    return (2 if stereo else 1), pkts


FAMILIES = [family_silk, family_celt, family_q4, family_hybrid]
TRIED = {}  # per function of an open side: what the search aimed at it (no side is open at present)


def tried(key):
    return TRIED.get(key.split("|")[1], "nlsf_corner_search and all four families, none aimed at this side in particular")


# ---- directed stage for the NLSF -> LPC sides: exhaustive corners, found through the oracle's own nlsf_decode + nlsf2a -------------------
# oc_test_nlsf2a (oracle/oc_silk.c) runs a stage-1 index with residuals through the oracle's NLSF decode and LPC conversion.  Every
# stage-1 index is enumerated with every residual vector over the alphabet below (order 10: 32 * 3^10 vectors, order 16: 32 * 2^16);
# the coverage counters say whether a wanted side was taken, a bisection over the enumeration finds the vector, and a SILK frame
# with exactly these indices is written and checked through the whole decoder.
NLSF_ALPHABET = {0: [-10, 0, 10], 1: [-10, 10]}


def nlsf_vector(wb, n):
    alpha, order = NLSF_ALPHABET[wb], 16 if wb else 10
    s1, rem = divmod(n, len(alpha) ** order)
    res = []
    for _ in range(order):
        rem, d = divmod(rem, len(alpha))
        res.append(alpha[d])
    return s1, res


def nlsf_worker(lib_path, wb, lo, hi):
    import ctypes as C
    lib = C.CDLL(lib_path)
    lib.oc_test_nlsf2a.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
    a = (C.c_int16 * 16)()
    for n in range(lo, hi):
        s1, res = nlsf_vector(wb, n)
        lib.oc_test_nlsf2a(bytes([s1] + [v & 0xFF for v in res]), wb, a)


def nlsf_corner_search(cov, left):
    import subprocess

    def taken(wb, lo, hi):
        cov.reset()
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--nlsf-worker", cov.lib, str(wb), str(lo), str(hi)])
        return cov.untaken()[1]

    entries = []
    wanted = {k for k in left if k.split("|")[1] in ("inverse_pred_gain", "nlsf2a", "lpc_fit", "nlsf_stabilize")}
    for wb in (0, 1):
        total = 32 * len(NLSF_ALPHABET[wb]) ** (16 if wb else 10)
        for key in sorted(wanted & taken(wb, 0, total)):
            if key not in wanted:
                continue
            lo, hi = 0, total
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if key in taken(wb, lo, mid) else (mid, hi)
            s1, res = nlsf_vector(wb, lo)
            for typ, fs in [(t, f) for f in ((16,) if wb else (8, 12)) for t in (0, 1, 2, 3)]:
                ch = {"vad": 1 if typ > 1 else 0, "type": typ, "gains": [20, 4, 4, 4], "nlsf1": s1, "nlsf_res": res, "interp": 4, "seed": 0}
                try:
                    pkt = bytes([SILK_TOC[fs]]) + rcc.silk_frame(60, 1, fs, chans=[ch], fill=[(29 * i + 3) & 0xFF for i in range(60)])
                except rcc.CraftError:
                    continue
                seq = {"channels": 1, "packets": [pkt.hex()]}
                expect = cov.decode([seq])[0]
                keys = sorted(wanted & cov.untaken()[1])
                if key in keys:
                    entries.append({"channels": 1, "packets": seq["packets"], "keys": keys, "expect": expect})
                    wanted -= set(keys)
                    print(f"nlsf corners wb={wb}: +{len(keys)}  stage-1 {s1} residuals {res}  {key}", file=sys.stderr)
                    break
            else:
                print(f"nlsf corners wb={wb}: vector {s1} {res} takes {key} but no frame type codes it", file=sys.stderr)
    return entries, left - {k for e in entries for k in e["keys"]}


def search(cov, targets, seed, rounds, batch):
    r = random.Random(seed)
    entries, left = [], set(targets)
    for rnd in range(rounds):
        if not left:
            break
        cands = []
        while len(cands) < batch:
            c = FAMILIES[rnd % len(FAMILIES)](r)
            if c:
                cands.append({"channels": c[0], "packets": [p.hex() for p in c[1]]})

        def new_sides(seqs):
            cov.decode(seqs)
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
            seq = lo[0]
            while len(seq["packets"]) > 1:  # shrink: drop packets from the front while the side stays taken
                shorter = {"channels": seq["channels"], "packets": seq["packets"][1:]}
                if key in new_sides([shorter]):
                    seq = shorter
                else:
                    break
            keys = sorted(new_sides([seq]))
            assert key in keys
            expect = cov.decode([seq])[0]
            entries.append({"channels": seq["channels"], "packets": seq["packets"], "keys": keys, "expect": expect})
            left -= set(keys)
            print(f"round {rnd}: +{len(keys)} ({len(left)} left)  {keys[0]}", file=sys.stderr)
            pool = [c for c in pool if c is not lo[0]]
    return entries, left


def main():
    if len(sys.argv) == 6 and sys.argv[1] == "--nlsf-worker":
        return nlsf_worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20240)
    ap.add_argument("--rounds", type=int, default=80)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--baseline", action="store_true", help="measure the baseline list again instead of reusing the fixture's")
    a = ap.parse_args()
    with ob.CoverageBuild() as cov:
        if a.baseline or not os.path.exists(OUT):
            cov.decode(ob.baseline_sequences())
            baseline = sorted(cov.untaken()[0])
        else:
            baseline = json.load(open(OUT))["baseline"]
        reasons, unreachable = [], {}  # the fixture holds every reason once: key -> index into "reasons"
        for k in baseline:
            why = unreachable_reason(k)
            if why:
                if why not in reasons:
                    reasons.append(why)
                unreachable[k] = reasons.index(why)
        targets = [k for k in baseline if k not in unreachable]
        entries, left = nlsf_corner_search(cov, set(targets))
        more, left = search(cov, sorted(left), a.seed, a.rounds, a.batch)
        entries += more
    fx = {"about": "directed packets for rarely taken branch sides of the oracle; made by tests/golden/make_rare_paths.py, read by "
                   "tests/test_rare_paths.py, tests/test_gpu_rare_paths.py and tools/oracle_branches.py --corpus.  expect: per packet "
                   "[return code, final range, crc32 of the PCM] of the oracle",
          "seed": a.seed, "rounds": a.rounds, "batch": a.batch, "baseline": baseline, "reasons": reasons,
          "unreachable": unreachable, "open": {k: tried(k) for k in sorted(left)}, "entries": entries}
    with open(OUT, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print(f"baseline {len(baseline)}: reached {len(targets) - len(left)}, unreachable {len(unreachable)}, open {len(left)}; "
          f"{len(entries)} entries, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
