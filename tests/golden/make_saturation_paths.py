#!/usr/bin/env python3
"""Regenerates tests/golden/saturation_paths.json: directed packets that make the saturating helpers of the oracle clamp, at the
call sites where the suite's random payloads clamp rarely or never.  CPU only, deterministic for a seed.

    python tests/golden/make_saturation_paths.py [--seed N] [--rounds N] [--baseline]

tools/oracle_saturation.py counts, per call site of sat16 / satsym / add_sat32 / sub_sat32 / lshift_sat32 / limit32, the calls and
the clamps on either side.  A site with at least ABUNDANT clamps a side under the baseline (the tool's report for the suite's
random payload families) needs nothing.  Every other site of oc_silk.c, oc_celt.c, oc_celt_math.c and oc_packet.c ends up in
exactly one of "reached" (the corpus clamps it on both sides), "unreachable" (UNREACHABLE below: a value-range argument; a site
may be unreachable on one side and reached on the other) or "open" (what was tried).

Three stages:
  1. the LPC synthesis update of decode_core (add_sat32 and lshift_sat32 on one line): a frame with the highest gain index whose
     shell blocks all carry ten LSB shifts saturates it thousands of times.  One entry per class of CLASSES (bandwidth x voicing
     x mono / stereo packet with the side channel absent), three packets each, chosen so that the positions report of the census
     shows what CLASS_NEEDS asks for; and the same frames in RFC mode, each followed by a lost packet (the concealment's and the
     comfort noise's synthesis updates, and the mix of the concealed layers);
  2. the NLSF -> LPC sites: every stage-1 index with every residual vector over the corner alphabet of make_rare_paths.py through
     oc_test_nlsf2a under the census; a vector that clamps a wanted site is written as a frame;
  3. a greedy pick, by the positions report, from candidate sequences: the rare-paths corpus, pitch lags at both ends of their
     range, saturating frames without voice activity and then a loss (the comfort noise), loud CELT frames with a long post-filter
     period and then losses (the pitch-based concealment), and the random families of make_rare_paths.py, in reference mode and
     in RFC mode with every packet followed by a loss.
An entry holds at most 4 packets of at most 250 payload bytes.
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
sys.path.insert(0, HERE)
import oracle_saturation as osat  # noqa: E402
import make_rare_paths as mrp  # noqa: E402
import rc_craft as rcc  # noqa: E402

OUT = os.path.join(HERE, "saturation_paths.json")
ABUNDANT = 1000
MAX_PACKETS, MAX_PAYLOAD = 4, 250
SYNTH = "decode_core|sLPC_Q14[MAX_LPC + i] = add_sat32(pres_Q14[i], lshift_sat32(LPC_pred_Q10, 4));"
SYNTH_KEYS = [f"oc_silk.c|{SYNTH}|add_sat32", f"oc_silk.c|{SYNTH}|lshift_sat32"]
CNG = "cng|sig_Q14[MAX_LPC + i] = add_sat32(sig_Q14[MAX_LPC + i], lshift_sat32(LPC_pred_Q10, 4));"
CNG_KEYS = [f"oc_silk.c|{CNG}|add_sat32", f"oc_silk.c|{CNG}|lshift_sat32"]
PLC = "plc_conceal|sLPC[MAX_LPC + i] = add_sat32(sLPC[MAX_LPC + i], lshift_sat32(LPC_pred_Q10, 4));"
UPDATE_KEYS = SYNTH_KEYS + [f"oc_silk.c|{PLC}|add_sat32", f"oc_silk.c|{PLC}|lshift_sat32"] + CNG_KEYS  # the four device forms' line
BANDS = {"nb": (0x08, 8), "mb": (0x28, 12), "wb": (0x48, 16), "hybrid": (0x78, 16)}  # TOC (20 ms, mono), internal kHz
CLASSES = [(b, v, s) for b in BANDS for v in ("unvoiced", "voiced") for s in ("mono", "stereo")]
CLASS_NEEDS = ("per class: add_sat32 and lshift_sat32 each clamp high and low at least 16 times; a clamp falls on every sample index "
               "mod 4, in the first and in the last subframe, and on sample 0 of a frame behind a frame whose last 10 samples (the "
               "shortest filter's history) hold an add_sat32 clamp")

# Why a site cannot clamp on a side: (substring of the key, sides, reason).  Lines are oracle/oc_silk.c : src/silk.cpp.
UNREACHABLE = [
    ("inverse32_varQ|", "high low",
     "the shift is 0 whenever the call is made: lshift = 61 - b_headrm - Qres is 0 from inverse_pred_gain (oc_silk.c:545-546: Qres = "
     "mult2Q + 30 = 62 - clz = 61 - b_headrm), 14 - b_headrm >= 0 from decode_core (:731: Qres 47, the gain is log2lin of 2090..3924, "
     "at least 2^16, so b_headrm <= 14) and 15 - b_headrm >= 1 from plc_conceal (:914); lshift_sat32(x, 0) clamps to the whole int32 "
     "range (silk.h:139; tests/test_saturation_paths.py walks the 64 gains)"),
    ("div32_varQ|", "high low",
     "the only caller divides two gains (oc_silk.c:733), both log2lin of 2090..3924 = 2^16.3 .. 2^30.7: lshift = 13 + a_headrm - b_headrm "
     "with both headrooms in 0..14 is negative only as -1, for a_headrm 0 and b_headrm 14; then result = a / b in Q29 with a_nrm < 2^31 and "
     "b_nrm = b << 14 >= 2^30.3, below 2^29.7 < INT32_MAX >> 1, and never negative (tests/test_saturation_paths.py walks the 64 x 64 pairs)"),
    ("nlsf_stabilize|i32 lo = sat16(", "low",
     "both terms are non-negative: NLSF_Q15[0] is at least NDeltaMin_Q15[0] > 0 (oc_silk.c:439) and every later one at least its "
     "predecessor (:442); NDeltaMin_Q15 is positive"),
]


# What is known about a site that stays open, in front of what was tried: (substring of the key, note).
OPEN_NOTES = [
    ("inverse_pred_gain|", "the step-down recursion's coefficients are Q24 and the subtraction clamps only when two of them sum past 128.0; "
                           "the guard on the next line (tmp64 outside int32 -> return 0, oc_silk.c:552, :555) ends the recursion once one passes "
                           "128.0, and in everything tried it fires first (the rare-paths corpus takes all of its sides) -- no proof that it must; "),
    ("lpc_fit|", "the line runs only when ten rounds of bandwidth expansion leave a coefficient outside 16 bits (oc_silk.c:517): two vectors of "
                 "the 4 million NLSF corners get there, both with the negative coefficient too large; "),
]


def open_note(key):
    return "".join(note for sub, note in OPEN_NOTES if sub in key)


def unreachable_sides(key):
    out = {}
    for sub, sides, why in UNREACHABLE:
        if sub in key:
            for s in sides.split():
                out.setdefault(s, why)
    return out


# ---- stage 1: the synthesis update, one entry per class -----------------------------------------------------------------------------
def _sat_chan(r, order, voiced):
    """(wide NLSF residuals: a resonant synthesis filter is what carries the excitation to 2^31; with residuals of -2..2 one frame
    in thirty saturates, with -10..10 five in six)"""
    t = r.choice([4, 5]) if voiced else r.choice([0, 1, 2, 3])
    ch = {"vad": 1 if t > 1 else 0, "type": t, "gains": [63, 4, 4, 4], "nlsf1": r.randrange(32),
          "nlsf_res": [r.randint(-10, 10) for _ in range(order)], "interp": r.randrange(5), "seed": r.randrange(4)}
    if voiced:
        ch.update(lag=(r.randrange(32), r.randrange(4)), contour=r.randrange(11), per=r.randrange(3), ltp_scale=r.randrange(3))
        ch["ltp"] = [r.randrange([8, 16, 32][ch["per"]]) for _ in range(4)]
    return ch


def sat_frame(r, band, voiced, stereo):
    """one packet: gain index 63 kept over the four subframes, ten LSB shifts in every shell block, the rest noise"""
    toc, fs = BANDS[band]
    ch = _sat_chan(r, 16 if fs == 16 else 10, voiced)
    pulses = {"rate_level": r.randrange(9), "blocks": [[17] * 10 + [r.randrange(1, 17)] for _ in range(20 * fs // 16)]}
    n = MAX_PAYLOAD
    fill = [r.randrange(256) for _ in range(n)]
    if not stereo:
        return bytes([toc]) + rcc.silk_frame(n, 1, fs, chans=[ch], pulses=pulses, fill=fill)
    pred = (r.randrange(25), [r.randrange(3), r.randrange(5)], [r.randrange(3), r.randrange(5)])
    return bytes([toc | 4]) + rcc.silk_frame(n, 2, fs, chans=[ch, {"vad": 0}], stereo_pred=pred, mid_only=1, pulses=pulses, fill=fill)


def class_report(positions, seq, band, frames):
    """What the positions report says about sequence `seq` at the synthesis update -> (counts {helper: [high, low]}, set of sample
    indices mod 4 with a clamp, clamp in the first subframe, in the last, on sample 0 behind a saturated history)"""
    flen = 20 * BANDS[band][1]
    counts, mod4, first, last, carried = {}, set(), False, False, False
    tail = set()  # packets whose last 10 samples hold an add_sat32 clamp
    for key in SYNTH_KEYS:
        c = counts[key.rsplit("|", 1)[1]] = [0, 0]
        for s, packet, ordinal, side in positions.get(key, []):
            if s != seq or packet >= frames:
                continue
            assert ordinal < flen  # one coded channel: the n-th call is sample n
            c[side - 1] += 1
            mod4.add(ordinal % 4)
            first |= ordinal < flen // 4
            last |= ordinal >= flen - flen // 4
            if key.endswith("add_sat32") and ordinal >= flen - 10:
                tail.add(packet)
    for key in SYNTH_KEYS:
        carried |= any(s == seq and ordinal == 0 and packet - 1 in tail for s, packet, ordinal, side in positions.get(key, []))
    return counts, mod4, first, last, carried


def class_ok(rep):
    counts, mod4, first, last, carried = rep
    return all(v >= 16 for c in counts.values() for v in c) and mod4 == {0, 1, 2, 3} and first and last and carried


def stage_classes(cb, seed, tries=24):
    entries = []
    for cls in CLASSES:
        band, voicing, chans = cls
        attempt, found = 0, None
        while found is None:
            cands = []
            while len(cands) < tries:
                r = random.Random(f"{seed}/{'-'.join(cls)}/{attempt}")
                attempt += 1
                try:
                    pk = [sat_frame(r, band, voicing == "voiced", chans == "stereo") for _ in range(3)]
                except rcc.CraftError:
                    continue
                cands.append({"channels": 2 if chans == "stereo" else 1, "packets": [p.hex() for p in pk], "rfc": False})
            cen = cb.decode(cands, positions=True)
            for i, c in enumerate(cands):
                if all(row[0] == 960 for row in cen["results"][i]) and class_ok(class_report(cen["positions"], i, band, 3)):
                    found = c
                    break
            assert attempt < 40 * tries, cls
        found["class"] = "-".join(cls)
        entries.append(found)
        # the same frames in RFC mode (these TOCs name 20 ms: the frames read the same there), each followed by a lost packet
        entries.append({"channels": found["channels"], "packets": [found["packets"][0], "", found["packets"][1], ""], "rfc": True,
                        "class": "-".join(cls) + "-lossy"})
        if cls in (("nb", "voiced", "mono"), ("wb", "unvoiced", "mono")):  # ... and as a mono packet in a stereo decoder
            entries.append({"channels": 2, "packets": found["packets"], "rfc": False, "class": "-".join(cls) + "-in-stereo-decoder"})
        print(f"class {'-'.join(cls)}: candidate {attempt - tries + i}", file=sys.stderr)
    return entries


# ---- stage 2: the NLSF -> LPC sites, exhaustive corners ------------------------------------------------------------------------------
def nlsf_candidates(cb, wanted):
    cands = []
    for wb in (0, 1):
        total = 32 * len(mrp.NLSF_ALPHABET[wb]) ** (16 if wb else 10)
        cen = cb.nlsf_corners(wb, mrp.NLSF_ALPHABET[wb], 0, total)  # (the tool enumerates as make_rare_paths.nlsf_vector does)
        for key in sorted(cen["positions"]):
            for side in (1, 2):
                if (key, side) not in wanted:
                    continue
                ns = [n for n, _, _, s in cen["positions"][key] if s == side][:2]
                for n in ns:
                    s1, res = mrp.nlsf_vector(wb, n)
                    for fs in ((16,) if wb else (8, 12)):
                        for typ in (0, 2):
                            ch = {"vad": 1 if typ > 1 else 0, "type": typ, "gains": [20, 4, 4, 4], "nlsf1": s1, "nlsf_res": res, "interp": 4, "seed": 0}
                            try:
                                pkt = bytes([mrp.SILK_TOC[fs]]) + rcc.silk_frame(60, 1, fs, chans=[ch], fill=[(29 * i + 3) & 0xFF for i in range(60)])
                            except rcc.CraftError:
                                continue
                            cands.append({"channels": 1, "packets": [pkt.hex()], "rfc": False})
                print(f"nlsf corners wb={wb}: {'high' if side == 1 else 'low'} at vectors {ns}  {key}", file=sys.stderr)
    return cands


# ---- stage 3: candidates for the greedy pick -------------------------------------------------------------------------------------------
def _fits(packets):
    return 1 <= len(packets) <= MAX_PACKETS and all(len(p) <= 2 * (MAX_PAYLOAD + 1) for p in packets)


def _lossy(seq):
    """the sequence in RFC mode, a lost packet behind each packet, as far as MAX_PACKETS reaches"""
    pk = [q for p in seq["packets"][:MAX_PACKETS // 2] for q in (p, "")]
    return {"channels": seq["channels"], "packets": pk, "rfc": True}


def lag_candidates(r):
    out = []
    for band in ("nb", "mb", "wb"):
        toc, fs = BANDS[band]
        for lag, contours in (((0, 0), range(11)), ((31, [3, 5, 7][("nb", "mb", "wb").index(band)]), range(11))):
            for contour in contours:
                ch = _sat_chan(r, 16 if fs == 16 else 10, True)
                ch.update(gains=[30, 4, 4, 4], lag=lag, contour=contour)
                try:
                    pkt = bytes([toc]) + rcc.silk_frame(60, 1, fs, chans=[ch], fill=[r.randrange(256) for _ in range(60)])
                except rcc.CraftError:
                    continue
                out.append({"channels": 1, "packets": [pkt.hex()], "rfc": False})
    return out


def observable(cb, seqs, key):
    """per sequence: does a WRAPPING operation at site `key` (what a wrong kernel would compute) change the crc of any packet's PCM?
    A clamp that the output does not show -- scaled by a gain of 0, or left in a state nothing reads again -- protects nothing."""
    return [a != b for a, b in zip(cb.decode(seqs)["results"], cb.decode(seqs, wrap=key)["results"])]


def cng_candidates(cb, r, count):
    """Saturating frames without voice activity and with the same side information (they feed the comfort noise's excitation buffer
    and move its smoothed gain and filter towards theirs, a quarter of the way per frame), the last of them 28 gain steps quieter,
    then a loss.  The comfort noise's gain is sqrt(smoothed gain^2 - 32 * (concealment gain)^2), 0 when the square root's argument
    is not positive (oc_silk.c:1023-1033): behind a loud last frame it is 0 and the saturated synthesis adds nothing to the PCM;
    behind a quiet one the smoothed gain, which follows slowly, wins.  Kept: the candidates whose PCM a wrapping add and a wrapping
    shift in the comfort noise's synthesis update both change."""
    out = []
    while len(out) < count:
        toc, fs = BANDS[r.choice(sorted(BANDS))]
        ch = _sat_chan(r, 16 if fs == 16 else 10, False)
        ch.update(vad=0, type=r.choice([0, 1]))
        quiet = dict(ch, gains=[r.randrange(0, 48), 0, 0, 0])  # the index falls by 16 at most, then by 4 per subframe: 63 -> 35
        try:
            pk = []
            for c in (ch, ch, quiet):
                pulses = {"rate_level": r.randrange(9), "blocks": [[17] * 10 + [r.randrange(1, 17)] for _ in range(20 * fs // 16)]}
                pk.append((bytes([toc]) + rcc.silk_frame(MAX_PAYLOAD, 1, fs, chans=[c], pulses=pulses, fill=mrp._noise(r, MAX_PAYLOAD))).hex())
        except rcc.CraftError:
            continue
        out.append({"channels": 1, "packets": pk + [""], "rfc": True})
    seen = [observable(cb, out, key) for key in CNG_KEYS]
    return [c for c, a, b in zip(out, *seen) if a and b]


def celt_loss_candidates(r, count):
    """loud CELT frames with a strong post-filter of a long period, then losses: the pitch-based concealment pre-filters its overlap
    through taps that reach back behind the frame (oc_celt.c:1490-1498)"""
    out = []
    while len(out) < count:
        stereo = r.random() < 0.5
        pk = []
        try:
            for _ in range(r.choice([1, 2])):
                n = r.choice([80, 160, 250])
                pf = (5, r.randrange(256, 512), r.choice([5, 6, 7]), r.randrange(3))
                coarse = [[r.choice([5, 8]), r.choice([5, 8])] for _ in range(21)]
                try:
                    body = rcc.celt_frame(n, 2 if stereo else 1, postfilter=pf, transient=0, intra=r.randrange(2), coarse=coarse, fill=mrp._noise(r, n))
                except rcc.CraftError:
                    body = rcc.celt_frame(n, 2 if stereo else 1, postfilter=pf, transient=0, fill=mrp._noise(r, n))
                pk.append((bytes([0xFC if stereo else 0xF8]) + body).hex())
        except rcc.CraftError:
            continue
        out.append({"channels": 2 if stereo else 1, "packets": pk + [""] * (MAX_PACKETS - len(pk)), "rfc": True})
    return out


def family_candidates(r, count):
    out = []
    while len(out) < count:
        c = mrp.FAMILIES[len(out) % len(mrp.FAMILIES)](r)
        if not c:
            continue
        seq = {"channels": c[0], "packets": [p.hex() for p in c[1][:MAX_PACKETS]], "rfc": False}
        if not _fits(seq["packets"]):
            seq["packets"] = [p for p in seq["packets"] if len(p) <= 2 * (MAX_PAYLOAD + 1)]
            if not seq["packets"]:
                continue
        out.append(seq)
        out.append(_lossy(seq))
    return out


def greedy(cb, cands, wanted):
    """pick, by the positions report, the sequences that clamp wanted (key, side) pairs nothing before them clamped"""
    if not cands or not wanted:
        return []
    cen = cb.decode(cands, positions=True)
    by_seq = {}
    for key, rows in cen["positions"].items():
        for s, _, _, side in rows:
            if (key, side) in wanted:
                by_seq.setdefault(s, set()).add((key, side))
    picked = []
    while True:
        best = max(sorted(by_seq), key=lambda s: len(by_seq[s] & wanted), default=None)
        if best is None or not (by_seq[best] & wanted):
            break
        wanted -= by_seq[best]
        picked.append(cands[best])
        print(f"greedy: +{len(by_seq[best])} ({len(wanted)} left)  {sorted(by_seq[best])[0][0]}", file=sys.stderr)
    return picked


def in_scope(key):
    return key.split("|")[0] in osat.SITE_FILES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20241)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=600)
    ap.add_argument("--baseline", action="store_true", help="measure the baseline census again instead of reusing the fixture's")
    a = ap.parse_args()
    with osat.CensusBuild() as cb:
        if a.baseline or not os.path.exists(OUT):
            baseline = {k: v for k, v in cb.decode(osat.ob.baseline_sequences())["sites"].items() if in_scope(k)}
        else:
            baseline = json.load(open(OUT))["baseline"]
        abundant = sorted(k for k, (_, hi, lo) in baseline.items() if hi >= ABUNDANT and lo >= ABUNDANT)
        reasons, unreachable = [], {}
        wanted = set()
        for k in sorted(baseline):
            if k in abundant:
                continue
            un = unreachable_sides(k)
            for side, why in un.items():
                if why not in reasons:
                    reasons.append(why)
                unreachable.setdefault(k, {})[side] = reasons.index(why)
            wanted |= {(k, s) for s, name in ((1, "high"), (2, "low")) if name not in un}
        entries = stage_classes(cb, a.seed)
        cen = cb.decode(entries, positions=True)
        wanted -= {(k, side) for k, rows in cen["positions"].items() for _, _, _, side in rows}
        r = random.Random(a.seed)
        rare = json.load(open(os.path.join(HERE, "rare_paths.json")))["entries"]
        pool = [{"channels": e["channels"], "packets": e["packets"], "rfc": False} for e in rare if _fits(e["packets"])]
        pool += [_lossy(s) for s in pool] + lag_candidates(r) + cng_candidates(cb, r, 200) + celt_loss_candidates(r, 200) + nlsf_candidates(cb, wanted)
        entries += greedy(cb, pool, wanted)
        for rnd in range(a.rounds):
            if not wanted:
                break
            entries += greedy(cb, family_candidates(r, a.batch), wanted)
        # what every entry clamps, alone, at the sites that are not abundant: its claims
        scope = [k for k in baseline if k not in abundant]
        total = {k: [0, 0] for k in scope}
        for e in entries:
            cen = cb.decode([e])
            e["expect"] = cen["results"][0]
            e["keys"] = {k: cen["sites"][k][1:] for k in sorted(scope) if cen["sites"][k][1] or cen["sites"][k][2]}
            for k, (hi, lo) in e["keys"].items():
                total[k][0] += hi
                total[k][1] += lo
        # which entries SHOW a wrong (wrapping) synthesis update in their PCM, per site of UPDATE_KEYS: indices into entries
        shows = {}
        for key in UPDATE_KEYS:
            who = [i for i, e in enumerate(entries) if sum(e["keys"].get(key, [0, 0]))]
            seen = observable(cb, [entries[i] for i in who], key)
            shows[key] = [i for i, ok in zip(who, seen) if ok]
            assert shows[key], ("no entry shows a wrapping operation at", key)
        verdicts, open_ = {}, {}
        for k in sorted(baseline):
            if k in abundant:
                verdicts[k] = f"abundant: {baseline[k][1]} high and {baseline[k][2]} low clamps in {baseline[k][0]} calls of the baseline"
                continue
            un = unreachable.get(k, {})
            sides = {"high": total[k][0], "low": total[k][1]}
            missing = [s for s in sides if not sides[s] and s not in un]
            reached = [s for s in sides if sides[s]]
            if missing:
                open_[k] = open_note(k) + (f"no clamp on the {' and the '.join(missing)} side: tried the classes' frames, the rare-paths corpus, the exhaustive NLSF "
                            f"corners, both ends of the pitch lag range, the comfort-noise and CELT loss candidates and {a.rounds} rounds of {a.batch} sequences of the rare-paths families, in "
                            "reference mode and in RFC mode with a loss behind every packet")
                verdicts[k] = "open"
            elif len(un) == 2:
                verdicts[k] = "unreachable"
            elif un:
                verdicts[k] = f"reached by the corpus on the {reached[0]} side, unreachable on the {list(un)[0]} side"
            else:
                verdicts[k] = "reached by the corpus on both sides"
    fx = {"about": "directed packets that make the oracle's saturating helpers clamp; made by tests/golden/make_saturation_paths.py, read by "
                   "tests/test_saturation_paths.py, tests/test_gpu_saturation_paths.py and tools/oracle_saturation.py --corpus.  baseline: "
                   "key -> [calls, high, low] under the suite's random payloads.  An entry: rfc = decoded in RFC mode, where an empty "
                   "packet is a lost one (20 ms concealed); expect: per packet [return code, final range, crc32 of the PCM] of the oracle; "
                   "keys: site -> [high, low] clamps of this entry alone, for every site that is not abundant.  shows_a_wrapping_update: per site of "
                   "the LPC synthesis update (decoded frames, concealment, comfort noise; both helpers), the entries whose PCM changes when "
                   "that operation wraps instead of saturating",
          "seed": a.seed, "rounds": a.rounds, "batch": a.batch, "abundant_from": ABUNDANT, "class_needs": CLASS_NEEDS, "baseline": baseline,
          "verdicts": verdicts, "reasons": reasons, "unreachable": unreachable, "open": open_, "shows_a_wrapping_update": shows, "entries": entries}
    with open(OUT, "w") as f:
        json.dump(fx, f, indent=1, sort_keys=True)
        f.write("\n")
    n = {v.split(":")[0].split(" on ")[0]: 0 for v in verdicts.values()}
    for v in verdicts.values():
        n[v.split(":")[0].split(" on ")[0]] += 1
    print(f"{len(baseline)} sites: {n}; {len(entries)} entries, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
