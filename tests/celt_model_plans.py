"""What tests/test_celt_model.py (CPU) and tests/test_gpu_celt_model.py (GPU) share: the packet plans, the oracle run that reads the
tap log (oracle/oc_batch.c oc_taps_log_*), the run of tests/celt_model.py over what the taps hand it, and the comparison.

A plan is a handful of streams of a dozen packets or fewer.  CELT-only frames pin their leading symbols with tests/rc_craft.py (the
post-filter's flag and parameters, the transient flag) so that every plan holds both block layouts and the post-filter on, off and
changing; everything behind those symbols is random.  Hybrid packets are random throughout: their CELT layer starts where SILK
stops, so nothing in it can be pinned, and it codes no post-filter at all (RFC 6716 section 4.3.7.1: only frames that start at band 0
do) -- such plans are required to hold both block layouts only.
"""
import ctypes as C

import numpy as np

import celt_model
import rc_craft

DURS = (120, 240, 480, 960)
# a closed walk over the four durations that takes every ordered pair once (an Euler circuit of the complete digraph with loops)
PAIR_WALK = (0, 0, 1, 1, 2, 2, 3, 3, 0, 2, 0, 3, 1, 3, 2, 1)
LENGTHS = (10, 17, 24, 33, 47, 60, 81, 100, 127, 160)
KIND_MAIN, KIND_Q4 = 0, 1


def _celt_payload(rng, lm, channels, nbytes):
    """a CELT frame: post-filter and transient flag pinned, noise behind them"""
    pf = None
    if rng.random() < 0.6:
        octave = int(rng.integers(0, 6))
        pf = (octave, int(rng.integers(0, 1 << (4 + octave))), int(rng.integers(0, 8)), int(rng.integers(0, 3)))
    transient = int(lm > 0 and rng.random() < 0.5)
    fill = rng.integers(0, 256, nbytes, dtype=np.uint8).tolist()
    return rc_craft.celt_frame(nbytes, channels, postfilter=pf, transient=transient, LM=lm, fill=fill)


def _celt_packet(rng, lm, stereo, bw, code):
    """an RFC-mode CELT-only packet of frame-count code 0..3 (bw 0..3: NB, WB, SWB, FB)"""
    toc = ((16 + 4 * bw + lm) << 3) | (4 if stereo else 0) | code
    ch = 2 if stereo else 1
    L = int(rng.choice(LENGTHS))
    if code == 0:
        return bytes([toc]) + _celt_payload(rng, lm, ch, L)
    if code == 1:
        return bytes([toc]) + _celt_payload(rng, lm, ch, L) + _celt_payload(rng, lm, ch, L)
    if code == 2:
        return bytes([toc, L]) + _celt_payload(rng, lm, ch, L) + _celt_payload(rng, lm, ch, int(rng.choice(LENGTHS)))
    cnt = int(rng.integers(2, 4))
    return bytes([toc, cnt]) + b"".join(_celt_payload(rng, lm, ch, L) for _ in range(cnt))


def _noise_packet(rng, toc, L):
    return bytes([toc]) + rng.integers(0, 256, L, dtype=np.uint8).tobytes()


def _stereo_of(rng, channels):
    """mostly the decoder's own channel count, now and then the other one"""
    return (channels == 2) if rng.random() < 0.8 else bool(rng.integers(2))


# Seeds chosen (on the CPU, the first of 0, 1, 2, ... to do so) so that each plan keeps its conditions with some room: at most 7 % of its
# samples left out (the cap is 10 %), every (duration, transient) cell with 10 compared frames or more (the floor is 8), and for the hybrid plans, whose transient flag is one random bit of
# probability 1/8, enough transient frames at all.  tests/test_celt_model.py asserts the conditions; they are not measurements.
PLAN_SEEDS = {"rfc_runs": 0, "rfc_pairs": 1, "rfc_codes": 0, "rfc_hybrid": 8, "ref_celt": 0, "ref_switch": 0}


def build_plan(name, seed=None):
    """-> {"name", "rfc", "hybrid", "streams": [{"channels", "packets": [bytes]}]}"""
    rng = np.random.default_rng([PLAN_SEEDS[name] if seed is None else seed, sorted(PLAN_SEEDS).index(name)])
    streams = []
    if name == "rfc_runs":      # every duration as a run of its own, mono and stereo decoders
        for lm in range(4):
            for channels in (1, 2):
                for _ in range(2):
                    streams.append({"channels": channels, "packets": [
                        _celt_packet(rng, lm, _stereo_of(rng, channels), int(rng.integers(0, 4)), 0) for _ in range(12)]})
    elif name == "rfc_pairs":   # every ordered pair of consecutive durations, per channel count
        for channels in (1, 2):
            for rot in (0, 8, 4, 12):
                walk = [PAIR_WALK[(rot + k) % 16] for k in range(12)]
                streams.append({"channels": channels, "packets": [
                    _celt_packet(rng, lm, _stereo_of(rng, channels), int(rng.integers(0, 4)), 0) for lm in walk]})
    elif name == "rfc_codes":   # packets of several frames (codes 1, 2, 3) among single ones, durations changing between packets
        for channels in (1, 2):
            for s in range(4):
                streams.append({"channels": channels, "packets": [
                    _celt_packet(rng, int(rng.integers(0, 4)), _stereo_of(rng, channels), int(rng.integers(0, 4)), (k + s) % 4)
                    for k in range(10)]})
    elif name == "rfc_hybrid":  # hybrid at 10 and 20 ms, SWB and FB: configurations 12 .. 15
        for channels in (1, 2):
            for s in range(8):
                pk = []
                for _ in range(12):
                    cfg = 12 + int(rng.integers(0, 4))
                    pk.append(_noise_packet(rng, (cfg << 3) | (4 if channels == 2 else 0), int(rng.choice((60, 90, 120, 160)))))
                streams.append({"channels": channels, "packets": pk})
    elif name == "ref_celt":    # reference mode: 20 ms CELT-only (every frame decodes as 20 ms there)
        for channels in (1, 2):
            for s in range(4):
                pk = []
                for _ in range(12):
                    stereo = _stereo_of(rng, channels)
                    toc = 0xF8 | (4 if stereo else 0)
                    pk.append(bytes([toc]) + _celt_payload(rng, 3, 2 if stereo else 1, int(rng.choice(LENGTHS[3:]))))
                streams.append({"channels": channels, "packets": pk})
    elif name == "ref_switch":  # reference mode: hybrid -> SILK-only -> hybrid -> SILK-only -> CELT-only -> hybrid: Q4's 120-sample
        order = "HHHSSHHSCCHH"  # frame, 960-sample frames after it, and every switch with the reference's partial reset behind it
        for channels in (1, 2):
            for s in range(8):
                c4 = 4 if channels == 2 else 0
                pk = []
                for k in order[s % 3:] + order[:s % 3]:
                    if k == "C":
                        pk.append(bytes([0xF8 | c4]) + _celt_payload(rng, 3, channels, int(rng.choice(LENGTHS[3:]))))
                    else:
                        pk.append(_noise_packet(rng, (0x78 | c4) if k == "H" else (0x48 | c4), int(rng.choice((70, 100, 130)) if k == "H" else 50)))
                streams.append({"channels": channels, "packets": pk})
    else:
        raise KeyError(name)
    return {"name": name, "rfc": name.startswith("rfc"), "hybrid": name in ("rfc_hybrid", "ref_switch"), "streams": streams}


CELT_PLANS = ("rfc_runs", "rfc_pairs", "rfc_codes", "ref_celt")
ALL_PLANS = CELT_PLANS + ("rfc_hybrid", "ref_switch")


# ---- the oracle, with its tap log ------------------------------------------------------------------------------------------------------
def _bind(lib):
    vp = C.c_void_p
    lib.oc_taps_log_enable.argtypes = [vp, C.c_int]
    lib.oc_taps_log_count.argtypes = [vp]
    lib.oc_taps_log_dropped.argtypes = [vp]
    lib.oc_taps_log_clear.argtypes = [vp]
    lib.oc_taps_log_clear.restype = None
    lib.oc_taps_log_copy.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]


def _tap(lib, d, index, what, c, dtype, count):
    buf = np.zeros(count, dtype=dtype)
    n = lib.oc_taps_log_copy(d.h, index, what, c, buf.ctypes.data)
    assert n == buf.nbytes, (what, n, buf.nbytes)
    return buf


def _is_celt_only(toc):
    return bool(toc & 0x80)


def decode_oracle(oracle, plan):
    """Every stream of the plan through an oracle decoder of its own.
    -> per stream a list over packets of {"ret", "pcm" int16 [ret][channels], "frames": [frame records in decoding order]}.
    A frame record holds what the model consumes (X, E, lm, transient, silence, start, end, pf), what it is compared with (syn_post,
    syn_pre as int32 in Q12; pcm for the frames of CELT-only packets, else None) and kind / resets_before of the log."""
    lib = oracle.lib
    _bind(lib)
    out = []
    for st in plan["streams"]:
        cc = st["channels"]
        d = oracle.decoder(cc)
        d.set_rfc(plan["rfc"])
        d.init()
        assert lib.oc_taps_log_enable(d.h, 8)
        packets = []
        for pkt in st["packets"]:
            lib.oc_taps_log_clear(d.h)
            buf, r = d.decode(pkt)
            assert r > 0 and lib.oc_taps_log_dropped(d.h) == 0, (plan["name"], r)
            pcm = buf[:r].copy()
            frames, main = [], 0
            for i in range(lib.oc_taps_log_count(d.h)):
                info = _tap(lib, d, i, 5, 0, np.int32, 8)
                hdr = _tap(lib, d, i, 4, 0, np.int32, 75)
                start, end, n, c_coded, cc_dec, kind, resets = (int(v) for v in info[:7])
                assert cc_dec == cc and n == 120 << int(hdr[6])
                rec = {"lm": int(hdr[6]), "transient": int(hdr[0]), "silence": int(hdr[1]), "start": start, "end": end, "n": n,
                       "C": c_coded, "kind": kind, "resets_before": resets,
                       "pf": (int(hdr[7]), int(hdr[8]), int(hdr[9])) if hdr[8] else None,
                       "X": _tap(lib, d, i, 0, 0, np.int16, 1920)[:c_coded * n].reshape(c_coded, n).copy(),
                       "E": _tap(lib, d, i, 1, 0, np.int16, 42).reshape(2, 21)[:c_coded].copy(),
                       "syn_post": np.stack([_tap(lib, d, i, 3, c, np.int32, 960)[:n] for c in range(cc)]),
                       "syn_pre": np.stack([_tap(lib, d, i, 2, c, np.int32, 1080)[:n + 120] for c in range(cc)]),
                       "pcm": None}
                if kind == KIND_MAIN:
                    if _is_celt_only(pkt[0]):
                        rec["pcm"] = pcm[main * n:(main + 1) * n]
                    main += 1
                frames.append(rec)
            packets.append({"ret": r, "pcm": pcm, "frames": frames})
        out.append(packets)
    return out


# ---- the model over the same frames ----------------------------------------------------------------------------------------------------
SAT_Q12 = 300000000
GAIN_CAP_LOG2 = 18   # the fixed-point denormalisation stops doubling its gain at 2^18 (its shift has run out); a float one goes on


def frame_clamps(rec):
    """Does a saturating helper of the oracle clamp on this frame (in the sense of tools/oracle_saturation.py: satsym at SIG_SAT in the
    synthesis and in the comb filter)?  A clamped sample sits exactly at the bound."""
    n = rec["n"]
    return bool((np.abs(rec["syn_pre"][:, :n]) >= SAT_Q12).any() or (np.abs(rec["syn_post"]) >= SAT_Q12).any())


def frame_over_range(rec, emeans_q4):
    """Is a band's gain past what the fixed-point denormalisation can represent?  Then the decoder departs from the formula in a way
    that is no rounding, and the rest of the stream is left out (counted against the cap)."""
    if rec["silence"]:
        return False
    lg = rec["E"][:, rec["start"]:rec["end"]].astype(np.int64) + (np.asarray(emeans_q4[rec["start"]:rec["end"]], dtype=np.int64) << 6)
    return bool(((lg >> 10) >= GAIN_CAP_LOG2).any())


def run_model(plan, decoded, slip=None):
    """-> per stream, per packet, per frame: {"syn" float [channels][n], "pcm" int16 [n][channels], "peak", "dead"}; dead: the stream
    was left behind at or before this frame (frame_over_range)"""
    emeans = rc_craft.rom("rom_emeans")
    out = []
    for st, packets in zip(plan["streams"], decoded):
        m = celt_model.CeltModel(st["channels"], slip=slip)
        dead = False
        per_packet = []
        for p in packets:
            res = []
            for rec in p["frames"]:
                dead = dead or frame_over_range(rec, emeans)
                for _ in range(rec["resets_before"]):  # (only ref_switch has any: no RFC-mode plan switches modes, so what the
                    m.reset(partial=True)              # reset does in RFC mode is not held to the model -- DESIGN section 11)
                syn, pcm = m.frame(rec["X"], rec["E"], rec["lm"], rec["transient"], rec["start"], rec["end"], rec["pf"],
                                   silence=bool(rec["silence"]))
                res.append({"syn": syn, "pcm": pcm, "peak": m.last_peak, "dead": dead})
            per_packet.append(res)
        out.append(per_packet)
    return out


def census(plan, decoded):
    """what the plan holds: (duration, transient) cells, post-filter on / off / changing, consecutive duration pairs, kinds"""
    cells, pairs, kinds = {}, set(), {}
    pf_on = pf_off = pf_change = 0
    for packets in decoded:
        prev_n, prev_pf = None, "first"
        for p in packets:
            for rec in p["frames"]:
                cells[(rec["n"], rec["transient"])] = cells.get((rec["n"], rec["transient"]), 0) + 1
                kinds[rec["kind"]] = kinds.get(rec["kind"], 0) + 1
                if prev_n is not None:
                    pairs.add((prev_n, rec["n"]))
                pf_on += rec["pf"] is not None
                pf_off += rec["pf"] is None
                pf_change += prev_pf != "first" and prev_pf is not None and rec["pf"] is not None and prev_pf != rec["pf"]
                prev_n, prev_pf = rec["n"], rec["pf"]
    return {"cells": cells, "pairs": pairs, "kinds": kinds, "pf_on": pf_on, "pf_off": pf_off, "pf_change": pf_change}


def compare(plan, decoded, modelled, pcm_of=None):
    """The oracle's taps (and PCM; or the PCM of `pcm_of`: per stream, per packet an int16 [ret][channels]) against the model.
    -> {"syn": [(error, peak)] per compared frame, "pcm": [(error, peak)] per compared CELT-only frame,
        "left_out", "samples": samples left out / all, "cells": compared frames per (duration, transient)}"""
    syn, pcm, cells = [], [], {}
    left = total = 0
    for si, (packets, mp) in enumerate(zip(decoded, modelled)):
        for pi, (p, mres) in enumerate(zip(packets, mp)):
            main = 0
            for rec, mr in zip(p["frames"], mres):
                n = rec["n"]
                total += n
                got_pcm = rec["pcm"]
                if got_pcm is not None and pcm_of is not None:
                    got_pcm = pcm_of[si][pi][main * n:(main + 1) * n]
                main += rec["kind"] == KIND_MAIN
                if mr["dead"] or frame_clamps(rec):
                    left += n
                    continue
                cells[(n, rec["transient"])] = cells.get((n, rec["transient"]), 0) + 1
                syn.append((np.abs(rec["syn_post"] / 4096.0 - mr["syn"]).max(), mr["peak"]))
                if got_pcm is not None:
                    a, b = got_pcm.astype(np.int64), mr["pcm"].astype(np.int64)
                    keep = (a > -32768) & (a < 32767) & (b > -32768) & (b < 32767)
                    pcm.append((np.abs(a - b)[keep].max() if keep.any() else 0, mr["peak"]))
    return {"syn": syn, "pcm": pcm, "left_out": left, "samples": total, "cells": cells}
