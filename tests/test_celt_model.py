"""The oracle's CELT synthesis chain against a float64 model of RFC 6716 sections 4.3.6 to 4.3.8 (tests/celt_model.py), at every frame
size, in RFC mode and in reference mode.  CPU only.

Why: every GPU parity test compares the kernels with oracle/, and both have one author.  Reference-origin answers pin 165 frames of
20 ms; nothing pins the arithmetic of 2.5 / 5 / 10 ms frames, short blocks at those sizes, packets of changing duration, hybrid at
10 ms or the 120-sample frame of the reference's hybrid -> SILK-only switch -- a reading shared by the oracle and the
kernels would pass everywhere.  The model shares neither code nor reading with them: it is handed the decoded spectrum, the band
energies and the frame's header (the oracle's tap log, oracle/oc_batch.c oc_taps_log_*) and restates denormalisation, the inverse
MDCT with window and overlap-add, the pitch post-filter with its cross-fade, and de-emphasis.  It does NOT pin entropy decoding,
band decoding, SILK or the concealments.

The plans (tests/celt_model_plans.py): rfc_runs (each duration as a run), rfc_pairs (all 16 ordered pairs of consecutive durations),
rfc_codes (code 1 / 2 / 3 packets), rfc_hybrid (10 and 20 ms, start band 17), ref_celt (20 ms CELT-only), ref_switch (hybrid ->
SILK-only -> hybrid -> SILK-only -> CELT-only -> hybrid: Q4's 120-sample frame, the 960-sample frames after it, and the reference's
partial reset at every switch, celt_model.QUIRK_PARTIAL_RESET).  Mono and stereo decoders, packets of either count.

Compared: the synthesis after the post-filter of every CELT frame (hybrid layers and Q4's frame included), and the PCM of CELT-only
frames where neither side sits at the 16-bit bounds.  Left out: frames on which the oracle's SIG_SAT saturation clamps (the satsym
sites of the saturation census: a clamped sample sits exactly at the bound), and what follows in a stream once a band's gain
exceeds the fixed-point denormalisation's range (2^18: no rounding, the decoder departs from the formula).  At most 10 % of a plan's
samples may be left out and every (duration, transient) cell keeps 8 compared frames; the seeds were chosen for that.

TOLERANCES.  The error of a fixed-point transform grows with the level, so the bound has the form  a + b * peak,  peak being the
largest magnitude among the frame before the post-filter, the 1024 samples of history the post-filter may read and the new overlap
tail (CeltModel.last_peak).  a is the oracle's worst deviation over the frames with peak < QUIET, b its worst deviation / peak over
the others, over all six plans:

    python tests/test_celt_model.py        # prints YARDSTICK_SYN, YARDSTICK_PCM and the slip table

    YARDSTICK_SYN = (0.1832, 2.209e-4)     # PCM steps; measured 0.18315 and 2.2087e-4, rounded up
    YARDSTICK_PCM = (1.0, 1.361e-3)        # measured 1 and 1.3603e-3 (de-emphasis sums the synthesis error with a gain of up to 1 / 0.15)
    TOL = 4 * YARDSTICK                    # the factor leaves room for nothing: the GPU routes equal the oracle bit for bit

THE TOLERANCE DISCRIMINATES.  celt_model.SLIPS are ten deliberate mistakes (the issue's nine, comb period T + 1 and T - 1 apart).  For every
slip, every plan with a frame the slip changes fails its own assertion against the slipped model.  The smallest worst-frame error / TOL
over all (slip, plan) is 12.43 -- the history anchored one sample off on ref_switch, where a 960-sample frame follows Q4's 120-sample
one: the mistake DESIGN section 2 records; next come 75 (the unsquared window on ref_switch) and 102.  The oracle itself reaches 0.25.
The comparison after the post-filter tells every slip, so none at the pre-comb synthesis (oracle tap 2) is needed.
"""
import os
import re

import numpy as np
import pytest

import celt_model
import celt_model_plans as P

QUIET = 1024.0
YARDSTICK_SYN = (0.1832, 2.209e-4)
YARDSTICK_PCM = (1.0, 1.361e-3)
FACTOR = 4.0
SMALLEST_SLIP_RATIO = 12.0  # measured 12.43; a floor in test_slips_fail, so that a later change that blunts the comparison shows


def tol_syn(peak):
    return FACTOR * (YARDSTICK_SYN[0] + YARDSTICK_SYN[1] * peak)


def tol_pcm(peak):
    return FACTOR * (YARDSTICK_PCM[0] + YARDSTICK_PCM[1] * peak)


# which plans hold a frame that a slip changes, as far as their assertions see it (rfc_hybrid compares no PCM and hybrid's CELT layer
# codes no post-filter; a run of one duration never changes its frame size; ref_switch has CELT-only frames behind Q4's 120-sample one)
EVERY = set(P.ALL_PLANS)
WITH_CELT_ONLY = EVERY - {"rfc_hybrid"}
AFFECTED = {
    "ola_shift": EVERY, "deinterleave": EVERY, "emeans": EVERY,
    "xfade_unsquared": WITH_CELT_ONLY, "period_plus": WITH_CELT_ONLY, "period_minus": WITH_CELT_ONLY,
    "tapset_swap": WITH_CELT_ONLY, "pf_swap": WITH_CELT_ONLY, "deemph": WITH_CELT_ONLY,
    "anchor": {"rfc_pairs", "rfc_codes", "ref_switch"},
}

_RUNS = {}


def run(oracle, name):
    """plan, oracle decode, clean model, comparison: computed once per plan and shared, never changed"""
    if name not in _RUNS:
        plan = P.build_plan(name)
        dec = P.decode_oracle(oracle, plan)
        mod = P.run_model(plan, dec)
        _RUNS[name] = (plan, dec, mod, P.compare(plan, dec, mod), P.census(plan, dec))
    return _RUNS[name]


def worst(pairs, tol):
    """largest error / tolerance over (error, peak) pairs"""
    return max((e / tol(pk) for e, pk in pairs), default=0.0)


def test_the_model_shares_nothing_with_the_decoders():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "celt_model.py")).read()
    assert set(re.findall(r"^\s*(?:import|from)\s+([\w.]+)", src, re.M)) == {"numpy", "rc_craft"}


@pytest.mark.parametrize("name", P.ALL_PLANS)
def test_plan_holds_what_it_must(oracle, name):
    plan, dec, _, res, cen = run(oracle, name)
    cells = cen["cells"]
    sizes = {n for n, _ in cells}
    assert all(cells.get((n, 0), 0) > 0 for n in sizes), cells                     # long blocks at every size
    assert all(cells.get((n, 1), 0) > 0 for n in sizes if n > 120), cells          # short blocks wherever the size has them
    if name != "rfc_hybrid":  # (hybrid's CELT layer codes no post-filter; ref_switch has its CELT-only frames)
        assert cen["pf_on"] and cen["pf_off"] and cen["pf_change"], cen            # post-filter on, off and changing
    if name in ("rfc_runs", "rfc_pairs", "rfc_codes"):
        assert sizes == set(P.DURS)
    if name == "rfc_runs":
        for packets in dec:
            assert len({f["n"] for p in packets for f in p["frames"]}) == 1        # each stream is a run of one duration
    if name == "rfc_pairs":
        assert cen["pairs"] == {(a, b) for a in P.DURS for b in P.DURS}            # all 16 ordered pairs
    if name == "rfc_codes":
        codes = {pk[0] & 3 for st in plan["streams"] for pk in st["packets"]}
        assert codes == {0, 1, 2, 3} and any(len(p["frames"]) >= 3 for packets in dec for p in packets)
    if name == "rfc_hybrid":
        assert sizes == {480, 960} and all(f["start"] == 17 for packets in dec for p in packets for f in p["frames"])
    if name == "ref_celt":
        assert sizes == {960}
    if name == "ref_switch":  # Q4's frame, and 960-sample frames after it in the same stream
        assert cen["kinds"].get(P.KIND_Q4, 0) >= len(dec) and (120, 960) in cen["pairs"] and (960, 120) in cen["pairs"]
        q4 = [f for packets in dec for p in packets for f in p["frames"] if f["kind"] == P.KIND_Q4]
        assert all(f["n"] == 120 and f["start"] == 0 for f in q4)


@pytest.mark.parametrize("name", P.ALL_PLANS)
def test_leave_out_caps(oracle, name):
    _, _, _, res, cen = run(oracle, name)
    assert res["left_out"] <= 0.10 * res["samples"], (res["left_out"], res["samples"])
    for cell in cen["cells"]:
        assert res["cells"].get(cell, 0) >= 8, (cell, res["cells"])


@pytest.mark.parametrize("name", P.ALL_PLANS)
def test_oracle_against_the_model(oracle, name):
    plan, _, _, res, _ = run(oracle, name)
    w = worst(res["syn"], tol_syn)
    print(name, "synthesis: worst error / TOL_SYN", w, "over", len(res["syn"]), "frames")
    assert w <= 1.0, ("post-comb synthesis", name, w)
    assert len(res["pcm"]) == (len(res["syn"]) if not plan["hybrid"] else 0) or name == "ref_switch"   # the CELT-only frames
    if name != "rfc_hybrid":
        assert len(res["pcm"]) >= 16
    w = worst(res["pcm"], tol_pcm)
    print(name, "PCM: worst error / TOL_PCM", w, "over", len(res["pcm"]), "frames")
    assert w <= 1.0, ("PCM", name, w)


def slip_ratio(oracle, name, slip):
    """-> (does the slip change what the plan compares?, worst error / TOL of the oracle against the slipped model)"""
    plan, dec, mod, _, _ = run(oracle, name)
    bad = P.run_model(plan, dec, slip=slip)
    changed = any(np.abs(a["syn"] - b["syn"]).max() > 1e-9 or (rec["pcm"] is not None and (a["pcm"] != b["pcm"]).any())
                  for sd, sa, sb in zip(dec, mod, bad) for pd, pa, pb in zip(sd, sa, sb) for rec, a, b in zip(pd["frames"], pa, pb))
    res = P.compare(plan, dec, bad)
    return changed, max(worst(res["syn"], tol_syn), worst(res["pcm"], tol_pcm))


@pytest.mark.parametrize("slip", celt_model.SLIPS)
@pytest.mark.parametrize("name", P.ALL_PLANS)
def test_slips_fail(oracle, name, slip):
    changed, ratio = slip_ratio(oracle, name, slip)
    assert changed == (name in AFFECTED[slip]), (slip, name, changed)
    if changed:
        print(slip, name, "error / TOL", ratio)
        assert ratio > 1.0, (slip, name, ratio)
        assert ratio >= SMALLEST_SLIP_RATIO


if __name__ == "__main__":
    import oracle_py
    o = oracle_py.load()
    a_syn = b_syn = a_pcm = b_pcm = 0.0
    for name in P.ALL_PLANS:
        res = run(o, name)[3]
        for key in ("syn", "pcm"):
            quiet = max((e for e, pk in res[key] if pk < QUIET), default=0.0)
            loud = max((e / pk for e, pk in res[key] if pk >= QUIET), default=0.0)
            print("%-11s %s  frames %3d  quiet: worst error %.5g   loud: worst error / peak %.5g" % (name, key, len(res[key]), quiet, loud))
            if key == "syn":
                a_syn, b_syn = max(a_syn, quiet), max(b_syn, loud)
            else:
                a_pcm, b_pcm = max(a_pcm, quiet), max(b_pcm, loud)
    print("YARDSTICK_SYN = (%.5g, %.5g)   YARDSTICK_PCM = (%.5g, %.5g)" % (a_syn, b_syn, a_pcm, b_pcm))
    smallest = None
    for slip in celt_model.SLIPS:
        row = []
        for name in P.ALL_PLANS:
            changed, ratio = slip_ratio(o, name, slip)
            row.append("%s %s" % (name, "%.3g" % ratio if changed else "-"))
            if changed:
                smallest = ratio if smallest is None else min(smallest, ratio)
        print("%-16s" % slip, "  ".join(row))
    print("smallest slip error / TOL = %.4g" % smallest)
