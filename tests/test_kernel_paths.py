"""The directed corpus tests/golden/kernel_paths.json on the CPU (tests/golden/make_kernel_paths.py makes it; tools/kernel_branches.py
measures it): the branch census of the KERNEL source in host emulation, the twin of tests/test_rare_paths.py for the device code.
  * the fixture's baseline list is the one in the tool's docstring; "reached", "emulation", "unreachable" and "open" partition it; every
    reason says why (more than 40 characters), an emulation reason names the test that runs the device form; the caps on the open
    set hold: a tenth of the baseline's sides at most, and none of RecWriter, celt_parse_lane, recon_fast_eligible, recon_begin,
    pvq_leaf_lane or comb_filter;
  * the tool over the corpus alone leaves no baseline side untaken outside "emulation", "unreachable" and "open", and every entry
    decoded alone takes every key it claims (the tool refuses to report when an entry point differs from the oracle);
  * the oracle gives each entry's `expect`, and every emulation entry point that applies to an entry -- emu_decode_frame,
    emu_decode_frame_single, emu_decode_frame_shadowed, emu_decode_frame_roles and the tight library in reference mode,
    emu_decode_frame_rfc / emu_decode_frame_rfc_fec in RFC mode (compared over rfc_common.same_pcm's domain) -- gives the oracle's
    PCM and return codes, in the libraries tests/emul/Makefile builds;
  * the bounds the "unreachable" reasons quote are derived here from the ROM tables: no frame exceeds the record limits
    (REC_MAX_WORDS, REC_MAX_LEAVES, FAST_MAX_LEAVES, read from og_celt_rec.hpp), no PVQ codebook with more dimensions than pulses
    has more than 13 pulses, and the lane filter of k_celt_recon's rest role is recon_fast_eligible, term for term;
  * the RFC walks the tool's baseline decodes are the plans tests/test_gpu_rfc.py walks (both take them from rfc_common).
A fixture made with another major version of gcc may number a line's branches differently: the census tests skip then (the fixture
records its compiler), everything else runs.
"""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_paths.json")
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
NO_OPEN_SIDE_OF = ("og_celt_parse.hpp|word|", "og_celt_parse.hpp|leaf|", "og_celt_parse.hpp|words4|", "og_celt_parse.hpp|patch|",
                   "|celt_parse_lane|", "|recon_fast_eligible|", "|recon_begin|", "|pvq_leaf_lane|", "|comb_filter|")


@pytest.fixture(scope="module")
def corpus():
    return json.load(open(FIXTURE))


def _same_compiler(corpus):
    import kernel_branches as kb
    if kb.gcc_version().split(".")[0] != corpus["gcc"].split(".")[0]:
        pytest.skip(f"the fixture's branch ordinals are gcc {corpus['gcc']}'s, this is gcc {kb.gcc_version()}")


def test_the_four_sets_partition_the_baseline(corpus):
    import kernel_branches as kb
    base = set(corpus["baseline"])
    reached = {k for e in corpus["entries"] for k in e["keys"]}
    emulation, unreachable, open_ = set(corpus["emulation"]), set(corpus["unreachable"]), set(corpus["open"])
    assert len(base) == len(corpus["baseline"]) and corpus["baseline"] == sorted(base)
    sets = [reached, emulation, unreachable, open_]
    assert all(s <= base for s in sets)
    assert not any(a & b for i, a in enumerate(sets) for b in sets[i + 1:])
    assert reached | emulation | unreachable | open_ == base
    assert all(len(corpus["reasons"][i]) > 40 for i in list(corpus["unreachable"].values()) + list(corpus["emulation"].values()))
    assert all("tests/" in corpus["reasons"][i] for i in corpus["emulation"].values())  # ... names the test that runs the device form
    assert all(len(why) > 40 for why in corpus["open"].values())                       # ... and what was tried
    assert all(len(why) > 40 and why.split(":")[0] in ("unreachable", "emulation", "open") for why in corpus["never_entered"].values())
    assert all(1 <= len(e["packets"]) <= 8 and e["keys"] and len(e["expect"]) == len(e["packets"]) for e in corpus["entries"])
    assert os.path.getsize(FIXTURE) < 1 << 20
    # the caps on the open set
    assert 10 * len(open_) <= len(base)
    assert not [k for k in open_ if any(f in k for f in NO_OPEN_SIDE_OF)]
    # the tool's docstring carries the same baseline list
    listed = [ln[4:] for ln in kb.__doc__.split("\n") if re.match(r"    og_\w+\.hpp\|", ln)]
    assert listed == corpus["baseline"]
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in kb.SCOPE_FILES)
    # a reason that names a test names one that exists
    for why in corpus["reasons"] + list(corpus["open"].values()) + list(corpus["never_entered"].values()):
        for path in re.findall(r"tests/[\w/]+\.(?:py|json|hip)", why):
            assert os.path.exists(os.path.join(ROOT, path)), path


def test_corpus_takes_what_it_claims_and_leaves_only_the_named_sides(corpus):
    import kernel_branches as kb
    _same_compiler(corpus)
    seqs = kb.fixture_sequences(corpus["entries"])
    allowed = set(corpus["emulation"]) | set(corpus["unreachable"]) | set(corpus["open"])
    with kb.CoverageBuild() as cov:
        res = cov.decode(seqs)  # (raises when an entry point differs from the oracle)
        untaken, taken = cov.untaken()
        # (lines the corpus never executes are not reported by the tool; of the baseline's sides none may be missing otherwise)
        missing = [k for k in corpus["baseline"] if k not in taken and k not in allowed]
        assert not missing, missing
        for e, r in zip(corpus["entries"], res):
            assert r == e["expect"]  # the oracle computes what the fixture recorded
        for i, e in enumerate(corpus["entries"]):
            cov.decode([seqs[i]])
            t = cov.untaken()[1]
            assert all(k in t for k in e["keys"]), (i, [k for k in e["keys"] if k not in t])


def test_every_entry_point_decodes_the_corpus_as_the_oracle_does(corpus, oracle):
    """the libraries of tests/emul/Makefile (the ones every other emulation test loads), through the tool's own comparison"""
    import kernel_branches as kb
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "libog_emul.so", "libog_emul_tight.so"])
    res = kb.check_sequences(os.path.join(EMUL_DIR, "libog_emul.so"), os.path.join(EMUL_DIR, "libog_emul_tight.so"),
                             kb.fixture_sequences(corpus["entries"]))
    for i, (e, r) in enumerate(zip(corpus["entries"], res)):
        assert r == e["expect"], ("the oracle's result is not the fixture's", i)


# ---- the bounds the reasons quote, derived from the ROM tables -----------------------------------------------------------------------
def _constants():
    """REC_MAX_LEAVES, REC_MAX_WORDS, FAST_MAX_LEAVES as og_celt_rec.hpp defines them"""
    text = open(os.path.join(CSRC, "og_celt_rec.hpp")).read()
    env = {"NBANDS": 21}
    for name in ("REC_BAND_WORDS", "REC_MAX_LEAVES", "REC_MAX_WORDS", "FAST_MAX_LEAVES"):
        expr = re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1)
        assert re.fullmatch(r"[\w\s+*()]+", expr), expr
        env[name] = eval(expr, {"__builtins__": {}}, env)
    return env


def _most_leaves_and_words(LM0):
    """The most PVQ-or-fill leaves and record words any frame of 120 << LM0 samples can have, whatever its bytes: parse_tree halves a
    job while LM != -1 and N > 2 (the bit budget can only stop it earlier), parse_all_bands gives a band of width 1 no job, a
    stereo band of width 2 one job and every other band at most two; a band costs up to 3 words of padding and 4 header words, a
    job one header word and two words per leaf without pulses."""
    import rc_craft
    eb = rc_craft.rom("rom_eband")
    leaves = words = 0
    for i in range(21):
        N, LM, depth = (eb[i + 1] - eb[i]) << LM0, LM0, 0
        words += 3 + 4
        if N == 1:
            continue
        while LM != -1 and N > 2:
            N, LM, depth = N >> 1, LM - 1, depth + 1
        jobs = 2
        leaves += jobs << depth
        words += jobs * (1 + 2 * (1 << depth))
    return leaves, words


def test_no_frame_exceeds_the_record_limits():
    """Why the limit sides of RecWriter, celt_parse_lane, parse_all_bands and recon_fast_eligible are unreachable (the fixture's reason):
    the partition tree's size is bounded by the band table alone, so no frame of any length -- 1275 bytes or fewer -- writes more
    leaves or words than the record holds, and every 20 ms frame is within what the fast kernel takes."""
    k = _constants()
    src = open(os.path.join(CSRC, "og_celt_parse.hpp")).read()
    assert re.search(r"const int CC = st->channels, C = ch, LM = 3,", src)  # the lane parse decodes 20 ms frames only
    for LM0 in range(4):
        leaves, words = _most_leaves_and_words(LM0)
        assert leaves <= k["FAST_MAX_LEAVES"] <= k["REC_MAX_LEAVES"], (LM0, leaves)
        assert words < k["REC_MAX_WORDS"], (LM0, words)
    assert _most_leaves_and_words(3) == (k["FAST_MAX_LEAVES"], 1021)  # (the constant is the bound itself; the reason quotes both figures)


def test_sparse_leaves_have_at_most_13_pulses():
    """Why `k <= 13` never fails inside pvq_leaf_lane's `if (sparse)` (the fixture's reason): over every band, every LM a leaf can have
    (3 down to -1: a split halves the band and takes LM down with it) and every entry of the pulse cache, a codebook with more
    dimensions than pulses has at most 13 pulses."""
    import rc_craft
    eb, idx, bits = rc_craft.rom("rom_eband"), rc_craft.rom("rom_pulse_idx"), rc_craft.rom("rom_pulse_bits")
    most, seen = 0, 0
    for LM in range(-1, 4):
        for i in range(21):
            N = (eb[i + 1] - eb[i]) << LM if LM >= 0 else (eb[i + 1] - eb[i]) >> 1
            if idx[(LM + 1) * 21 + i] < 0 or N < 1:
                continue
            cache = bits[idx[(LM + 1) * 21 + i]:]
            for q in range(1, cache[0] + 1):
                K = q if q < 8 else (8 + (q & 7)) << ((q >> 3) - 1)  # get_pulses celt.h
                seen += 1
                if N > K:
                    most = max(most, K)
    assert seen > 1000 and most <= 13, most


def test_the_rest_kernels_lane_filter_is_recon_fast_eligible():
    """Why a fast frame never reaches recon_begin in the role RECON_REST_ONLY (the fixture's reason): k_celt_recon's lanes choose the
    frames of that role with recon_fast_eligible's conditions written out on the record's words (og_api.hip).  The two texts,
    brought to one spelling, are the same expression."""
    hdr = open(os.path.join(CSRC, "og_celt_recon.hpp")).read()
    m = re.search(r"OG_DEV bool recon_fast_eligible\(const ReconHdr &h\) \{\s*if \((.*?)\) return false;\s*return (.*?);\s*\}", hdr, re.S)
    eligible = f"!({m.group(1)}) && {m.group(2)}"
    api = open(os.path.join(CSRC, "og_api.hip")).read()
    lane = re.search(r"const bool fast = (.*?);\s*mine = !fast &&", api, re.S).group(1)
    norm = lambda t: re.sub(r"\s+", "", t.replace("recs[f0].flags", "F").replace("recs[f0].", "h.").replace("h.flags", "F").replace("fl", "F"))
    assert "const u32 fl = recs[f0].flags;" in api
    assert norm(lane) == norm(eligible), (norm(lane), norm(eligible))


def test_the_tool_and_the_gpu_test_walk_the_same_rfc_plans():
    import inspect
    import kernel_branches as kb
    import rfc_common as rc
    assert "rc.rfc_plan(name)" in inspect.getsource(kb.rfc_plan_sequences) and "rc.draw_step(" in inspect.getsource(kb.rfc_plan_sequences)
    gpu = open(os.path.join(ROOT, "tests", "test_gpu_rfc.py")).read()
    assert "rc.draw_step(oracle, plan, rng, f, channels)" in gpu and all(f'"{name}"' in gpu for name in rc.RFC_PLANS)
