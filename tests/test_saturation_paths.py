"""The directed corpus tests/golden/saturation_paths.json on the CPU (tests/golden/make_saturation_paths.py makes it;
tools/oracle_saturation.py measures it): packets that make the saturating helpers of oracle/oc_math.h clamp at the call sites
where random payloads clamp rarely or never -- first of all the LPC synthesis update, add_sat32(residual, lshift_sat32(prediction,
4)), which a kernel could compute with a wrapping add and pass every test of random payloads at the suite's sizes.
  * the oracle's result for every corpus packet is the fixture's; the census over the corpus gives every entry the clamps it
    claims; the census over the suite's random payload families is the fixture's baseline; every site of oc_silk.c, oc_celt.c,
    oc_celt_math.c and oc_packet.c has one verdict, and the verdicts follow from the two censuses;
  * per class of (NB, MB, WB, the SILK layer of hybrid FB) x (unvoiced, voiced) x (mono, stereo packet with the side channel absent),
    from the positions report of the census and not from any kernel: add_sat32 and lshift_sat32 of the synthesis update each
    clamp high and low at least 16 times; a clamp falls on every sample index mod 4 (the row form's four samples per trip), in the
    first and in the last subframe, and on sample 0 of a frame whose history the frame before left saturated (an add_sat32 clamp
    among its last 10 samples: the shortest filter's history).  An empty class fails.  In RFC mode the same frames, each followed by
    a lost packet, clamp the concealment's synthesis update and output and the mix of the concealed layers on both sides;
  * the kernel source in host emulation decodes every corpus stream to the oracle's PCM, return codes and SILK stage values: the
    split path, the single kernel, the narrowband layout (NB entries) and RFC mode with the losses.  (Of the two tight layouts
    tests/emul builds, the other, libog_emul_tight.so, decodes CELT-only frames alone, and the corpus has none in reference
    mode: its CELT-only entries are the RFC ones with losses.)  For each site of the synthesis update, the census build with that
    one operation wrapping gives another PCM for the entries the fixture names: the clamps are visible.  The emulation runs the
    one-lane synthesis core (og_silk.hpp silk_decode_core_lane); the row form of the synthesis kernels exists on the GPU only
    (tests/test_gpu_saturation_paths.py);
  * the helpers themselves -- og_common.hpp's through tests/emul, oc_math.h's through a library built here -- against Python
    integers at INT32_MIN, INT32_MAX, +-1 around every clamp threshold and shifts 0..31; and the two value-range arguments of the
    fixture's "unreachable" sites, walked over every gain index.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "saturation_paths.json")
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

from rfc_common import dur  # noqa: E402
from test_rare_paths import _mode_bw, py_log2lin  # noqa: E402


@pytest.fixture(scope="module")
def corpus():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def census(corpus):
    """the tool over the whole corpus, with positions, once"""
    import oracle_saturation as osat
    with osat.CensusBuild() as cb:
        seqs = [{"channels": e["channels"], "packets": e["packets"], "rfc": e["rfc"]} for e in corpus["entries"]]
        whole = cb.decode(seqs, positions=True)
        alone = [cb.decode([s])["sites"] for s in seqs]
    return whole, alone


def _emu(name):
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", name])
    lib = C.CDLL(os.path.join(EMUL_DIR, name))
    lib.emu_state_size.restype = C.c_int
    lib.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
    for f in (lib.emu_decode_frame, lib.emu_decode_frame_single):
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.emu_decode_frame_rfc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.emu_tap_silk.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def emu():
    return _emu("libog_emul.so")


# ---- the fixture and the tool --------------------------------------------------------------------------------------------------------
def test_every_site_has_a_verdict_that_follows_from_the_counts(corpus):
    import oracle_saturation as osat
    import make_saturation_paths as msp
    keys = {k for k in osat.static_sites().values() if k.split("|")[0] in osat.SITE_FILES}
    assert keys == set(corpus["baseline"]) == set(corpus["verdicts"])
    total = {}
    for e in corpus["entries"]:
        assert 1 <= len(e["packets"]) <= 4 and all(len(p) <= 2 * 251 for p in e["packets"]) and e["keys"]
        assert e["rfc"] or all(e["packets"])  # a lost packet only where there is concealment
        for k, (hi, lo) in e["keys"].items():
            t = total.setdefault(k, [0, 0])
            t[0], t[1] = t[0] + hi, t[1] + lo
    for k, v in corpus["verdicts"].items():
        calls, hi, lo = corpus["baseline"][k]
        un = corpus["unreachable"].get(k, {})
        got = total.get(k, [0, 0])
        if v.startswith("abundant"):
            assert hi >= 1000 and lo >= 1000 and str(hi) in v and str(lo) in v, k
        elif v == "open":
            assert len(corpus["open"][k]) > 40, k  # says what was tried
        else:
            assert (got[0] > 0 or "high" in un) and (got[1] > 0 or "low" in un), (k, v, got)
            assert all(len(corpus["reasons"][i]) > 40 for i in un.values())
            assert not (got[0] and "high" in un) and not (got[1] and "low" in un), ("clamped where the fixture argues it cannot", k)
        assert (k in corpus["open"]) == (v == "open")
    assert len(corpus["open"]) <= 3
    assert not [k for k in corpus["open"] if "decode_core" in k or "plc_conceal" in k or "oc_packet.c" in k]
    assert sorted(w for _, _, w in msp.UNREACHABLE) == sorted(corpus["reasons"])
    assert os.path.getsize(FIXTURE) < 200 * 1024


def test_census_over_the_corpus_is_what_the_entries_claim(corpus, census):
    whole, alone = census
    for i, (e, sites) in enumerate(zip(corpus["entries"], alone)):
        assert whole["results"][i] == e["expect"], ("the census build decodes something else", i)
        got = {k: v[1:] for k, v in sites.items() if k in corpus["verdicts"] and not corpus["verdicts"][k].startswith("abundant") and (v[1] or v[2])}
        assert got == e["keys"], (i, e.get("class"))


def test_baseline_census_is_the_fixtures(corpus):
    import oracle_saturation as osat
    with osat.CensusBuild() as cb:
        sites = cb.decode(osat.ob.baseline_sequences())["sites"]
    assert {k: v for k, v in sites.items() if k in corpus["baseline"]} == corpus["baseline"]


def test_every_class_clamps_where_the_row_form_could_go_wrong(corpus, census):
    import make_saturation_paths as msp
    whole, _ = census
    seen = set()
    for i, e in enumerate(corpus["entries"]):
        cls = tuple(e.get("class", "").split("-"))
        if cls not in msp.CLASSES:
            continue
        seen.add(cls)
        band, voicing, chans = cls
        toc = msp.BANDS[band][0] | (4 if chans == "stereo" else 0)
        assert not e["rfc"] and e["channels"] == (2 if chans == "stereo" else 1)
        assert all(int(p[:2], 16) == toc for p in e["packets"]) and all(r[0] == 960 for r in e["expect"])
        counts, mod4, first, last, carried = msp.class_report(whole["positions"], i, band, len(e["packets"]))
        assert all(v >= 16 for c in counts.values() for v in c), (cls, counts)
        assert mod4 == {0, 1, 2, 3} and first and last and carried, (cls, mod4, first, last, carried)
    assert seen == set(msp.CLASSES)  # no class is empty
    lossy = [e for e in corpus["entries"] if e.get("class", "").endswith("-lossy")]
    assert len(lossy) == len(msp.CLASSES) and all(e["rfc"] and e["packets"][1::2] == ["", ""] for e in lossy)
    rfc = [e for e in corpus["entries"] if e["rfc"]]  # (the mix of the concealed layers clamps where a hybrid stream's CELT layer is loud too)
    for part, among in (("plc_conceal|sLPC[MAX_LPC + i] = add_sat32", lossy), ("plc_conceal|frame[i] = sat16", lossy),
                        ("oc_packet.c|conceal_frame|", rfc)):
        ks = [k for k in corpus["verdicts"] if part in k]
        assert ks
        for k in ks:
            assert sum(e["keys"].get(k, [0, 0])[0] for e in among) > 0 and sum(e["keys"].get(k, [0, 0])[1] for e in among) > 0, k


def test_a_wrapping_synthesis_update_changes_the_pcm(corpus):
    """A clamp protects only where the output shows it: the comfort noise's synthesis is scaled by a gain that is 0 behind a loud last
    frame, and then a wrong kernel's saturated state changes no sample.  For each site of the LPC synthesis update -- decoded
    frames, concealment, comfort noise; add_sat32 and lshift_sat32 -- the fixture names the entries whose PCM changes when that one
    operation WRAPS in the census build, as a wrong kernel's would; here each of them is decoded so and must differ from the
    fixture's result in a packet's crc."""
    import oracle_saturation as osat
    import make_saturation_paths as msp
    shows = corpus["shows_a_wrapping_update"]
    assert set(shows) == set(msp.UPDATE_KEYS)
    with osat.CensusBuild() as cb:
        for key, who in shows.items():
            assert who, key
            ents = [corpus["entries"][i] for i in who]
            assert all(sum(e["keys"][key]) > 0 for e in ents), key
            wrapped = cb.decode([{"channels": e["channels"], "packets": e["packets"], "rfc": e["rfc"]} for e in ents], wrap=key)["results"]
            for i, e, w in zip(who, ents, wrapped):
                assert [r[0] for r in w] == [r[0] for r in e["expect"]] and w != e["expect"], (key, i)


def test_classes_voicing_is_what_the_oracle_decodes(corpus, oracle):
    """the class names are claims about the frames: signal type 2 for the voiced ones, the side channel not coded in the stereo ones"""
    oracle.lib.oc_silk_taps_copy.argtypes = [C.c_int, C.c_int, C.c_void_p]
    oracle.lib.oc_silk_taps_enable.argtypes = [C.c_int]
    oracle.lib.oc_silk_taps_enable(1)
    try:
        for e in corpus["entries"]:
            cls = e.get("class", "").split("-")
            if len(cls) != 3:
                continue
            d = oracle.decoder(e["channels"])
            d.init()
            for hx in e["packets"]:
                d.decode(bytes.fromhex(hx))
                b = np.zeros(6, dtype=np.int32)
                assert oracle.lib.oc_silk_taps_copy(0, 0, b.ctypes.data) >= 0
                assert b[0] and (b[1] == 2) == (cls[1] == "voiced"), (cls, b)
                if cls[2] == "stereo":
                    assert oracle.lib.oc_silk_taps_copy(0, 1, b.ctypes.data) >= 0
                    assert not b[0], cls
    finally:
        oracle.lib.oc_silk_taps_enable(0)


# ---- emulation and oracle on the corpus ---------------------------------------------------------------------------------------------
def _silk_taps_equal(emu, oracle, pch, where):
    for ch in range(pch):
        def both(what, dtype, count):
            a, b = np.zeros(count, dtype=dtype), np.zeros(count, dtype=dtype)
            assert emu.emu_tap_silk(what, ch, a.ctypes.data) >= 0 and oracle.lib.oc_silk_taps_copy(what, ch, b.ctypes.data) >= 0
            return a, b
        sa, sb = both(0, np.int32, 6)
        assert bool(sa[0]) == bool(sb[0]), ("coded", where, ch)
        if not sb[0]:
            continue
        flen, order = int(sb[3]), int(sb[4])
        assert (sa[1], sa[2], sa[5]) == (sb[1], sb[2], sb[5]), ("signal type / offset type / LTP scale", where, ch)
        a, b = both(1, np.int32, 8)
        assert (a == b).all(), ("pitch lags / gains", where, ch)
        a, b = both(2, np.int16, 32)
        assert (a.reshape(2, 16)[:, :order] == b.reshape(2, 16)[:, :order]).all(), ("LPC coefficients", where, ch)
        a, b = both(3, np.int16, 20)
        assert (a == b).all(), ("LTP coefficients", where, ch)
        a, b = both(4, np.int16, 320)
        assert (a[:flen] == b[:flen]).all(), ("synthesis core output", where, ch, np.argwhere(a[:flen] != b[:flen])[:4].tolist())


def _reference_entries(corpus, emu, oracle, entry, only=lambda e: True):
    oracle.lib.oc_silk_taps_copy.argtypes = [C.c_int, C.c_int, C.c_void_p]
    oracle.lib.oc_silk_taps_enable.argtypes = [C.c_int]
    st = C.create_string_buffer(emu.emu_state_size())
    out = np.zeros((960, 2), dtype=np.int16)
    ran = 0
    oracle.lib.oc_silk_taps_enable(1)
    try:
        for i, e in enumerate(corpus["entries"]):
            if e["rfc"] or not only(e):
                continue
            ch = e["channels"]
            d = oracle.decoder(ch)
            d.init()
            emu.emu_stream_init(st, ch)
            for f, (hx, exp) in enumerate(zip(e["packets"], e["expect"])):
                p = bytes.fromhex(hx)
                ref, r = d.decode(p)
                got = [r, oracle.lib.oc_decoder_final_range(d.h), zlib.crc32(ref[:max(r, 0)].tobytes())]
                assert got == exp, ("the oracle's result is not the fixture's", i, f, got, exp)
                m, bw = _mode_bw(p[0])
                pch = 2 if p[0] & 4 else 1
                out[:] = 0
                r2 = entry(st, p[1:], len(p) - 1, m, bw, pch, out.ctypes.data)
                assert r2 == r, (i, f, r, r2)
                if r > 0:
                    if m != 1002:
                        _silk_taps_equal(emu, oracle, pch, (i, e.get("class"), f))  # first: a difference names the stage
                    ncmp = 960 * pch if (m == 1000 and pch < ch) else 960 * ch
                    assert np.array_equal(out.reshape(-1)[:ncmp], ref[:960].reshape(-1)[:ncmp]), ("PCM", i, e.get("class"), f, hex(p[0]))
                ran += 1
    finally:
        oracle.lib.oc_silk_taps_enable(0)
    return ran


def test_emulated_split_path_decodes_the_corpus_as_the_oracle_does(corpus, emu, oracle):
    assert _reference_entries(corpus, emu, oracle, emu.emu_decode_frame) >= 16 * 3


def test_emulated_single_kernel_decodes_the_corpus_as_the_oracle_does(corpus, emu, oracle):
    assert _reference_entries(corpus, emu, oracle, emu.emu_decode_frame_single) >= 16 * 3


def test_emulated_narrowband_layout_decodes_the_nb_entries_as_the_oracle_does(corpus, oracle):
    nb = _emu("libog_emul_nb.so")  # the SILK working set sized for 8 kHz, under the bounds sanitizer
    only = lambda e: all((int(p[:2], 16) & 0xE0) == 0 for p in e["packets"])  # noqa: E731
    assert _reference_entries(corpus, nb, oracle, nb.emu_decode_frame, only) >= 4 * 3


def test_emulated_rfc_mode_decodes_and_conceals_the_corpus_as_the_oracle_does(corpus, emu, oracle):
    st = C.create_string_buffer(emu.emu_state_size())
    ran = lost = 0
    for i, e in enumerate(corpus["entries"]):
        if not e["rfc"]:
            continue
        ch = e["channels"]
        d = oracle.decoder(ch)
        d.init()
        d.set_rfc(True)
        emu.emu_stream_init(st, ch)
        m, bw, pch = 1002, 1105, ch  # what a loss before any packet would be concealed as
        for f, (hx, exp) in enumerate(zip(e["packets"], e["expect"])):
            p = bytes.fromhex(hx)
            if p:
                ref, r = d.decode(p)
                (m, bw), pch, pay = _mode_bw(p[0]), (2 if p[0] & 4 else 1), p[1:]
                assert (p[0] & 3) == 0 and dur(p[0]) == 960  # one 20 ms frame
            else:
                ref, r = d.conceal(960)
                pay = b""
                lost += 1
            got = [r, oracle.lib.oc_decoder_final_range(d.h), zlib.crc32(ref[:max(r, 0)].tobytes())]
            assert got == exp, ("the oracle's result is not the fixture's", i, f, got, exp)
            out = np.zeros((960, ch), dtype=np.int16)
            r2 = emu.emu_decode_frame_rfc(st, pay, len(pay), m, bw, pch, out.ctypes.data, 960)
            assert r2 == r == 960, (i, f, r, r2)
            ncmp = 960 * pch if (m == 1000 and pch < ch) else 960 * ch
            assert np.array_equal(out.reshape(-1)[:ncmp], ref[:960].reshape(-1)[:ncmp]), ("PCM", i, e.get("class"), f, "lost" if not p else hex(p[0]))
            ran += 1
    assert ran >= 16 * 4 and lost >= 16 * 2


# ---- the helpers: plain Python integers ---------------------------------------------------------------------------------------------
def _i32(x):
    return ((x + 0x80000000) & 0xFFFFFFFF) - 0x80000000


def py_add_sat32(a, b):  # silk.h:480
    return max(I32_MIN, min(I32_MAX, a + b))


def py_sub_sat32(a, b):  # silk.h:483
    return max(I32_MIN, min(I32_MAX, a - b))


def py_limit32(a, l1, l2):  # silk.h:427: the limits in either order
    return max(min(l1, l2), min(max(l1, l2), a))


def py_lshift_sat32(a, s):  # silk.h:139
    return _i32(py_limit32(a, I32_MIN >> s, I32_MAX >> s) << s)


def py_sat16(x):  # celt.h:401
    return max(-32768, min(32767, x))


EDGES = sorted({I32_MIN, I32_MIN + 1, I32_MIN + 2, -(1 << 30) - 1, -(1 << 30), -(1 << 30) + 1, -32769, -32768, -32767, -2, -1, 0, 1, 2,
                32766, 32767, 32768, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, I32_MAX - 2, I32_MAX - 1, I32_MAX})


def _helper_cases():
    add = [(a, b) for a in EDGES for b in EDGES]  # (every sum within +-1 of either bound is among them: a + b = bound + d, d in -2..2)
    shift = []
    for s in range(32):
        hi, lo = I32_MAX >> s, I32_MIN >> s
        shift += [(a, s) for a in sorted({hi - 1, hi, hi + 1, lo - 1, lo, lo + 1, 0, 1, -1, I32_MIN, I32_MAX}) if I32_MIN <= a <= I32_MAX]
    limit = []
    for l1, l2 in [(0, 63), (63, 0), (-32768, 32767), (32767, -32768), (16, 288), (5, 5), (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (-7, -3)]:
        for t in {l1, l2}:
            limit += [(a, l1, l2) for a in (t - 1, t, t + 1) if I32_MIN <= a <= I32_MAX]
        limit += [(I32_MIN, l1, l2), (I32_MAX, l1, l2), (0, l1, l2)]
    sat = [-32770, -32769, -32768, -32767, 32766, 32767, 32768, 32769, 0, -1, 1, I32_MIN, I32_MAX, 65535, 65536, -65536]
    return add, shift, limit, sat


def _check_helpers(f_add, f_sub, f_shift, f_limit, f_sat, who):
    add, shift, limit, sat = _helper_cases()
    for a, b in add:
        assert f_add(a, b) == py_add_sat32(a, b), (who, "add_sat32", a, b)
        assert f_sub(a, b) == py_sub_sat32(a, b), (who, "sub_sat32", a, b)
    for a, s in shift:
        assert f_shift(a, s) == py_lshift_sat32(a, s), (who, "lshift_sat32", a, s)
    for a, l1, l2 in limit:
        assert f_limit(a, l1, l2) == py_limit32(a, l1, l2), (who, "limit32", a, l1, l2)
    for x in sat:
        assert f_sat(x) == py_sat16(x), (who, "sat16", x)


def test_python_restatements_at_their_own_known_values():
    assert py_add_sat32(I32_MAX, 1) == I32_MAX and py_add_sat32(I32_MIN, -1) == I32_MIN and py_add_sat32(I32_MAX, I32_MIN) == -1
    assert py_sub_sat32(I32_MIN, 1) == I32_MIN and py_sub_sat32(0, I32_MIN) == I32_MAX and py_sub_sat32(-1, I32_MIN) == I32_MAX
    assert py_lshift_sat32(1 << 27, 4) == I32_MAX >> 4 << 4 == 0x7FFFFFF0 and py_lshift_sat32((1 << 27) - 1, 4) == 0x7FFFFFF0
    assert py_lshift_sat32(-(1 << 27) - 1, 4) == I32_MIN and py_lshift_sat32(-(1 << 27), 4) == I32_MIN and py_lshift_sat32(5, 0) == 5
    assert py_lshift_sat32(I32_MAX, 31) == 0 and py_lshift_sat32(I32_MIN, 31) == I32_MIN and py_lshift_sat32(1, 31) == 0
    assert py_limit32(70, 0, 63) == 63 == py_limit32(70, 63, 0) and py_limit32(-1, 63, 0) == 0 and py_limit32(7, 63, 0) == 7
    assert py_sat16(32768) == 32767 and py_sat16(-32769) == -32768 and py_sat16(-32768) == -32768


def test_kernel_helpers_at_the_clamp_thresholds(emu):
    for f, n in ((emu.emu_add_sat32, 2), (emu.emu_sub_sat32, 2), (emu.emu_lshift_sat32, 2), (emu.emu_limit32, 3), (emu.emu_sat16, 1)):
        f.argtypes, f.restype = [C.c_int32] * n, C.c_int32
    _check_helpers(emu.emu_add_sat32, emu.emu_sub_sat32, emu.emu_lshift_sat32, emu.emu_limit32, emu.emu_sat16, "og_common.hpp")


def test_oracle_helpers_at_the_clamp_thresholds(tmp_path):
    src = tmp_path / "kat.c"
    src.write_text('#include "oc_math.h"\n'
                   "i32 k_add_sat32(i32 a, i32 b) { return add_sat32(a, b); }\ni32 k_sub_sat32(i32 a, i32 b) { return sub_sat32(a, b); }\n"
                   "i32 k_lshift_sat32(i32 a, int s) { return lshift_sat32(a, s); }\ni32 k_limit32(i32 a, i32 l1, i32 l2) { return limit32(a, l1, l2); }\n"
                   "i32 k_sat16(i32 x) { return sat16(x); }\ni32 k_satsym(i32 x, i32 a) { return satsym(x, a); }\n")
    so = str(tmp_path / "libkat.so")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-fwrapv", "-I", os.path.join(ROOT, "oracle"), str(src), "-o", so])
    lib = C.CDLL(so)
    for f, n in ((lib.k_add_sat32, 2), (lib.k_sub_sat32, 2), (lib.k_lshift_sat32, 2), (lib.k_limit32, 3), (lib.k_sat16, 1), (lib.k_satsym, 2)):
        f.argtypes, f.restype = [C.c_int32] * n, C.c_int32
    _check_helpers(lib.k_add_sat32, lib.k_sub_sat32, lib.k_lshift_sat32, lib.k_limit32, lib.k_sat16, "oc_math.h")
    for x in (300000000, 300000001, 299999999, -300000000, -300000001, -299999999, 0, I32_MAX, I32_MIN + 1):
        assert lib.k_satsym(x, 300000000) == max(-300000000, min(300000000, x)), ("satsym", x)


# ---- the value-range arguments of the unreachable sites, walked -------------------------------------------------------------------------
def _clz32(x):
    return 32 - x.bit_length() if x else 32


def _smulwb(a, b):
    return _i32((a * (((b + 0x8000) & 0xFFFF) - 0x8000)) >> 16)


def test_the_gain_divisions_never_shift_into_their_clamp():
    """oc_silk.c div32_varQ / inverse32_varQ with the only arguments decode_core has for them: gains of index 0..63"""
    gains = [py_log2lin(min(_smulwb(1907825, idx) + 2090, 3967)) for idx in range(64)]
    assert min(gains) >= 1 << 16 and max(gains) < 1 << 31
    for b in gains:  # inverse32_varQ(gain, 47): lshift = 61 - b_headrm - 47; the clamp is called for lshift <= 0, with shift -lshift
        assert 61 - (_clz32(b) - 1) - 47 >= 0
    worst = 0
    for a in gains:  # div32_varQ(previous gain, gain, 16): silk.h:913-940 restated
        for b in gains:
            ah, bh = _clz32(a) - 1, _clz32(b) - 1
            a_nrm, b_nrm = _i32(a << ah), _i32(b << bh)
            inv = (I32_MAX >> 2) // (b_nrm >> 16)
            res = _smulwb(a_nrm, inv)
            a_nrm = _i32(a_nrm - _i32(((b_nrm * res) >> 32) << 3))
            res = _i32(res + _smulwb(a_nrm, inv))
            lshift = 29 + ah - bh - 16
            assert lshift >= -1
            if lshift < 0:
                worst = max(worst, res)
                assert (I32_MIN >> 1) <= res <= (I32_MAX >> 1), (a, b, res)
    assert worst > 0  # the shift by one does occur
