"""The directed corpus tests/golden/rare_paths.json on the CPU (tests/golden/make_rare_paths.py makes it; tools/oracle_branches.py
measures it):
  * the branch tool over the corpus alone leaves no side of the baseline list untaken outside the "unreachable" and "open" sets, the
    three sets partition the baseline, and every key an entry claims is taken by that entry alone;
  * the kernel source in host emulation (tests/emul, emu_decode_frame: CELT-only and hybrid frames through the split path, SILK
    through the record path the emulation has) decodes every corpus sequence to the oracle's PCM and return code, and the oracle's
    result for every packet is the one recorded in the fixture.  What the emulation lacks: it runs one lane, so nothing of the
    64-frame parse kernels' divergence or of the pipelined routes is seen here (tests/test_gpu_rare_paths.py);
  * the arithmetic helpers the corpus is aimed at -- square root, exp2, the bit-exact cosine pair, log2lin -- in the oracle and in
    the kernel source against plain Python-integer restatements, at the corners their branch conditions name.  The log-gain clamp
    of the denormalisation is no function of its own on either side: the oracle's line runs through oc_test_denorm_coef
    (denormalise on one coefficient), the kernel's through emu_denorm_gain (denorm_gains on one band), both over band log
    energies that put lg32 at 32767 / 32768 and beyond and at every shift corner (shift > 31, == -1, <= -2).  lg32 < -32768 cannot
    be produced through either: bandLogE is 16 bits and eMeans is at least 60, so lg32 >= -32768 + 3840; that corner is checked on
    the restatement alone.
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
FIXTURE = os.path.join(ROOT, "tests", "golden", "rare_paths.json")
EMUL = os.path.join(ROOT, "tests", "emul", "libog_emul.so")


@pytest.fixture(scope="module")
def corpus():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.dirname(EMUL), "-s"])
    lib = C.CDLL(EMUL)
    lib.emu_state_size.restype = C.c_int
    lib.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
    lib.emu_decode_frame.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


# ---- the tool over the corpus -------------------------------------------------------------------------------------------------------
def test_the_three_sets_partition_the_baseline(corpus):
    base = set(corpus["baseline"])
    reached = {k for e in corpus["entries"] for k in e["keys"]}
    unreachable, open_ = set(corpus["unreachable"]), set(corpus["open"])
    assert len(base) == len(corpus["baseline"])
    assert reached <= base and unreachable <= base and open_ <= base
    assert not (reached & unreachable) and not (reached & open_) and not (unreachable & open_)
    assert reached | unreachable | open_ == base
    assert all(len(corpus["reasons"][i]) > 40 for i in corpus["unreachable"].values())  # every one says why
    assert all(len(why) > 40 for why in corpus["open"].values())                         # ... and what was tried
    assert all(1 <= len(e["packets"]) <= 8 and e["keys"] for e in corpus["entries"])
    biggest = max(os.path.getsize(os.path.join(os.path.dirname(FIXTURE), f)) for f in os.listdir(os.path.dirname(FIXTURE))
                  if f != "rare_paths.json" and os.path.isfile(os.path.join(os.path.dirname(FIXTURE), f)))
    assert os.path.getsize(FIXTURE) <= biggest
    assert not any(k.startswith("oc_celt_math.c") for k in open_)
    assert 10 * len(open_) <= len(base) - len(unreachable)  # the cap on the open set: a tenth of what is reachable
    import oracle_branches as ob
    listed = [ln.strip() for ln in ob.__doc__.split("\n") if ln.startswith("    oc_")]
    assert listed == corpus["baseline"]  # the tool's docstring carries the same baseline list
    src = "".join(open(os.path.join(ROOT, "oracle", f)).read() for f in ob.SCOPE_FILES)
    assert all(f + "(" in src for f in ob.EXCLUDED_FUNCTIONS)  # the exclusion list names functions that exist


def test_corpus_takes_what_it_claims_and_leaves_only_the_named_sides(corpus):
    import oracle_branches as ob
    seqs = [{"channels": e["channels"], "packets": e["packets"]} for e in corpus["entries"]]
    allowed = set(corpus["unreachable"]) | set(corpus["open"])
    with ob.CoverageBuild() as cov:
        res = cov.decode(seqs)
        untaken, taken = cov.untaken()
        # (lines the corpus never executes are not reported by the tool; of the baseline's sides none may be missing otherwise)
        missing = [k for k in corpus["baseline"] if k not in taken and k not in allowed]
        assert not missing, missing
        assert not [k for k in untaken if k in set(corpus["baseline"]) - allowed]
        for e, r in zip(corpus["entries"], res):
            assert r == e["expect"]  # the coverage build computes what the fixture recorded
        for i, e in enumerate(corpus["entries"]):
            cov.decode([seqs[i]])
            t = cov.untaken()[1]
            assert all(k in t for k in e["keys"]), (i, [k for k in e["keys"] if k not in t])


# ---- emulation and oracle on the corpus ---------------------------------------------------------------------------------------------
def _mode_bw(toc):
    if toc & 0x80:
        bw = 1102 + ((toc >> 5) & 3)
        return 1002, (1101 if bw == 1102 else bw)
    if (toc & 0x60) == 0x60:
        return 1001, (1105 if toc & 0x10 else 1104)
    return 1000, 1101 + ((toc >> 5) & 3)


def test_emulated_kernels_decode_the_corpus_as_the_oracle_does(corpus, emu, oracle):
    st = C.create_string_buffer(emu.emu_state_size())
    out = np.zeros((960, 2), dtype=np.int16)
    for i, e in enumerate(corpus["entries"]):
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
            r2 = emu.emu_decode_frame(st, p[1:], len(p) - 1, m, bw, pch, out.ctypes.data)
            assert r2 == r, (i, f, r, r2)
            if r > 0:
                ncmp = 960 * pch if (m == 1000 and pch < ch) else 960 * ch
                assert np.array_equal(out.reshape(-1)[:ncmp], ref[:960].reshape(-1)[:ncmp]), ("PCM", i, f, hex(p[0]))


# ---- the helpers at their corners: plain Python integers ---------------------------------------------------------------------------
def _i16(x):
    return ((x + 0x8000) & 0xFFFF) - 0x8000


def _i32(x):
    return ((x + 0x80000000) & 0xFFFFFFFF) - 0x80000000


def _m16_q15(a, b):
    return (_i16(a) * _i16(b)) >> 15


def _m16_p15(a, b):
    return (16384 + _i16(a) * _i16(b)) >> 15


def _add16(a, b):
    return _i16(_i16(a) + _i16(b))


def _vshr32(a, s):
    return a >> s if s > 0 else _i32(a << -s)


def py_sqrt(x):  # src/celt.cpp:3131
    if x == 0:
        return 0
    if x >= 1 << 30:
        return 32767
    k = ((x.bit_length() - 1) >> 1) - 7
    x = _vshr32(x, 2 * k)
    n = _i16(x - 32768)
    acc = -664
    for c in (1699, -3011, 11561, 23175):
        acc = _add16(c, _m16_q15(n, acc))
    return _vshr32(acc, 7 - k)


def py_exp2(x_in):  # celt.h:494-510
    x = _i16(x_in)
    integer = x >> 10
    if integer > 14:
        return 0x7F000000
    if integer < -15:
        return 0
    frac = _i16((_i16(x - _i16((integer << 10) & 0xFFFF)) << 4) & 0xFFFF)
    frac = _add16(16383, _m16_q15(frac, _add16(22804, _m16_q15(frac, _add16(14819, _m16_q15(10204, frac))))))
    return _vshr32(frac, -integer - 2)


def _py_cos_pi_2(x):  # src/celt.cpp:3151
    x2 = _i16(_m16_p15(x, x))
    v = (32767 - x2) + _m16_p15(x2, -7651 + _m16_p15(x2, 8277 + _m16_p15(-626, x2)))
    return _add16(1, min(32766, v))


def py_cos_norm(x):  # src/celt.cpp:3161
    x &= 0x1FFFF
    if x > 1 << 16:
        x = (1 << 17) - x
    if x & 0x7FFF:
        if x < 1 << 15:
            return _py_cos_pi_2(_i16(x))
        return _i16(-_py_cos_pi_2(_i16(65536 - x)))
    if x & 0xFFFF:
        return 0
    if x & 0x1FFFF:
        return -32767
    return 32767


def py_log2lin(q7):  # src/silk.cpp:2248
    if q7 < 0:
        return 0
    if q7 >= 3967:
        return 0x7FFFFFFF
    out = 1 << (q7 >> 7)
    frac = q7 & 0x7F
    t = frac + ((frac * (128 - frac) * -174) >> 16)  # silk_SMLAWB(frac, silk_SMULBB(frac, 128 - frac), -174)
    if q7 < 2048:
        return _i32(out + ((out * t) >> 7))
    return _i32(out + (out >> 7) * t)


def py_log_gain(bandLogE, emean):  # src/celt.cpp:958-962: the clamp to 16 bits of lg = bandLogE + (eMeans << 6)
    lg32 = bandLogE + (emean << 6)
    return 32767 if lg32 > 32767 else (-32768 if lg32 < -32768 else lg32)


def py_denorm_gain(bandLogE, emean):  # src/celt.cpp:958-996 -> (gain, shift)
    lg = py_log_gain(bandLogE, emean)
    shift = 16 - (lg >> 10)
    if shift > 31:
        shift, g = 0, 0
    else:
        f = _i16(((lg & 1023) << 4) & 0xFFFF)
        g = _add16(16383, _m16_q15(f, _add16(22804, _m16_q15(f, _add16(14819, _m16_q15(10204, f))))))
    if shift <= -2:
        g, shift = 16384, -2
    return g, shift


def py_denorm_coef(bandLogE, emean, x):
    g, shift = py_denorm_gain(bandLogE, emean)
    p = _i16(x) * _i16(g)
    return _i32(p << -shift) if shift < 0 else p >> shift


def _emeans():
    import rc_craft
    return rc_craft.rom("rom_emeans")


def _log_gain_corners(emean):
    """band log energies that put lg32 = E + (emean << 6) at the clamp's and the shift's corners, within 16 bits"""
    want = [32766, 32767, 32768, 32769, 40000,                # the upper clamp
            -16 * 1024 - 1, -16 * 1024, -15 * 1024 - 1, -15 * 1024,  # shift 33 / 32 / 32 / 31: `shift > 31`
            16 * 1024 - 1, 16 * 1024, 17 * 1024 - 1, 17 * 1024, 18 * 1024 - 1, 18 * 1024, 31 * 1024,  # shift 1, 0, 0, -1, -1, -2, -15
            0, 1023, 1024, -1]
    es = {w - (emean << 6) for w in want} | {-32768, 32767}   # (-32768: the lowest lg32 there is, -32768 + (emean << 6))
    return sorted(e for e in es if -32768 <= e <= 32767)


SQRT_CORNERS = [0, 1, 2, 3, 4, 255, 256, 32767, 32768, 65535, 65536, (1 << 22), 176 << 22, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, 0x7FFFFFFF]
EXP2_CORNERS = [0, 1, -1, 1023, 1024, -1024, 14 << 10, (14 << 10) + 1023, 15 << 10, (15 << 10) + 1, 31 << 10, -(15 << 10), -(15 << 10) - 1,
                -(16 << 10), -32768, 32767]
COS_CORNERS = [0, 1, 32767, 32768, 32769, 65535, 65536, 65537, 98303, 98304, 98305, 131071, 131072, 16384, 49152, -1, 1 << 17 | 5]
LOG2LIN_CORNERS = [-1, 0, 1, 127, 128, 2047, 2048, 2049, 2090, 3924, 3966, 3967, 3968, 1 << 20, -(1 << 20)]


def test_python_restatements_at_their_own_known_values():
    """the restatements pinned without either implementation: exact powers, and values read off the reference's formulas by hand"""
    assert py_sqrt(0) == 0 and py_sqrt(1 << 30) == 32767 and py_sqrt((1 << 30) + 7) == 32767
    assert abs(py_sqrt(1 << 28) - (1 << 14)) <= 16 and abs(py_sqrt(1 << 16) - 256) <= 1  # (a degree-4 polynomial: good to about 2^-11)
    assert py_exp2(15 << 10) == 0x7F000000 and py_exp2(-(16 << 10)) == 0
    assert abs(py_exp2(0) - 65536) <= 8 and abs(py_exp2(-1024) - 32768) <= 4 and abs(py_exp2(14 << 10) - (1 << 30)) <= 1 << 17
    assert py_cos_norm(0) == 32767 and py_cos_norm(32768) == 0 and py_cos_norm(65536) == -32767 and py_cos_norm(98304) == 0
    assert py_cos_norm(131072) == 32767 and py_cos_norm(1) == py_cos_norm(131071)  # the fold
    assert py_log2lin(-1) == 0 and py_log2lin(3967) == 0x7FFFFFFF and py_log2lin(0) == 1 and py_log2lin(2048) == 1 << 16
    assert py_log2lin(128) == 2 and py_log2lin(3966) < 0x7FFFFFFF
    assert py_log_gain(32767, 1) == 32767 and py_log_gain(-28 * 1024, 0) == -28672 and py_log_gain(-32768, -1) == -32768
    assert py_log_gain(32767 - 64, 1) == 32767 and py_log_gain(32767 - 65, 1) == 32766
    assert py_log_gain(-32769, 0) == -32768 and py_log_gain(-32768, 0) == -32768 and py_log_gain(32768, 0) == 32767
    assert py_denorm_gain(-16 * 1024, 0) == (0, 0) and py_denorm_gain(-15 * 1024, 0)[1] == 31  # shift > 31 gives nothing
    assert py_denorm_gain(17 * 1024, 0) == (16383, -1) and py_denorm_gain(18 * 1024, 0) == (16384, -2) == py_denorm_gain(32767, 1)
    assert py_denorm_coef(0, 0, 16384) == (16384 * 16383) >> 16 and py_denorm_coef(17 * 1024, 0, 3) == 3 * 16383 * 2


def test_oracle_helpers_at_the_corners(oracle):
    lib = oracle.lib
    for f in (lib.oc_sqrt, lib.oc_exp2, lib.oc_test_log2lin):
        f.argtypes, f.restype = [C.c_int32], C.c_int32
    lib.oc_cos_norm.argtypes, lib.oc_cos_norm.restype = [C.c_int32], C.c_int16
    for x in SQRT_CORNERS:
        assert lib.oc_sqrt(x) == py_sqrt(x), ("sqrt", x)
    for x in EXP2_CORNERS:
        assert lib.oc_exp2(x) == py_exp2(x), ("exp2", x)
    for x in COS_CORNERS:
        assert lib.oc_cos_norm(x) == py_cos_norm(x), ("cos_norm", x)
    for x in LOG2LIN_CORNERS:
        assert lib.oc_test_log2lin(x) == py_log2lin(x), ("log2lin", x)


def test_kernel_helpers_at_the_corners(emu):
    for f in (emu.emu_celt_sqrt, emu.emu_celt_exp2, emu.emu_cos_norm, emu.emu_silk_log2lin):
        f.argtypes, f.restype = [C.c_int32], C.c_int32
    for x in SQRT_CORNERS:
        assert emu.emu_celt_sqrt(x) == py_sqrt(x), ("celt_sqrt", x)
    for x in EXP2_CORNERS:
        assert emu.emu_celt_exp2(x) == py_exp2(x), ("celt_exp2", x)
    for x in COS_CORNERS:
        assert _i16(emu.emu_cos_norm(x)) == py_cos_norm(x), ("cos_norm", x)
    for x in LOG2LIN_CORNERS:
        assert emu.emu_silk_log2lin(x) == py_log2lin(x), ("silk_log2lin", x)


def test_oracle_log_gain_at_the_corners(oracle):
    f = oracle.lib.oc_test_denorm_coef
    f.argtypes, f.restype = [C.c_int, C.c_int, C.c_int], C.c_int32
    em = _emeans()
    shifts = set()
    for band in (0, 5, 20):
        for e in _log_gain_corners(em[band]):
            shifts.add(py_denorm_gain(e, em[band])[1])
            for x in (16384, -16384, 1, -1, 32767, -32768, 12345):
                assert f(band, e, x) == py_denorm_coef(e, em[band], x), (band, e, x)
    assert {0, 31, 1, -1, -2} <= shifts


def test_kernel_log_gain_at_the_corners(emu):
    f = emu.emu_denorm_gain
    f.argtypes, f.restype = [C.c_int, C.c_int], C.c_int32
    em = _emeans()
    for band in (0, 5, 20):
        for e in _log_gain_corners(em[band]):
            v = f(band, e)
            assert (_i16(v & 0xFFFF), v >> 16) == py_denorm_gain(e, em[band]), (band, e)


def test_a_mono_split_never_has_qn_1():
    """Why `} else if (stereo) {` in compute_theta never sees a mono band (the fixture's reason for that side): quant_partition splits
    a band only for b > cache[cache[0]] + 12 (src/celt.cpp:1400), compute_qn answers 1 only for qb < 4 (src/celt.cpp:1229), qb does
    not fall when b grows, and over every band, both frame sizes of reference mode (LM 3, and 0 for the 2.5 ms frame) and every
    depth of the recursion the smallest b that splits leaves qb far above 4."""
    import rc_craft
    eb, logn = rc_craft.rom("rom_eband"), rc_craft.rom("rom_logn")
    idx, bits = rc_craft.rom("rom_pulse_idx"), rc_craft.rom("rom_pulse_bits")
    lowest, splits = None, 0
    for LM0 in (0, 3):
        for i in range(21):
            N, LM = (eb[i + 1] - eb[i]) << LM0, LM0
            while LM != -1 and N > 2:  # quant_partition's condition besides b
                cache = bits[idx[(LM + 1) * 21 + i]:]
                b = cache[cache[0]] + 12 + 1
                N, LM = N >> 1, LM - 1
                pulse_cap = logn[i] + LM * 8
                offset = (pulse_cap >> 1) - 4
                N2 = 2 * N - 1
                assert b + N2 * offset >= 0  # (so that // is C's division)
                qb = min((b + N2 * offset) // N2, b - pulse_cap - 32, 64)
                lowest = qb if lowest is None else min(lowest, qb)
                splits += 1
    assert splits > 60 and lowest >= 4, lowest
