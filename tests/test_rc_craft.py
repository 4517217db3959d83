"""tests/rc_craft.py on the CPU.
The range encoder against the oracle's range decoder (oracle/oc_range.c): random symbol sequences over random models come back
symbol for symbol, and the decoder's final range equals the encoder's.
The frame writers: what a CELT or SILK frame pins is read back through the oracle's stage taps."""
import ctypes as C
import random

import pytest

import rc_craft


class RC(C.Structure):  # oc_rc, oracle/oc_opus.h
    _fields_ = [("buf", C.c_char_p), ("storage", C.c_uint32), ("end_offs", C.c_uint32), ("end_window", C.c_uint32),
                ("nend_bits", C.c_int32), ("nbits_total", C.c_int32), ("offs", C.c_uint32), ("rng", C.c_uint32), ("val", C.c_uint32),
                ("ext", C.c_uint32), ("rem", C.c_int32), ("error", C.c_int32)]


def _bind(lib):
    p = C.POINTER(RC)
    lib.oc_rc_init.argtypes = [p, C.c_char_p, C.c_uint32]
    lib.oc_rc_decode.argtypes = [p, C.c_uint32]
    lib.oc_rc_decode.restype = C.c_uint32
    lib.oc_rc_update.argtypes = [p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.oc_rc_bit_logp.argtypes = [p, C.c_uint]
    lib.oc_rc_icdf.argtypes = [p, C.c_char_p, C.c_uint]
    lib.oc_rc_uint.argtypes = [p, C.c_uint32]
    lib.oc_rc_uint.restype = C.c_uint32
    lib.oc_rc_bits.argtypes = [p, C.c_uint]
    lib.oc_rc_bits.restype = C.c_uint32
    lib.oc_rc_laplace.argtypes = [p, C.c_uint32, C.c_int]
    return lib


def _random_icdf(r):
    n = r.randint(2, 12)
    ftb = r.choice([2, 5, 7, 8])
    n = min(n, 1 << ftb)
    cuts = sorted(r.sample(range(1, 1 << ftb), n - 1), reverse=True)
    return cuts + [0], ftb


def _random_symbols(r, count):
    syms = []
    for _ in range(count):
        kind = r.choice(["encode", "bit", "icdf", "uint", "bits", "laplace"])
        if kind == "encode":
            ft = r.randint(2, 60000)
            fl = r.randrange(ft)
            syms.append((kind, fl, r.randint(fl + 1, min(ft, fl + 1 + r.choice([0, 3, 1000]))), ft))
        elif kind == "bit":
            logp = r.randint(1, 15)
            syms.append((kind, int(r.random() < 2.0 ** -logp * 4), logp))
        elif kind == "icdf":
            t, ftb = _random_icdf(r)
            syms.append((kind, r.randrange(len(t)), t, ftb))
        elif kind == "uint":
            ft = r.choice([2, 6, 255, 256, 257, 1000, 70000, (1 << 24) + 5, (1 << 32) - 1])
            syms.append((kind, r.randrange(ft), ft))
        elif kind == "bits":
            n = r.randint(1, 16)
            syms.append((kind, r.randrange(1 << n), n))
        else:
            fs, decay = r.choice([(72 << 7, 127 << 6), (42 << 7, 121 << 6), (15 << 7, 9 << 6), (96 << 7, 60 << 6)])
            syms.append((kind, r.choice([0, 0, 1, -1, 2, -3, 7, -12]), fs, decay))
    return syms


@pytest.mark.parametrize("seed", range(40))
def test_every_symbol_comes_back_and_the_ranges_agree(oracle, seed):
    lib = _bind(oracle.lib)
    r = random.Random(seed)
    syms = _random_symbols(r, r.choice([1, 3, 20, 200]))
    e = rc_craft.Encoder()
    for s in syms:
        getattr(e, {"encode": "encode", "bit": "bit_logp", "icdf": "icdf", "uint": "uint", "bits": "bits", "laplace": "laplace"}[s[0]])(*s[1:])
    need = len(e.done(4000))  # (how many bytes the symbols take: found by closing into a roomy packet and trimming below)
    e_rng = e.rng
    tight = None
    for nbytes in range(1, 4000):
        try:
            tight = e.done(nbytes)
            break
        except rc_craft.CraftError:
            continue
    noise = [r.randrange(256) for _ in range(97)]
    for pkt in (tight, e.done(len(tight) + 1, noise), e.done(len(tight) + 50, noise), e.done(need)):
        rc = RC()
        lib.oc_rc_init(C.byref(rc), pkt, len(pkt))
        for s in syms:
            if s[0] == "encode":
                got = lib.oc_rc_decode(C.byref(rc), s[3])
                assert s[1] <= got < s[2], s
                lib.oc_rc_update(C.byref(rc), s[1], s[2], s[3])
            elif s[0] == "bit":
                assert lib.oc_rc_bit_logp(C.byref(rc), s[2]) == s[1], s
            elif s[0] == "icdf":
                assert lib.oc_rc_icdf(C.byref(rc), bytes(s[2]), s[3]) == s[1], s
            elif s[0] == "uint":
                assert lib.oc_rc_uint(C.byref(rc), s[2]) == s[1], s
            elif s[0] == "bits":
                assert lib.oc_rc_bits(C.byref(rc), s[2]) == s[1], s
            else:
                assert lib.oc_rc_laplace(C.byref(rc), s[2], s[3]) == s[1], s
        assert rc.rng == e_rng and rc.error == 0
        assert rc.nbits_total == e.nbits_total  # the same bit position, so oc_rc_tell agrees with Encoder.tell


def test_done_returns_exactly_nbytes_and_refuses_what_does_not_fit():
    e = rc_craft.Encoder()
    for _ in range(10):
        e.uint(1234, 70000)
    for n in (40, 41, 1275):
        assert len(e.done(n, [1, 2, 3])) == n
    with pytest.raises(rc_craft.CraftError):
        e.done(5)
    assert e.done(60, [0xAB])[30] == 0xAB  # the gap carries the caller's bytes


# ---- the frame writers: what they pin comes back through the oracle's taps -------------------------------------------------------------
def _celt_taps(oracle, channels, packet):
    import numpy as np
    d = oracle.decoder(channels)
    d.init()
    oracle.lib.oc_taps_enable.argtypes = [C.c_void_p]
    oracle.lib.oc_taps_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert oracle.lib.oc_taps_enable(d.h)
    _, r = d.decode(packet)
    assert r == 960
    h, e = np.zeros(75, dtype=np.int32), np.zeros(42, dtype=np.int16)
    assert oracle.lib.oc_taps_copy(d.h, 4, 0, h.ctypes.data) == h.nbytes and oracle.lib.oc_taps_copy(d.h, 1, 0, e.ctypes.data) == e.nbytes
    return h, e


def _coarse_on_fresh_state(coarse, beta):
    """oracle/oc_celt.c coarse_energy on a fresh decoder (old energies 0, so the inter-frame term vanishes) -> per channel per band"""
    out = []
    for c in range(2):
        prev, row = 0, []
        for q in coarse:
            q = q[c] << 10
            row.append((prev + (q << 7) + 64) >> 7)
            prev += (q << 7) - beta * ((q + 128) >> 8)
        out.append(row)
    return out


@pytest.mark.parametrize("intra", [1, 0])
def test_celt_frame_pins_what_it_says(oracle, intra):
    coarse = [[2, 2]] * 14 + [[1, 1]] * 7  # (a sum of 34 before the last band: energies stay inside 16 bits)
    noise = [(37 * i + 11) & 0xFF for i in range(300)]
    pkt = b"\xfc" + rc_craft.celt_frame(120, 2, postfilter=(3, 37, 5, 2), transient=1, intra=intra, coarse=coarse, fill=noise)
    assert len(pkt) == 121 and len(coarse) == 21
    h, e = _celt_taps(oracle, 2, pkt)
    assert (h[0], h[1]) == (1, 0)                                  # transient, no silence
    assert (h[7], h[8], h[9]) == ((16 << 3) + 37 - 1, 3072 * 6, 2)  # post-filter period, gain, tapset
    # band energies: the coarse values plus fine energy (|offset| <= 512) and one final bit (|offset| <= 256): within 768 of the
    # prediction with this frame's intra flag -- and, the two predictors drifting apart by (6554 - 4915) * 4 q / 128 per band, more
    # than 2 * 768 apart by the last band, so not within it for the other flag there
    want = _coarse_on_fresh_state(coarse, 4915 if intra else 6554)
    other = _coarse_on_fresh_state(coarse, 6554 if intra else 4915)
    for c in range(2):
        for i in range(len(coarse)):
            assert abs(int(e[c * 21 + i]) - want[c][i]) <= 768, (c, i, int(e[c * 21 + i]), want[c][i])
        assert abs(want[c][20] - other[c][20]) > 2 * 768 and abs(int(e[c * 21 + 20]) - other[c][20]) > 768
    # the silence flag, and a frame without post-filter
    h, _ = _celt_taps(oracle, 2, b"\xfc" + rc_craft.celt_frame(20, 2, silence=1, fill=noise))
    assert h[1] == 1
    h, _ = _celt_taps(oracle, 1, b"\xf8" + rc_craft.celt_frame(50, 1, transient=0, intra=1, coarse=[1, -1, 2], fill=noise))
    assert (h[0], h[1], h[7], h[8]) == (0, 0, 0, 0)


@pytest.mark.parametrize("LM", [0, 1, 2])
def test_celt_frame_of_a_shorter_duration_pins_what_it_says_in_rfc_mode(oracle, LM):
    """celt_frame(LM=...) writes the 2.5 / 5 / 10 ms frames RFC mode decodes at their own duration (tests/golden/make_kernel_paths.py): the
    frame comes back with that LM, the pinned flags and post-filter, and the coarse energies of LM's own probability model"""
    import numpy as np
    coarse = [[2, 2]] * 14 + [[1, 1]] * 7
    noise = [(53 * i + 7) & 0xFF for i in range(300)]
    transient = 1 if LM else 0
    body = rc_craft.celt_frame(120, 2, postfilter=(2, 21, 4, 1), transient=transient, intra=1, coarse=coarse, fill=noise, LM=LM)
    d = oracle.decoder(2)
    d.init()
    d.set_rfc(True)
    oracle.lib.oc_taps_enable.argtypes = [C.c_void_p]
    oracle.lib.oc_taps_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert oracle.lib.oc_taps_enable(d.h)
    _, r = d.decode(bytes([0xE4 | LM << 3]) + body)  # CELT fullband, stereo, 2.5 << LM ms
    assert r == 120 << LM
    h, e = np.zeros(75, dtype=np.int32), np.zeros(42, dtype=np.int16)
    assert oracle.lib.oc_taps_copy(d.h, 4, 0, h.ctypes.data) == h.nbytes and oracle.lib.oc_taps_copy(d.h, 1, 0, e.ctypes.data) == e.nbytes
    assert (h[0], h[1], h[6]) == (transient, 0, LM)
    assert (h[7], h[8], h[9]) == ((16 << 2) + 21 - 1, 3072 * 5, 1)
    want = _coarse_on_fresh_state(coarse, 4915)  # (intra: the predictor does not depend on LM, the Laplace model does)
    for c in range(2):
        for i in range(21):
            assert abs(int(e[c * 21 + i]) - want[c][i]) <= 768, (LM, c, i, int(e[c * 21 + i]), want[c][i])
    if LM == 0:
        with pytest.raises(rc_craft.CraftError):  # a 2.5 ms frame has no transient flag
            rc_craft.celt_frame(120, 2, transient=1, LM=0)


@pytest.mark.parametrize("fs, toc, stereo", [(8, 0x08, 0), (16, 0x48, 0), (12, 0x2C, 1)])
def test_silk_frame_pins_what_it_says(oracle, fs, toc, stereo):
    import numpy as np
    from test_rare_paths import py_log2lin
    order = 16 if fs == 16 else 10
    ch = {"vad": 1, "type": 4, "gains": [37, 6, 2, 4], "nlsf1": 9, "nlsf_res": [(-1) ** i * (i % 3) for i in range(order)], "interp": 4,
          "lag": (10, 2), "contour": 0, "per": 1, "ltp": [3, 0, 7, 15], "ltp_scale": 2, "seed": 1}
    noise = [(91 * i + 5) & 0xFF for i in range(300)]
    if stereo:
        body = rc_craft.silk_frame(80, 2, fs, chans=[ch, {"vad": 0}], stereo_pred=(7, [1, 2], [2, 4]), mid_only=1,
                                   pulses={"rate_level": 3, "blocks": [[5], [17, 17, 2]]}, fill=noise)
    else:
        body = rc_craft.silk_frame(80, 1, fs, chans=[ch], pulses={"rate_level": 3, "blocks": [[5], [17, 17, 2]]}, fill=noise)
    lib = oracle.lib
    lib.oc_silk_taps_copy.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.oc_silk_taps_enable.argtypes = [C.c_int]
    d = oracle.decoder(2 if stereo else 1)
    d.init()
    lib.oc_silk_taps_enable(1)
    try:
        _, r = d.decode(bytes([toc]) + body)
        assert r == 960

        def tap(what, chn, dtype, n):
            b = np.zeros(n, dtype=dtype)
            assert lib.oc_silk_taps_copy(what, chn, b.ctypes.data) >= 0
            return b
        sb = tap(0, 0, np.int32, 6)
        assert sb[0] == 1 and (sb[1], sb[2]) == (2, 0) and sb[3] == 20 * fs and sb[4] == order
        assert sb[5] == rc_craft.rom("rom_silk_ltp_scales_q14")[2]
        if stereo:
            assert tap(0, 1, np.int32, 6)[0] == 0  # the side channel is absent
        b = tap(1, 0, np.int32, 8)
        # gains: index 37 (above LastGainIndex 10 - 16), then deltas 6, 2, 4 -> +2, -2, 0 (src/silk.cpp:2148-2172)
        assert list(b[4:]) == [py_log2lin(((1907825 * g) >> 16) + 2090) for g in (37, 39, 37, 37)]
        # pitch: lag index 10 * (fs / 2) + 2 above the minimum lag 2 fs, contour 0 (src/silk.cpp:2055-2080)
        cbk, size = (rc_craft.rom("rom_silk_lags_stage2"), 11) if fs == 8 else (rc_craft.rom("rom_silk_lags_stage3"), 34)
        lag = 2 * fs + 10 * (fs >> 1) + 2
        assert list(b[:4]) == [min(max(lag + cbk[k * size], 2 * fs), 18 * fs) for k in range(4)]
        vq = rc_craft.rom("rom_silk_ltp_vq1")
        assert list(tap(3, 0, np.int16, 20)) == [vq[ix * 5 + i] << 7 for ix in (3, 0, 7, 15) for i in range(5)]
    finally:
        lib.oc_silk_taps_enable(0)
