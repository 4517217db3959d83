"""The parse kernel's allocation scratch in host emulation (the one-frame-per-lane parse, LaneArr in og_celt_parse.hpp, through
tests/emul/og_emul_tight.cpp) against the oracle, bit for bit.  A band's dynalloc boost rests as a COUNT in the band's fine_quant
byte from celt_parse_header's boost loop until compute_allocation has read it for the last time; the i16 array it had took a
quarter of a 64-frame parse wave's LDS.  Stereo payloads of 20 / 40 / 80 / 160 / 400 bytes, 64 streams x 8 frames
each (tests/parse_alloc_batches.py), through a stand-alone program built with ASan + UBSan (tests/emul/og_parse_alloc_main.cpp:
nothing sanitized is loaded into python), which also counts what the batches reach.  None of these classes may be empty: frames
with a boost, bands boosted three times or more, a boost stopped by its cap, frames whose budget went negative.

The oracle has no counters.  What it says about the census on its own, before the emulation is asked: the silent frames decode to
digital silence, and the directed payload decodes; the counts themselves are the emulation's, which equals the oracle in every sample."""
import functools
import os
import subprocess

import numpy as np

from parse_alloc_batches import ROOT, SIZES, reference

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
STREAMS, FRAMES = 64, 8
COUNTERS = ("frames", "frames_boosted", "bands_boosted_3up", "boosts_at_cap", "frames_negative_budget")


def test_the_oracle_alone_sees_the_directed_frames():
    for L in SIZES:
        pay, ref = reference(L, STREAMS, FRAMES)
        assert (pay[2:4, STREAMS - 2, :4] == 0xFF).all()
        # a silent CELT frame leaves only what the frame before left in the overlap and the de-emphasis: it dies away
        assert np.abs(ref[STREAMS - 2, 3, 480:].astype(np.int32)).max() <= np.abs(ref[STREAMS - 2, 1].astype(np.int32)).max()
        assert np.abs(ref[STREAMS - 2, 3, 900:].astype(np.int32)).max() < 64, L
    pay, ref = reference(160, STREAMS, FRAMES)
    assert (pay[0, STREAMS - 1] == pay[FRAMES - 1, STREAMS - 1]).all() and ref[STREAMS - 1, 0].any()


@functools.lru_cache(maxsize=None)
def _counters(tmp):
    """The sizes through the sanitized program: -> {L: counters}; the PCM is compared here."""
    exe = os.path.join(tmp, "og_parse_alloc_main")
    flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wno-pedantic", "-Wno-attributes", *flags, "-I", CSRC,
                           os.path.join(EMUL_DIR, "og_parse_alloc_main.cpp"), "-o", exe])
    got = {}
    for L in SIZES:
        pay, ref = reference(L, STREAMS, FRAMES)
        fin, fout = os.path.join(tmp, f"in{L}.bin"), os.path.join(tmp, f"out{L}.bin")
        with open(fin, "wb") as f:
            f.write(np.array([STREAMS, FRAMES, L, 2, 2], dtype=np.int32).tobytes())
            f.write(pay.tobytes())
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert p.returncode == 0, (L, p.returncode, p.stderr[-2000:])
        got[L] = dict(zip(COUNTERS, (int(x) for x in p.stdout.split())))
        pcm = np.fromfile(fout, dtype=np.int16).reshape(ref.shape)
        bad = (pcm != ref).any(axis=(2, 3))
        assert not bad.any(), (L, "PCM of (stream, frame)", np.argwhere(bad)[:8].tolist())
    return got


def test_program_under_sanitizers_matches_the_oracle_and_reaches_every_class(tmp_path_factory):
    got = _counters(str(tmp_path_factory.mktemp("parse_alloc")))
    total = {k: sum(got[L][k] for L in SIZES) for k in COUNTERS}
    for L in SIZES:
        print(L, got[L])
    print("all", total)
    for L in SIZES:
        assert got[L]["frames"] == STREAMS * FRAMES
        assert got[L]["frames_negative_budget"] >= 2  # the two silent frames of every batch
    assert got[160]["boosts_at_cap"] >= 2             # the directed payload, twice
    assert all(total[k] > 0 for k in COUNTERS), total
