"""The fill jobs of the phase-major band loop (pm_fill_jobs, og_celt_recon_pm.hpp) in host emulation (the emulated tight layout,
tests/emul/og_emul_tight.cpp) against the oracle, bit for bit: stereo CELT fullband packets of 20, 40, 80, 160 and 400 LCG bytes,
64 streams x 8 frames each -- few bytes leave many bands without pulses (many fill jobs), many bytes leave few.  (Up to 160 bytes
every frame has a fill job -- counted: 15.2, 10.2, 6.1, 3.2 per frame; 400 bytes were added for the frames without one: 169 of
its 512.)

What this test is and is not.  It was specified for a change that requested each fill job's word window ahead of the job; that
change was built, measured, lost and is not in the tree.  The fill jobs read their words through rec_word's window
as before, and this test would pass on the code before round 11 but for the counters it reads.  The emulation compiles the
GENERAL forms of what round 11 did change (LcgTab::at_lane falls back to at(), band_w is read from the record, the stereo
merge's band edges at their use): those are held on the GPU by tests/test_gpu_fill_windows.py, which runs these batches.  What
it gives: the batches and their oracle PCM, shared with that test; the kernel source under ASan + UBSan on them
(tests/emul/og_fill_windows_main.cpp); and the counts that make the batches worth running -- frames with no fill job, with one,
with four or more, and with two fill jobs less than a window (64 words) apart must all occur, and the refills of the window are
printed (at 160 bytes about one per frame for 3.2 fill jobs: most jobs start inside the window of the one before, which is why
requesting windows ahead had nothing to win)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
STREAMS, FRAMES, TOC = 64, 8, 0xFC
SIZES = (20, 40, 80, 160, 400)
COUNTERS = ("frames", "fill_jobs", "skipped", "run", "refills", "frames_0", "frames_1", "frames_4up", "frames_close_pair")


def _pkg():
    from conftest import load_pkg
    return load_pkg()


@functools.lru_cache(maxsize=None)
def reference(L):
    """-> payloads uint8 [frames, n, L], oracle PCM int16 [n, frames, 960, 2].  Computed once, read-only."""
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    pay = pkg.lcg_payloads(STREAMS, FRAMES, L, seed_base=0xF111A000 + L)
    pcm = np.zeros((STREAMS, FRAMES, 960, 2), dtype=np.int16)
    d = oracle.decoder(2)
    for s in range(STREAMS):
        d.init()
        for f in range(FRAMES):
            ref, r = d.decode(bytes([TOC]) + pay[f, s].tobytes())
            assert r == 960, (L, s, f, r)
            pcm[s, f] = ref[:960]
    pay.setflags(write=False)
    pcm.setflags(write=False)
    return pay, pcm


@pytest.mark.parametrize("L", SIZES)
def test_emulated_kernel_matches_the_oracle(L):
    pay, ref = reference(L)
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "libog_emul_tight.so"])
    emu = C.CDLL(os.path.join(EMUL_DIR, "libog_emul_tight.so"))
    emu.emu_state_size.restype = C.c_int
    emu.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
    emu.emu_decode_frame.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    st = C.create_string_buffer(emu.emu_state_size())
    out = np.zeros((960, 2), dtype=np.int16)
    for s in range(STREAMS):
        emu.emu_stream_init(st, 2)
        for f in range(FRAMES):
            out[:] = 0
            r = emu.emu_decode_frame(st, pay[f, s].tobytes(), L, 1002, 1105, 2, out.ctypes.data)
            assert r == 960, (L, s, f, r)
            assert np.array_equal(out, ref[s, f]), f"{L} bytes: stream {s}, frame {f}: emulated PCM differs from the oracle"


@functools.lru_cache(maxsize=None)
def _counters(tmp):
    """The sizes through the sanitized program: -> {L: counters}; the PCM is compared here."""
    exe = os.path.join(tmp, "og_fill_windows_main")
    flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wno-pedantic", "-Wno-attributes", *flags, "-I", CSRC,
                           os.path.join(EMUL_DIR, "og_fill_windows_main.cpp"), "-o", exe])
    got = {}
    for L in SIZES:
        pay, ref = reference(L)
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


def test_program_under_sanitizers_and_its_counters(tmp_path_factory):
    got = _counters(str(tmp_path_factory.mktemp("fill_windows")))
    total = {k: sum(got[L][k] for L in SIZES) for k in COUNTERS}
    for L in SIZES:
        print(L, got[L])
    print("all", total)
    for L in SIZES:
        c = got[L]
        assert c["frames"] == STREAMS * FRAMES
        assert c["fill_jobs"] == c["skipped"] + c["run"]
        assert 0 < c["refills"] <= c["run"] or c["run"] == 0, c  # (the first job of a frame refills; most others do not)
    # every class occurs, over the sizes together
    assert total["frames_0"] > 0 and total["frames_1"] > 0 and total["frames_4up"] > 0 and total["frames_close_pair"] > 0, total
    assert total["refills"] < total["run"], total
