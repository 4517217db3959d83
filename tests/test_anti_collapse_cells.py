"""Anti-collapse of the reconstruction kernel of 20 ms frames (anti_collapse_pm, og_celt_recon_pm.hpp): the collapsed (band,
channel, block) cells of a transient frame are filled in whole-wave passes -- seeds by a prefix over the (band, channel) entries,
a lane per group of 8 coefficients, one gain per entry that had a fill.  The kernel's source in host emulation (the emulated
tight layout, tests/emul/og_emul_tight.cpp) against the oracle, bit for bit, on batches whose classes are counted first from the
oracle's header taps (tests need data, not luck):

* stereo: lcg_payloads(256, 12, 160), the bench's payloads -- 3,072 frames, at least 300 transient, at least 150 with anti-collapse;
* 64 streams x 12 frames each of mono packets in a mono decoder (C = 1), mono packets in a stereo decoder, and hybrid fullband
  packets (the CELT layer starts at band 17).

The emulated tight layout takes CELT-only frames; the hybrid batch goes through the emulation of the general layout here (the
band-by-band anti-collapse), and through the 20 ms kernel itself in tests/test_gpu_transient_frames.py, which shares these batches.

The same code runs once more as a program of its own under AddressSanitizer and UBSan (tests/emul/og_anti_collapse_main.cpp);
that run also counts the cells filled and the (band, channel) entries renormalised."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
FRAMES = 12
# name -> (streams, decoder channels, TOC, payload bytes, LCG seed base; None: the bench's)
BATCHES = {
    "stereo": (256, 2, 0xFC, 160, None),
    "mono": (64, 1, 0xF8, 160, 0xAC011A00),
    "mono_in_stereo": (64, 2, 0xF8, 160, 0xAC011B00),
    "hybrid": (64, 2, 0x7C, 120, 0xAC011C00),
}
CELT_ONLY = ("stereo", "mono", "mono_in_stereo")


def _pkg():
    from conftest import load_pkg
    return load_pkg()


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> payloads uint8 [frames, n, L], oracle PCM int16 [n, frames, 960, ch], class counts.  Computed once, read-only."""
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    n, channels, toc, L, seed = BATCHES[name]
    pay = pkg.lcg_payloads(n, FRAMES, L) if seed is None else pkg.lcg_payloads(n, FRAMES, L, seed_base=seed)
    pcm = np.zeros((n, FRAMES, 960, channels), dtype=np.int16)
    count = {"frames": 0, "transient": 0, "anti_collapse": 0}
    oracle.lib.oc_taps_enable.argtypes = [C.c_void_p]
    oracle.lib.oc_taps_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    d = oracle.decoder(channels)
    hdr = np.zeros(75, dtype=np.int32)
    for s in range(n):
        d.init()
        assert oracle.lib.oc_taps_enable(d.h)
        for f in range(FRAMES):
            ref, r = d.decode(bytes([toc]) + pay[f, s].tobytes())
            assert r == 960, (name, s, f, r)
            pcm[s, f] = ref[:960]
            assert oracle.lib.oc_taps_copy(d.h, 4, 0, hdr.ctypes.data) == hdr.nbytes
            assert hdr[6] == 3, (name, s, f, "LM")  # 20 ms
            count["frames"] += 1
            count["transient"] += int(hdr[0] != 0)
            count["anti_collapse"] += int(hdr[10] != 0)
    pay.setflags(write=False)
    pcm.setflags(write=False)
    return pay, pcm, count


def test_every_class_occurs():
    count = reference("stereo")[2]
    print("stereo", count)
    assert count["frames"] == 256 * FRAMES
    assert count["transient"] >= 300 and count["anti_collapse"] >= 150, count
    for name in ("mono", "mono_in_stereo", "hybrid"):
        c = reference(name)[2]
        print(name, c)
        # (the oracle reaches every class with these payloads: long blocks, transient frames without and with anti-collapse)
        assert c["frames"] > c["transient"] > c["anti_collapse"] > 0, (name, c)


def _emu(lib):
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", lib])
    emu = C.CDLL(os.path.join(EMUL_DIR, lib))
    emu.emu_state_size.restype = C.c_int
    emu.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
    emu.emu_decode_frame.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return emu


@pytest.mark.parametrize("name", list(BATCHES))
def test_emulated_kernel_matches_the_oracle(name):
    n, channels, toc, L, _ = BATCHES[name]
    pay, ref, _ = reference(name)
    emu = _emu("libog_emul_tight.so" if name in CELT_ONLY else "libog_emul.so")
    mode = 1002 if toc & 0x80 else 1001
    st = C.create_string_buffer(emu.emu_state_size())
    out = np.zeros((960, channels), dtype=np.int16)
    for s in range(n):
        emu.emu_stream_init(st, channels)
        for f in range(FRAMES):
            out[:] = 0
            r = emu.emu_decode_frame(st, pay[f, s].tobytes(), L, mode, 1105, 2 if toc & 4 else 1, out.ctypes.data)
            assert r == 960, (name, s, f, r)
            assert np.array_equal(out, ref[s, f]), f"{name}: stream {s}, frame {f}: emulated PCM differs from the oracle"


@functools.lru_cache(maxsize=None)
def _sanitized_program(tmp):
    exe = os.path.join(tmp, "og_anti_collapse_main")
    flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wno-pedantic", "-Wno-attributes", *flags, "-I", CSRC,
                           os.path.join(EMUL_DIR, "og_anti_collapse_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", CELT_ONLY)
def test_program_under_sanitizers_matches_the_oracle(name, tmp_path_factory):
    """The emulated tight layout as a program of its own under ASan + UBSan: clean, bit-exact, and its event counters agree with
    the oracle's header taps.  Prints the cells filled and the entries renormalised (the reference decoder, counted the same
    way on the stereo batch: 360 transient frames, 179 with anti-collapse, 5,984 cells, 2,647 bands)."""
    n, channels, toc, L, _ = BATCHES[name]
    pay, ref, count = reference(name)
    exe = _sanitized_program(str(tmp_path_factory.getbasetemp()))
    tmp = tmp_path_factory.mktemp(name)
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, FRAMES, L, channels, 2 if toc & 4 else 1], dtype=np.int32).tobytes())
        f.write(pay.tobytes())
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert p.returncode == 0, (name, p.returncode, p.stderr[-2000:])
    frames, transient, ran, cells, bands = (int(x) for x in p.stdout.split())
    print(f"{name}: {frames} frames, {transient} transient, {ran} with anti-collapse, {cells} cells filled, {bands} bands renormalised")
    assert (frames, transient, ran) == (count["frames"], count["transient"], count["anti_collapse"])
    assert cells >= bands > 0
    pcm = np.fromfile(fout, dtype=np.int16).reshape(ref.shape)
    bad = (pcm != ref).any(axis=(2, 3))
    assert not bad.any(), (name, "PCM of (stream, frame)", np.argwhere(bad)[:8].tolist())
