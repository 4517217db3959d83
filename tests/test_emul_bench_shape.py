"""The headline workload of bench.py on the CPU: TOC 0xFC (CELT-only, fullband, 20 ms, stereo), 160-byte LCG payloads, 2,048 streams
x 8 frames, through the emulated parse (celt_parse_lane) and reconstruction, every PCM sample against the oracle's batch decode.
The parse kernel is tuned on exactly these payloads; this runs its source over them before a GPU does."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul", "libog_emul.so")


def test_bench_shape_celt_fb_stereo_matches_oracle(pkg, oracle):
    subprocess.check_call(["make", "-C", os.path.dirname(EMUL), "-s"])
    emu = C.CDLL(EMUL)
    emu.emu_state_size.restype = C.c_int
    emu.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
    emu.emu_decode_frame.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    toc, n, frames, L = 0xFC, 2048, 8, 160
    assert toc == pkg.TOC_CELT_FB_STEREO
    pay = pkg.lcg_payloads(n, frames, L)
    ref, ok = oracle.batch_decode_threads(2, toc, pay)
    assert ok == n * frames
    st = C.create_string_buffer(emu.emu_state_size())
    out = np.zeros((960, 2), dtype=np.int16)
    for s in range(n):
        emu.emu_stream_init(st, 2)
        for f in range(frames):
            out[:] = 0
            r = emu.emu_decode_frame(st, pay[f, s].tobytes(), L, 1002, 1105, 2, out.ctypes.data)
            assert r == 960, (s, f, r)
            assert np.array_equal(out, ref[s, f]), f"stream {s}, frame {f}: emulated PCM differs from the oracle"
