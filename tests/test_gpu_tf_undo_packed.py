"""The packed-word forms of k_celt_recon_fb (og_celt_packed.hpp: interleave gather by rows, Haar steps and stereo merge on packed words,
ring and tail writes in 16-byte pieces) on the GPU, against the oracle, bit for bit:

* 256 stereo streams x 6 frames of LCG payloads at 40, 160 and 400 bytes;
* 64 streams of mono packets in a stereo decoder;
* 32 hybrid fullband streams x 24 frames of 200 bytes, whose CELT layer starts at band 17 (four bands a frame: the longer run is what
  gives every class its bands);
* 64 streams of crafted transient frames (rc_craft.celt_frame, the transient flag pinned, LCG bytes behind it).

Each set runs step by step and as ONE queued window; EVERY step's PCM and result codes are compared.  Six frames move the ring head
over 5,760 samples: the ring write wraps twice per stream at least.

What the sets exercise is counted on the CPU first (test_every_class_occurs, no GPU): the class of every coded band of every frame --
(interleave stride, Hadamard ordering, Haar steps), derived in tests/test_tf_undo_packed.py from the oracle's tf table -- from the
oracle's taps (transient flag, tf_res, first and last band).  No class that a set can have may be missing from it: a set of long
blocks and transient frames has all six, the crafted set the four of transient frames.  (A band counted here whose job has a leaf
without pulses is undone by the fill jobs instead of the whole-wave passes -- about 3 of a frame's 42 jobs on these payloads --
so the bar per class is 24 bands, not one.)"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_tf_undo_packed import NO_CHANGE, band_widths, classes, job_class

# name -> (streams, decoder channels, TOC, payload bytes, LCG seed base; None: the bench's, frames)
SETS = {
    "stereo_40": (256, 2, 0xFC, 40, None, 6),
    "stereo_160": (256, 2, 0xFC, 160, None, 6),
    "stereo_400": (256, 2, 0xFC, 400, None, 6),
    "mono_in_stereo": (64, 2, 0xF8, 160, 0x7F0D1A00, 6),
    "hybrid": (32, 2, 0x7C, 200, 0x7F0D1B00, 24),
    "crafted_transient": (64, 2, 0xFC, 160, 0x7F0D1C00, 6),
}
MIN_BANDS = 24


def _payloads(name):
    from conftest import load_pkg
    pkg = load_pkg()
    n, _, toc, L, seed, FRAMES = SETS[name]
    pay = pkg.lcg_payloads(n, FRAMES, L) if seed is None else pkg.lcg_payloads(n, FRAMES, L, seed_base=seed)
    if name == "crafted_transient":
        import rc_craft
        pay = pay.copy()
        for f in range(FRAMES):
            for s in range(n):
                pay[f, s] = np.frombuffer(rc_craft.celt_frame(L, 2 if toc & 4 else 1, transient=1, fill=pay[f, s]), dtype=np.uint8)
    return pay


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> payloads uint8 [frames, n, L], oracle PCM int16 [frames, n, 960 * ch], {class: bands}, transient frames.  Once, read-only."""
    import oracle_py
    oracle = oracle_py.load()
    n, channels, toc, L, _, FRAMES = SETS[name]
    pay = _payloads(name)
    pcm = np.zeros((FRAMES, n, 960 * channels), dtype=np.int16)
    oracle.lib.oc_taps_enable.argtypes = [C.c_void_p]
    oracle.lib.oc_taps_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    d = oracle.decoder(channels)
    hdr, what = np.zeros(75, dtype=np.int32), np.zeros(8, dtype=np.int32)
    widths = band_widths()
    count, transient = {}, 0
    for s in range(n):
        d.init()
        assert oracle.lib.oc_taps_enable(d.h)
        for f in range(FRAMES):
            ref, r = d.decode(bytes([toc]) + pay[f, s].tobytes())
            assert r == 960, (name, s, f, r)
            pcm[f, s] = ref[:960].reshape(-1)
            assert oracle.lib.oc_taps_copy(d.h, 4, 0, hdr.ctypes.data) == hdr.nbytes
            assert oracle.lib.oc_taps_copy(d.h, 5, 0, what.ctypes.data) == what.nbytes
            assert hdr[6] == 3, (name, s, f, "LM")  # 20 ms
            if hdr[1]:  # silence: no band is decoded
                continue
            transient += int(hdr[0] != 0)
            for i in range(what[0], what[1]):
                c = job_class(int(hdr[54 + i]), widths[i], 8 if hdr[0] else 1)
                if c != NO_CHANGE:
                    count[c] = count.get(c, 0) + 1
    pay.setflags(write=False)
    pcm.setflags(write=False)
    return pay, pcm, count, transient


@pytest.mark.parametrize("name", list(SETS))
def test_every_class_occurs(name):
    _, _, count, transient = reference(name)
    print(name, "transient frames", transient, {str(k): v for k, v in sorted(count.items())})
    every = set(classes())
    want = {c for c in every if not c[1]} if name == "crafted_transient" else every  # (ordered rows: long blocks only)
    assert len(want) == (4 if name == "crafted_transient" else 6)
    assert set(count) <= every
    for c in want:
        assert count.get(c, 0) >= MIN_BANDS, (name, c, count.get(c, 0))
    if name == "crafted_transient":
        assert transient == SETS[name][0] * SETS[name][5]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
@pytest.mark.parametrize("name", list(SETS))
def test_every_step_matches_the_oracle(pkg, gpu_ctx, name, route):
    from test_gpu_pipeline import run_queued
    n, channels, toc, L, _, FRAMES = SETS[name]
    pay, ref, _, _ = reference(name)
    pk = np.empty((FRAMES, n, L + 1), dtype=np.uint8)  # packets back to back, frame-major: TOC byte + payload
    pk[:, :, 0] = toc
    pk[:, :, 1:] = pay
    arena = np.concatenate([pk.reshape(-1), np.zeros(16, dtype=np.uint8)])
    offs = (np.arange(FRAMES * n, dtype=np.int64) * (L + 1)).reshape(FRAMES, n)
    lens = np.full((FRAMES, n), L, dtype=np.int64)
    tocs = np.full((FRAMES, n), toc, dtype=np.uint8)
    if route == "in_order":
        pcm, res = run_queued(pkg, gpu_ctx, channels, arena, offs, lens, tocs, pipeline=False)
    else:
        pcm, res = run_queued(pkg, gpu_ctx, channels, arena, offs, lens, tocs, pipeline=True, window=True, modes=pkg.toc_modes(toc))
    assert (res == 960).all(), (name, route, "result codes of (frame, stream)", np.argwhere(res != 960)[:4].tolist())
    bad = (pcm != ref).any(axis=-1)
    assert not bad.any(), (name, route, "PCM of (frame, stream)", np.argwhere(bad)[:8].tolist(), "frames that differ per step",
                           bad.sum(axis=1).tolist())
