"""The synthesis half of k_celt_recon_fb -- inverse MDCT (long block: imdct_long_front, the lane-by-lane radix-3 and radix-5
stages, imdct_long_back; short blocks and down-mixes: the generic stages) and the pitch comb filter -- whose table words are
requested a stage ahead of their use (og_celt.hpp).  Batches of CELT fullband frames of LCG payloads against the oracle:

* 256 stereo streams x 6 frames in a stereo decoder: 1,536 frames, the smallest batch in which the rare classes below turn up;
* 64 streams each of: mono packets in a mono decoder, stereo packets in a mono decoder (the down-mix: two spectra per coefficient,
  generic code), mono packets in a stereo decoder (one transform, two output planes).

Each batch runs step by step and as ONE pipelined window; EVERY step's PCM and result codes are compared, not only the last
step's.  Which paths the frames take is counted on the CPU from the oracle's header taps (tests need data, not luck): long
blocks, transient frames (eight short blocks), and by the comb filter's call on a frame's last 840 samples -- gains g0 = the
previous frame's, g1 = this frame's, lags T0, T1 likewise (celt_decode_with_ec celt.cpp:2459) -- post-filter off (g0 = g1 = 0),
on (g1 != 0), cross-fade only (g1 = 0, g0 != 0) and a lag below 64 with a gain that counts (a step of fewer than 64 samples).
An empty class fails the test; that check needs no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_pipeline import run_queued

FRAMES, L = 6, 160
TOC_STEREO, TOC_MONO = 0xFC, 0xF8
# name -> (streams, decoder channels, TOC)
BATCHES = {
    "stereo": (256, 2, TOC_STEREO),
    "mono": (64, 1, TOC_MONO),
    "downmix": (64, 1, TOC_STEREO),
    "mono_in_stereo": (64, 2, TOC_MONO),
}
CLASSES = ("long", "transient", "pf_off", "pf_on", "crossfade_only", "lag_below_64")


def _pkg():
    from conftest import load_pkg
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """-> packets[frame][stream], oracle PCM [frames, n, 960 * ch], return codes [frames, n], class counts.  Computed once."""
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    n, channels, toc = BATCHES[name]
    pay = pkg.lcg_payloads(n, FRAMES, L, seed_base=0x5EED0000 + 0x100 * list(BATCHES).index(name))  # (a payload set of its own per batch)
    pk = [[bytes([toc]) + pay[f, s].tobytes() for s in range(n)] for f in range(FRAMES)]
    pcm = np.zeros((FRAMES, n, 960 * channels), dtype=np.int16)
    rets = np.zeros((FRAMES, n), dtype=np.int32)
    count = dict.fromkeys(CLASSES, 0)
    oracle.lib.oc_taps_enable.argtypes = [C.c_void_p]
    oracle.lib.oc_taps_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    d = oracle.decoder(channels)
    hdr = np.zeros(75, dtype=np.int32)
    for s in range(n):
        d.init()
        assert oracle.lib.oc_taps_enable(d.h)
        g0, t0 = 0, 0  # the post-filter the previous frame left
        for f in range(FRAMES):
            ref, r = d.decode(pk[f][s])
            rets[f, s] = r
            assert r == 960, (name, f, s, r)
            pcm[f, s] = ref[:960].reshape(-1)
            assert oracle.lib.oc_taps_copy(d.h, 4, 0, hdr.ctypes.data) == hdr.nbytes
            transient, g1, t1 = int(hdr[0]), int(hdr[8]), int(hdr[7])
            count["transient" if transient else "long"] += 1
            count["pf_off"] += g0 == 0 and g1 == 0
            count["pf_on"] += g1 != 0
            count["crossfade_only"] += g1 == 0 and g0 != 0
            count["lag_below_64"] += (g1 != 0 and max(t1, 15) < 64) or (g0 != 0 and max(t0, 15) < 64)
            g0, t0 = g1, t1
    pcm.setflags(write=False)
    rets.setflags(write=False)
    return pk, pcm, rets, count


def test_every_synthesis_class_occurs():
    """(no GPU) the 1,536 stereo frames hold every class; so does every small batch for the two block sizes."""
    count = _reference("stereo")[3]
    print(count)
    assert count["long"] + count["transient"] == 256 * FRAMES
    empty = [c for c in CLASSES if count[c] == 0]
    assert not empty, (empty, count)
    for name in ("mono", "downmix", "mono_in_stereo"):
        c = _reference(name)[3]
        print(name, c)
        assert c["long"] and c["transient"] and c["pf_on"] and c["pf_off"], (name, c)


def _arena(pk, n):
    lens = np.array([[len(p) for p in row] for row in pk], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens.reshape(-1))[:-1]]).reshape(len(pk), n)
    arena = np.frombuffer(b"".join(p for row in pk for p in row) + bytes(16), dtype=np.uint8).copy()
    return arena, offs, lens


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_every_step_matches_the_oracle(pkg, gpu_ctx, name, route):
    n, channels, toc = BATCHES[name]
    pk, ref, rets, _ = _reference(name)
    arena, offs, lens = _arena(pk, n)
    tocs = np.full((FRAMES, n), toc, dtype=np.uint8)
    if route == "in_order":
        pcm, res = run_queued(pkg, gpu_ctx, channels, arena, offs, lens - 1, tocs, pipeline=False)
    else:
        pcm, res = run_queued(pkg, gpu_ctx, channels, arena, offs, lens - 1, tocs, pipeline=True, window=True, modes=pkg.toc_modes(toc))
    assert (res == rets).all(), (name, route, "result codes of (frame, stream)", np.argwhere(res != rets)[:4].tolist())
    bad = (pcm != ref).any(axis=-1)
    assert not bad.any(), (name, route, "PCM of (frame, stream)", np.argwhere(bad)[:8].tolist(), "frames that differ per step",
                           bad.sum(axis=1).tolist())
