"""The comb filter's steps in k_celt_recon_fb (og_comb_step.hpp: gains in scalar registers, dead lanes that compute with what they
read, one lane address per window, the cross-fade's window word through a lane offset) on the GPU against the oracle, on DIRECTED
frames.  Stereo decoder, 64 streams x 12 frames of stereo packets crafted by rc_craft.celt_frame(160, 2, postfilter=(octave, low,
qg, tapset), transient=..., fill=LCG bytes):

* the lag of (stream s, frame f) is LAGS[(5 f + s) mod 24]: 15, 16, 17, 32 .. 34, 65 .. 67, 118 .. 122, 300, 511 .. 513, 1020 ..
  1022 and 64 -- around the minimum, half a step, the 64-sample step, the second call's first sample, the middle and the longest;
* every fourth frame has the post-filter off (cross-fade-only calls and off -> on calls follow from it), tapsets 0 / 1 / 2, gain
  indices 0 and 7, one frame in six transient.

The oracle must decode each packet to 960 samples and report the crafted lag in its header tap.  The classes of steps the frames
reach are counted on the CPU (no GPU) by replaying the filter's step rule (comb_call, comb_step_len, comb_win_class) with the
oracle's taps and the frame index, and an empty class fails: a step's 68-sample window wholly in the synthesis buffer, wholly in
the ring without wrap, or across (ring and buffer, or the ring's end) -- each of the three in and past the cross-fade.  On the GPU
the batch runs step by step and as ONE queued window; EVERY step's PCM and result codes are compared.  The bar is equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import rc_craft
from test_gpu_pipeline import run_queued

N_STREAMS, FRAMES, TOC, SEED = 64, 12, 0xFC, 0xC0B05700
LAGS = [15, 16, 17, 32, 33, 34, 65, 66, 67, 118, 119, 120, 121, 122, 300, 511, 512, 513, 1020, 1021, 1022, 64, 123, 700]
CLASSES = tuple(w + "_" + p for p in ("in_fade", "past_fade") for w in ("buffer", "ring", "across"))
RING, OVERLAP = 2048, 120


def _pkg():
    from conftest import load_pkg
    return load_pkg()


def _frame_params(s, f):
    """-> (lag or None, qg, tapset, transient) of stream s, frame f"""
    lag = None if f % 4 == 3 else LAGS[(5 * f + s) % len(LAGS)]
    return lag, (0 if (s + f) % 2 else 7), (s + f) % 3, int((f + s) % 6 == 0)


def _count_call(count, pos, off, N, T0, T1, g0, g1, tap0, tap1):
    """comb_filter's step rule (og_comb_step.hpp), windows classified"""
    if g0 == 0 and g1 == 0:
        return
    T0, T1 = max(T0, 15), max(T1, 15)
    overlap = 0 if (g0 == g1 and T0 == T1 and tap0 == tap1) else OVERLAP
    use0, use1 = g0 != 0, g1 != 0
    chunk_fade = min(T0 if use0 else 1 << 20, T1 if use1 else 1 << 20) - 2
    end = overlap if g1 == 0 else N
    base = 0
    while base < end:
        fade = base < overlap
        lim = min(chunk_fade if fade else T1 - 2, 64, end - base)
        for T, used in ((T1, use1), (T0, use0 and fade)):
            if not used:
                continue
            first = off + base - T - 2
            if first >= 0:
                w = "buffer"
            elif first + 67 < 0 and (pos + first) % RING + 67 <= RING - 1:
                w = "ring"
            else:
                w = "across"
            count[w + ("_in_fade" if fade else "_past_fade")] += 1
        base += lim


@functools.lru_cache(maxsize=None)
def _reference():
    """-> packets[frame][stream], oracle PCM [frames, n, 1920], class counts.  Computed once, read-only."""
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    n = N_STREAMS
    fill = pkg.lcg_payloads(n, FRAMES, 160, seed_base=SEED)
    pk = [[None] * n for _ in range(FRAMES)]
    pcm = np.zeros((FRAMES, n, 960 * 2), dtype=np.int16)
    count = dict.fromkeys(CLASSES, 0)
    oracle.lib.oc_taps_enable.argtypes = [C.c_void_p]
    oracle.lib.oc_taps_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    d = oracle.decoder(2)
    hdr = np.zeros(75, dtype=np.int32)
    for s in range(n):
        d.init()
        assert oracle.lib.oc_taps_enable(d.h)
        Tp, gp, tapp = 0, 0, 0  # the post-filter the frame before left (period == period_old after a 20 ms frame)
        for f in range(FRAMES):
            lag, qg, tapset, transient = _frame_params(s, f)
            pf = None
            if lag is not None:
                octave = (lag + 1).bit_length() - 5
                pf = (octave, lag + 1 - (16 << octave), qg, tapset)
            pk[f][s] = bytes([TOC]) + rc_craft.celt_frame(160, 2, postfilter=pf, transient=transient, fill=fill[f, s])
            ref, r = d.decode(pk[f][s])
            assert r == 960, (s, f, r)
            pcm[f, s] = ref[:960].reshape(-1)
            assert oracle.lib.oc_taps_copy(d.h, 4, 0, hdr.ctypes.data) == hdr.nbytes
            T, g = int(hdr[7]), int(hdr[8])
            assert int(hdr[0]) == transient, (s, f)
            assert (g != 0) == (lag is not None) and (lag is None or (T == lag and g == 3072 * (qg + 1))), (s, f, lag, T, g)
            now = (T, g, tapset if lag is not None else 0)
            pos = (960 * f) % RING
            for _ in range(2):  # both channels run the same two calls
                _count_call(count, pos, 0, 120, Tp, Tp, gp, gp, tapp, tapp)
                _count_call(count, pos, 120, 840, Tp, now[0], gp, now[1], tapp, now[2])
            Tp, gp, tapp = now
    pcm.setflags(write=False)
    return pk, pcm, count


def test_every_class_of_step_occurs():
    """(no GPU) every lag crafts, decodes to 960 samples and comes back in the oracle's header tap; no class of step is empty"""
    count = _reference()[2]
    print(count)
    empty = [c for c in CLASSES if count[c] == 0]
    assert not empty, (empty, count)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
def test_every_step_matches_the_oracle(pkg, gpu_ctx, route):
    n = N_STREAMS
    pk, ref, _ = _reference()
    lens = np.full((FRAMES, n), 161, dtype=np.int64)
    offs = (np.arange(FRAMES * n, dtype=np.int64) * 161).reshape(FRAMES, n)
    arena = np.frombuffer(b"".join(p for row in pk for p in row) + bytes(16), dtype=np.uint8).copy()
    tocs = np.full((FRAMES, n), TOC, dtype=np.uint8)
    if route == "in_order":
        pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens - 1, tocs, pipeline=False)
    else:
        pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens - 1, tocs, pipeline=True, window=True, modes=pkg.toc_modes(TOC))
    assert (res == 960).all(), (route, "result codes of (frame, stream)", np.argwhere(res != 960)[:4].tolist())
    bad = (pcm != ref).any(axis=-1)
    assert not bad.any(), (route, "PCM of (frame, stream)", np.argwhere(bad)[:8].tolist(), "frames that differ per step",
                           bad.sum(axis=1).tolist())
