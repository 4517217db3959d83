"""The pitch comb filter's history taps in k_celt_recon_fb (comb_filter, og_celt.hpp; the history lines are touched ahead of the
filter by imdct_channel: comb_touch_plan) on the GPU against the oracle, on DIRECTED frames: random payloads draw their lag
uniformly per octave and never sit on the edges of the filter's paths.  Stereo decoder, 64 streams x 36 frames (36 frames of 960
samples pass every one of the ring's 32 phases) of stereo packets and 32 streams x 36 frames of mono packets, crafted by
rc_craft.celt_frame(160, channels, postfilter=(octave, low, qg, tapset), transient=..., fill=LCG bytes):

* the lag of (stream s, frame f) is LAGS[(5 f + s) mod 36]: 15, 16, 17, 63 .. 68, 118 .. 124, 127 .. 129, 510 .. 516, 956 .. 966 even,
  1018, 1020, 1021, 1022 -- around the minimum, the 64-sample step (lag 66), the second call's first sample (lag 118 .. 122), the
  span of 512 history samples and the longest lag;
* every fourth frame has the post-filter off (cross-fade-only frames and off -> on frames follow from it), tapsets 0 / 1 / 2, gain
  indices 0 and 7, one frame in six transient.

The oracle must decode each packet to 960 samples and report the crafted lag in its header tap.  The classes of history windows
the frames reach are counted on the CPU (no GPU) by replaying the filter's step rule with the oracle's taps and the frame index,
and an empty class fails: a step's 68-sample window wholly in the ring; across the ring's end; across ring and this frame's
buffer; a history span longer than 512 samples; a step shorter than 64 samples (short lag); a cross-fade with both lags >= 66;
one with a lag below 66.  On the GPU the batches run step by step and as ONE queued window; EVERY step's PCM and result codes are
compared.  The bar is equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import rc_craft
from test_gpu_pipeline import run_queued

FRAMES = 36
LAGS = [15, 16, 17, 63, 64, 65, 66, 67, 68, 118, 119, 120, 121, 122, 123, 124, 127, 128, 129, 510, 511, 512, 513, 514, 515, 516,
        956, 958, 960, 962, 964, 966, 1018, 1020, 1021, 1022]
BATCHES = {"stereo": (64, 2, 0xFC, 0xC0B00A00), "mono_in_stereo": (32, 1, 0xF8, 0xC0B00B00)}  # streams, packet channels, TOC, fill seed
CLASSES = ("in_ring", "ring_end", "ring_and_buffer", "span_over_512", "short_step", "fade_both_66", "fade_one_below_66")
RING, OVERLAP = 2048, 120


def _pkg():
    from conftest import load_pkg
    return load_pkg()


def _frame_params(s, f):
    """-> (lag or None, qg, tapset, transient) of stream s, frame f"""
    lag = None if f % 4 == 3 else LAGS[(5 * f + s) % len(LAGS)]
    return lag, (0 if (s + f) % 2 else 7), (s + f) % 3, int((f + s) % 6 == 0)


def _count_call(count, pos, off, N, T0, T1, g0, g1, tap0, tap1):
    """comb_filter's step rule (og_celt.hpp), windows classified"""
    if g0 == 0 and g1 == 0:
        return
    T0, T1 = max(T0, 15), max(T1, 15)
    overlap = 0 if (g0 == g1 and T0 == T1 and tap0 == tap1) else OVERLAP
    use0, use1 = g0 != 0, g1 != 0
    chunk_fade = min(T0 if use0 else 1 << 20, T1 if use1 else 1 << 20) - 2
    end = overlap if g1 == 0 else N
    if overlap and use0 and use1:
        count["fade_both_66" if min(T0, T1) >= 66 else "fade_one_below_66"] += 1
    base = 0
    while base < end:
        lim = min(chunk_fade if base < overlap else T1 - 2, 64, end - base)
        count["short_step"] += lim < 64 and lim < end - base
        for T, used in ((T1, use1), (T0, use0 and base < overlap)):
            if not used:
                continue
            first = off + base - T - 2
            if first >= 0:
                continue
            head = (pos + first) % RING
            if first + 67 >= 0:
                count["ring_and_buffer"] += 1
            elif head + 67 > RING - 1:
                count["ring_end"] += 1
            else:
                count["in_ring"] += 1
        base += lim
    for T, used in ((T1, use1), (T0, use0)):
        count["span_over_512"] += used and off - T - 2 < -512


@functools.lru_cache(maxsize=None)
def _reference(name):
    """-> packets[frame][stream], oracle PCM [frames, n, 1920], class counts.  Computed once, read-only."""
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    n, pch, toc, seed = BATCHES[name]
    fill = pkg.lcg_payloads(n, FRAMES, 160, seed_base=seed)
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
        T_prev, g_prev, tap_prev = 0, 0, 0  # the post-filter the frame before left (period == period_old after a 20 ms frame)
        for f in range(FRAMES):
            lag, qg, tapset, transient = _frame_params(s, f)
            pf = None
            if lag is not None:
                octave = (lag + 1).bit_length() - 5
                pf = (octave, lag + 1 - (16 << octave), qg, tapset)
            pk[f][s] = bytes([toc]) + rc_craft.celt_frame(160, pch, postfilter=pf, transient=transient, fill=fill[f, s])
            ref, r = d.decode(pk[f][s])
            assert r == 960, (name, s, f, r)
            pcm[f, s] = ref[:960].reshape(-1)
            assert oracle.lib.oc_taps_copy(d.h, 4, 0, hdr.ctypes.data) == hdr.nbytes
            T, g = int(hdr[7]), int(hdr[8])
            assert int(hdr[0]) == transient, (name, s, f)
            assert (g != 0) == (lag is not None) and (lag is None or (T == lag and g == 3072 * (qg + 1))), (name, s, f, lag, T, g)
            tap = tapset if lag is not None else 0
            pos = (960 * f) % RING
            _count_call(count, pos, 0, 120, T_prev, T_prev, g_prev, g_prev, tap_prev, tap_prev)
            _count_call(count, pos, 120, 840, T_prev, T, g_prev, g, tap_prev, tap)
            T_prev, g_prev, tap_prev = T, g, tap
    pcm.setflags(write=False)
    return pk, pcm, count


@pytest.mark.parametrize("name", list(BATCHES))
def test_every_class_of_history_window_occurs(name):
    """(no GPU) every lag crafts, decodes to 960 samples and comes back in the oracle's header tap; no class is empty"""
    count = _reference(name)[2]
    print(name, count)
    empty = [c for c in CLASSES if count[c] == 0]
    assert not empty, (name, empty, count)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_every_step_matches_the_oracle(pkg, gpu_ctx, name, route):
    n, _, toc, _ = BATCHES[name]
    pk, ref, _ = _reference(name)
    lens = np.full((FRAMES, n), 161, dtype=np.int64)
    offs = (np.arange(FRAMES * n, dtype=np.int64) * 161).reshape(FRAMES, n)
    arena = np.frombuffer(b"".join(p for row in pk for p in row) + bytes(16), dtype=np.uint8).copy()
    tocs = np.full((FRAMES, n), toc, dtype=np.uint8)
    if route == "in_order":
        pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens - 1, tocs, pipeline=False)
    else:
        pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens - 1, tocs, pipeline=True, window=True, modes=pkg.toc_modes(toc))
    assert (res == 960).all(), (name, route, "result codes of (frame, stream)", np.argwhere(res != 960)[:4].tolist())
    bad = (pcm != ref).any(axis=-1)
    assert not bad.any(), (name, route, "PCM of (frame, stream)", np.argwhere(bad)[:8].tolist(), "frames that differ per step",
                           bad.sum(axis=1).tolist())
