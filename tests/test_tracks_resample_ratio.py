"""Track ratios of the whole-file path (include/opusgpu.h, TRACK RATIOS), what needs no GPU: the exported symbols, the taps against a
float64 numpy restatement of their recipe, the quality of the integer filter against scipy's resample_poly, the layout helper, the
refusals that the C calls and decode_files raise before any device work, and the kernel's resources.  resample_ratio_ref is the
numpy restatement of the header's VALUE rule that every bit-for-bit check (tests/test_gpu_tracks_resample_ratio.py) compares
against."""
import os
import re

import numpy as np
import pytest

from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_mix import mix_ref, record
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_resample_ratio_taps", "opusgpu_resample_ratio_layout", "opusgpu_tracks_resample_ratio_device", "opusgpu_files_decode_ratio",
       "opusgpu_ms_files_decode_ratio"]
RATIOS = [(147, 160), (2, 3), (147, 320), (147, 640), (5, 8), (1, 2)]


def resample_ratio_ref(x, up, down, taps, mono=False, mix=None):
    """TRACK RATIOS, VALUE: x int16 [n, channels], all of it signal (the FINAL length), zeros outside -> int16 [ceil(n up / down),
    output channels].  up / down reduced, taps: opusgpu_resample_ratio_taps(up, down); mix: an int16 Q14 matrix [out, in].  Every
    output takes the taps of its phase, h[p], h[p + up], ..., against x[b], x[b - 1], ...; int64 throughout."""
    x = np.asarray(x)
    x = x[:, None] if x.ndim == 1 else x
    assert not (mono and mix is not None)
    if mix is not None:
        x = mix_ref(x, np.asarray(mix))
    x = x.astype(np.int64)
    if mono:
        assert x.shape[1] <= 2
        x = (x.sum(axis=1, keepdims=True) + 1) >> 1 if x.shape[1] == 2 else x
    h = np.asarray(taps).astype(np.int64)
    lp, c = 24 * down + 1, 12 * down
    assert len(h) == lp and np.gcd(up, down) == 1
    n = len(x)
    m = np.arange(-(-n * up // down), dtype=np.int64)
    if not len(m):
        return np.zeros((0, x.shape[1]), dtype=np.int16)
    t = m * down + c
    p, b = t % up, t // up
    T = -(-lp // up)
    k = p[:, None] + np.arange(T, dtype=np.int64)[None, :] * up        # tap index of x[b - j]
    hk = np.where(k < lp, h[np.minimum(k, lp - 1)], 0)
    idx = b[:, None] - np.arange(T, dtype=np.int64)[None, :]           # sample index
    pad = np.zeros((T + max(int(b.max()) + 1, n), x.shape[1]), dtype=np.int64)  # pad[i] = x[i - T]
    pad[T:T + n] = x
    assert idx.min() + T >= 0
    acc = np.stack([(pad[:, ch][idx + T] * hk).sum(axis=1) for ch in range(x.shape[1])], axis=1)
    assert np.abs(acc).max(initial=0) + 16384 < 2 ** 31
    return np.clip((acc + 16384) >> 15, -32768, 32767).astype(np.int16)


def taps_restated(up, down):
    """TAPS in float64 numpy: -> (int64 table [Lp], the largest per-phase sum |h|)."""
    lp, c = 24 * down + 1, 12 * down
    i = np.arange(lp, dtype=np.float64)
    fc = 0.92 / down
    g = fc * np.sinc(fc * (i - c)) * np.i0(8 * np.sqrt(np.maximum(0, 1 - ((i - c) / c) ** 2))) / np.i0(8.0)
    h = np.zeros(lp, dtype=np.int64)
    worst = 0
    for p in range(up):
        q = np.rint(g[p::up] * (32768 / g[p::up].sum())).astype(np.int64)
        q[int(np.argmax(q))] += 32768 - q.sum()  # argmax: the first of the largest
        h[p::up] = q
        worst = max(worst, int(np.abs(q).sum()))
    return h, worst


def test_symbols_header_and_exports(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "TRACK RATIOS" in hdr and hdr.index("TRACK RATES.") < hdr.index("TRACK RATIOS.") < hdr.index("TRACK FEATURES.")
    for name in ("resample_ratio_taps", "resample_ratio_layout", "track_ratio_args"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.Context.tracks_resample_ratio_device)


@pytest.mark.parametrize("up,down", RATIOS)
def test_taps(pkg, up, down):
    h = pkg.resample_ratio_taps(up, down).astype(np.int64)
    assert h.dtype == np.int64 and pkg.load_lib().opusgpu_resample_ratio_taps(up, down, None) == len(h) == 24 * down + 1
    sums = [int(h[p::up].sum()) for p in range(up)]
    abs_sums = [int(np.abs(h[p::up]).sum()) for p in range(up)]
    assert set(sums) == {32768} and max(abs_sums) <= 65535
    want, worst = taps_restated(up, down)
    print(f"{up}/{down}: largest difference from the float64 restatement {np.abs(h - want).max()} LSB, largest phase sum |h| {max(abs_sums)}"
          f" (restated {worst})")
    assert np.abs(h - want).max() <= 1
    assert worst <= 59248  # the restatement's largest over RATIOS
    # unreduced pairs are the reduced ones
    assert np.array_equal(pkg.resample_ratio_taps(3 * up, 3 * down), h)


def test_the_named_rates_are_ratios(pkg):
    assert pkg.track_ratio(44100) == (147, 160) and pkg.track_ratio(32000) == (2, 3) and pkg.track_ratio(22050) == (147, 320)
    assert pkg.track_ratio(11025) == (147, 640) and pkg.track_ratio((294, 320)) == (147, 160) and pkg.track_ratio(24000) == (1, 2)
    assert pkg.track_ratio(np.int64(44100)) == (147, 160) and pkg.track_ratio([np.int32(2), 3]) == (2, 3)
    lib = pkg.load_lib()
    for up, down in ((1, 1), (3, 2), (160, 160), (1, 9), (161, 162), (100, 641), (81, 641), (0, 3), (2, 0), (-2, 3), (2, -3), (-2, -3)):
        assert lib.opusgpu_resample_ratio_taps(up, down, None) == pkg.OPUSGPU_BAD_ARG, (up, down)
        with pytest.raises(ValueError):
            pkg.resample_ratio_taps(up, down)
        with pytest.raises(ValueError):
            pkg.track_ratio((up, down))
    for bad in (48000, 96000, 0, -44100, 5000, 44100.0, "44100", (2,), (2, 3, 4), (2.0, 3), None, True):
        with pytest.raises(ValueError):
            pkg.track_ratio(bad)
    # the edges of the set
    for up, down in ((160, 161), (1, 8), (80, 640), (159, 160), (480, 483)):
        assert lib.opusgpu_resample_ratio_taps(up, down, None) == 24 * (down // np.gcd(up, down)) + 1
    # TRACK RATES is as it was
    assert lib.opusgpu_resample_taps(44100, None) == pkg.OPUSGPU_BAD_ARG and lib.opusgpu_resample_taps(32000, None) == pkg.OPUSGPU_BAD_ARG


def test_taps_from_two_threads(pkg):
    """Two threads that ask for a table nobody has asked for get the same one."""
    import threading
    got = [None, None]

    def ask(i):
        got[i] = pkg.resample_ratio_taps(11, 23)
    threads = [threading.Thread(target=ask, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert np.array_equal(got[0], got[1]) and len(got[0]) == 24 * 23 + 1 and np.array_equal(got[0], pkg.resample_ratio_taps(11, 23))


@pytest.mark.parametrize("up,down", RATIOS)
def test_reference_restatement_by_hand(pkg, up, down):
    """resample_ratio_ref on cases small enough to work out: an impulse hands out the taps of every output's phase, a constant
    comes back exactly away from the ends, the length is ceil(len up / down)."""
    h = pkg.resample_ratio_taps(up, down)
    c = 12 * down
    n_at = 30  # the impulse: output m meets tap m down + c - n_at up
    x = np.zeros((60 * down // up + 60, 1), dtype=np.int16)
    x[n_at] = 32767
    y = resample_ratio_ref(x, up, down, h)[:, 0]
    k = np.arange(len(y), dtype=np.int64) * down + c - n_at * up
    want = np.where((k >= 0) & (k < len(h)), (32767 * h.astype(np.int64)[np.clip(k, 0, len(h) - 1)] + 16384) >> 15, 0)
    assert np.array_equal(y, want) and np.count_nonzero(y) > 10
    flat = resample_ratio_ref(np.full((80 * down // up + 80, 2), -1234, dtype=np.int16), up, down, h)
    edge = 12 + 2  # the filter's half length in outputs, and the rounding of the two grids
    assert (flat[edge:-edge] == -1234).all() and len(flat) > 4 * edge
    for n in (0, 1, 2, down, down + 1, 1000):
        assert len(resample_ratio_ref(np.zeros((n, 1), dtype=np.int16), up, down, h)) == -(-n * up // down)
    lr = np.array([[1, 2], [-1, -2], [-3, 0]] * 200, dtype=np.int16)
    assert np.array_equal(resample_ratio_ref(lr, up, down, h, mono=True),
                          resample_ratio_ref(np.array([2, -1, -1] * 200, dtype=np.int16), up, down, h))
    assert np.array_equal(resample_ratio_ref(lr, up, down, h, mix=[[8192, 8192]]), resample_ratio_ref(lr, up, down, h, mono=True))


@pytest.mark.parametrize("up,down", RATIOS + [(3, 4)])
def test_quality_against_resample_poly(pkg, up, down):
    """The integer filter is no worse than scipy's default resample_poly, in test_tracks_resample.py's setting: sines of amplitude
    16000, one second at 48 kHz, 200 outputs left out at both ends.  Pass band: worst RMS error against the ideal resampled sine over
    the tones {0.05, 0.2, 0.35} fs_out.  Stop band: worst output RMS over those of {0.6, 0.65, 0.8, 0.95} fs_out that exist below
    the input's Nyquist (f up / down <= 0.48): a resampler must remove them, they alias.  For 147 / 160 none does, for 3 / 4 only
    0.6 fs_out (0.45 of the input rate), and only the pass band is held where there is none."""
    signal = pytest.importorskip("scipy.signal")
    h = pkg.resample_ratio_taps(up, down)
    n = np.arange(48000)
    m = np.arange(-(-48000 * up // down))[200:-200]
    rms = lambda e: float(np.sqrt(np.mean(np.square(e))))
    ours_pass, poly_pass, ours_stop, poly_stop = [], [], [], []
    for f in (0.05, 0.2, 0.35):  # in units of fs_out: f up / down of the input rate
        x = np.round(16000 * np.sin(2 * np.pi * f * up / down * n))
        ideal = 16000 * np.sin(2 * np.pi * f * m)
        ours_pass.append(rms(resample_ratio_ref(x.astype(np.int16), up, down, h)[200:-200, 0] - ideal))
        poly_pass.append(rms(signal.resample_poly(x, up, down)[200:-200] - ideal))
    stops = [f for f in (0.6, 0.65, 0.8, 0.95) if f * up / down <= 0.48]
    assert bool(stops) == ((up, down) != (147, 160)) and (stops == [0.6] or (up, down) != (3, 4))
    for f in stops:
        x = np.round(16000 * np.sin(2 * np.pi * f * up / down * n))
        ours_stop.append(rms(resample_ratio_ref(x.astype(np.int16), up, down, h)[200:-200, 0]))
        poly_stop.append(rms(signal.resample_poly(x, up, down)[200:-200]))
    print(f"{up}/{down}: pass-band error {max(ours_pass):.2f} LSB (resample_poly {max(poly_pass):.2f}), alias residue over {stops}: "
          f"{max(ours_stop, default=0):.2f} LSB (resample_poly {max(poly_stop, default=0):.2f})")
    assert max(ours_pass) <= max(poly_pass), (ours_pass, poly_pass)
    if stops:
        assert max(ours_stop) <= max(poly_stop), (ours_stop, poly_stop)


def test_layout_helper(pkg):
    planned = np.array([0, 1, 63, 64, 65, 64 * 6, 64 * 6 + 1, 0, 100000, 7], dtype=np.int64)
    for up, down in RATIOS + [(3, 4), (294, 320)]:
        offs, total = pkg.resample_ratio_layout(planned, up, down)
        lens = -(-planned * up // down)
        want = np.concatenate([[0], np.cumsum((lens + 63) // 64 * 64)])
        assert (offs % 64 == 0).all() and np.array_equal(offs, want[:-1]) and total == want[-1], (up, down)
        assert offs[1] == 0 and offs[8] == offs[7]  # an empty track takes no room
    offs, total = pkg.resample_ratio_layout([], 2, 3)
    assert len(offs) == 0 and total == 0
    lib = pkg.load_lib()
    assert lib.opusgpu_resample_ratio_layout(planned.size, planned.ctypes.data, 2, 3, None) == pkg.resample_ratio_layout(planned, 2, 3)[1]
    big = np.array([2 ** 40 + 1], dtype=np.int64)  # the product with `up` does not fit 32 bits, nor 2^31 outputs
    assert pkg.resample_ratio_layout(big, 147, 160)[1] == (-(-(2 ** 40 + 1) * 147 // 160) + 63) // 64 * 64
    for up, down in ((3, 2), (1, 1), (0, 1), (1, 9), (161, 162)):
        with pytest.raises(ValueError):
            pkg.resample_ratio_layout(planned, up, down)
    with pytest.raises(ValueError):
        pkg.resample_ratio_layout([5, -1], 2, 3)


BAD_RATIOS = [(3, 2), (2, 2), (1, 9), (100, 641), (161, 162), (0, 3), (2, 0), (-2, 3), (2, -3)]  # up >= down, down > 8 up, > 640, up > 160, <= 0


def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """Every refusal of the three device-facing calls comes back as OPUSGPU_BAD_ARG with d_in / d_out NULL, from real decoders
    where there is a device and from zeroed memory where there is none (test_tracks_resample.py::handles)."""
    lib = pkg.load_lib()
    S16, F32, PL = pkg.TRACKS_S16, pkg.TRACKS_F32, pkg.TRACKS_F32_PLANAR
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    n = batch.n_files
    one = np.ones(n, dtype=np.float32)
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)
    inf = np.array([np.inf] + [1] * (n - 1), dtype=np.float32)
    ok2, ok6 = record(pkg, [[8192, 8192]]), record(pkg, pkg.downmix_matrix(6, 2))
    over2 = record(pkg, [[16384, 0], [32767, -32768], [0, 1]])
    over2["m"][0, 1, 0] = -32768  # a row of abs-sum 65536
    ptr = lambda a: None if a is None else a.ctypes.data

    def files(up, down, mono, mix, fmt, scale, ctx=fake, b=batch.h):
        return lib.opusgpu_files_decode_ratio(ctx, b, up, down, mono, ptr(mix), fmt, ptr(scale), None, None, None, None, None)

    def ms_files(up, down, mix, fmt, scale, ms=fake_ms, b=ms_batch.h):
        return lib.opusgpu_ms_files_decode_ratio(ms, b, up, down, ptr(mix), fmt, ptr(scale), None, None, None, None, None)
    assert files(2, 3, 0, None, S16, None, ctx=None) == BAD and files(2, 3, 0, None, S16, None, b=None) == BAD
    assert ms_files(2, 3, None, S16, None, ms=None) == BAD and ms_files(2, 3, None, S16, None, b=None) == BAD
    for up, down in BAD_RATIOS:
        assert files(up, down, 0, None, S16, None) == BAD and files(up, down, 1, None, F32, None) == BAD, (up, down)
        assert files(up, down, 0, ok2, S16, None) == BAD and ms_files(up, down, None, S16, None) == BAD, (up, down)
        assert ms_files(up, down, ok6, PL, None) == BAD, (up, down)
    for mono, mix, fmt, scale in ((0, None, 3, None), (1, None, -1, None),          # unknown formats
                                  (1, ok2, S16, None), (1, ok2, F32, None),         # mono together with a mix
                                  (0, over2, S16, None), (0, ok6, S16, None),       # a matrix CHANNEL MIX refuses, or of other tracks
                                  (0, None, S16, one), (1, None, S16, one),         # a scale with S16
                                  (0, None, F32, nan), (1, None, PL, inf), (0, ok2, F32, nan)):  # a scale that is not finite
        assert files(147, 160, mono, mix, fmt, scale) == BAD, (mono, fmt)
    for mix, fmt, scale in ((None, 3, None), (ok2, S16, None), (None, S16, one), (ok6, S16, one), (None, F32, nan), (ok6, PL, nan)):
        assert ms_files(2, 3, mix, fmt, scale) == BAD, fmt

    spans = np.zeros(2, dtype=pkg.RESAMPLE_SPAN_DTYPE)
    spans["in_samples"], spans["scale"], spans["out_plane"] = 100, 1.0, 128
    spans["in_offset"], spans["out_offset"] = [0, 128], [0, 128]

    def kernel(s, channels, up, down, mono, mix, fmt, ctx=fake):
        return lib.opusgpu_tracks_resample_ratio_device(ctx, len(s), s.ctypes.data, None, channels, up, down, mono, ptr(mix), fmt, None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    assert kernel(spans, 2, 2, 3, 0, None, S16, ctx=None) == BAD
    for up, down in BAD_RATIOS:
        assert kernel(spans, 2, up, down, 0, None, S16) == BAD and kernel(spans, 2, up, down, 0, ok2, F32) == BAD, (up, down)
    for channels, mono, mix, fmt in ((3, 1, None, F32), (6, 1, None, S16), (0, 0, None, S16), (9, 0, None, S16), (2, 0, None, 3),
                                     (2, 1, ok2, S16), (2, 0, over2, S16), (6, 0, ok2, S16), (2, 0, ok6, S16)):
        assert kernel(spans, channels, 147, 160, mono, mix, fmt) == BAD, (channels, mono, fmt)
    assert -(-100 * 147 // 160) == 92 and -(-140 * 147 // 160) == 129
    for s, fmt in ((but(in_offset=4), S16), (but(in_offset=-8), S16), (but(in_samples=-1), S16), (but(out_offset=32), S16),
                   (but(out_offset=-64), S16), (but(out_plane=32), PL), (but(in_samples=140), PL), (but(scale=np.nan), F32),
                   (but(scale=np.inf), PL)):
        assert kernel(s, 2, 147, 160, 0, None, fmt) == BAD
    # these are in order, unreduced pairs included: refused for the NULL buffers, still before the device
    for up, down in ((147, 160), (294, 320), (2, 3), (20, 30), (1, 8)):
        assert kernel(spans, 2, up, down, 0, None, PL) == BAD and kernel(spans, 6, up, down, 0, ok6, S16) == BAD
        assert kernel(spans, 2, up, down, 1, None, F32) == BAD
    assert kernel(but(scale=np.nan), 2, 2, 3, 0, None, S16) == BAD  # (the scale is not read for S16: the NULL buffers again)
    empty = spans.copy()
    empty["in_samples"] = 0
    # nothing to do is no error and no device work; an unreduced pair is accepted
    assert kernel(empty, 2, 294, 320, 0, None, S16) == 0 and kernel(spans[:0], 6, 20, 30, 0, ok6, F32) == 0
    assert kernel(empty, 2, 147, 160, 1, None, PL) == 0


def test_python_refusals_need_no_device(pkg, batch):
    """track_ratio_args, and decode_files raising before it touches its decoder (an object without one is enough to see it)."""
    (up, down), ch, offs, total, out, rec = pkg.track_ratio_args(batch, 44100, True, None, "f32")
    assert (up, down, ch, out, rec) == (147, 160, 1, None, None)
    assert total == pkg.resample_ratio_layout(batch.info["track_samples"], 147, 160)[1] and len(offs) == batch.n_files
    assert pkg.track_ratio_args(batch, (4, 6))[:2] == ((2, 3), 2)
    q = pkg.track_ratio_args(batch, 32000, mix="mono")
    assert q[:2] == ((2, 3), 1) and q[5]["out_channels"][0] == 1
    for kw in (dict(resample=48000), dict(resample=(3, 2)), dict(resample=44100.0), dict(resample="44100"), dict(resample=(1, 9)),
               dict(resample=44100, rate=16000), dict(resample=44100, rate=48000), dict(resample=(1, 3), features="logmel", mono=True),
               dict(resample=44100, format="f64"), dict(resample=44100, mono=True, allow_mono=False),
               dict(resample=44100, mono=True, mix="mono"), dict(resample=44100, mix="quad"), dict(resample=44100, mix=[[1, 2, 3]])):
        with pytest.raises(ValueError):
            pkg.track_ratio_args(batch, **kw)
    six = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files, "track_samples": batch.track_samples})()
    with pytest.raises(ValueError):
        pkg.track_ratio_args(six, 32000, True)
    assert pkg.track_ratio_args(six, 32000)[:2] == ((2, 3), 6) and pkg.track_ratio_args(six, 32000, mix="stereo")[:2] == ((2, 3), 2)
    # `out` is held against the RESAMPLED size
    need = total
    assert pkg.track_ratio_args(batch, 44100, True, None, "f32", Tensor(need), 0)[4] is not None
    for t, fmt, dev in ((Tensor(need - 1), "f32", 0), (Tensor(need, dtype="torch.int16"), "f32", 0), (Tensor(need), "s16", 0),
                        (Tensor(need, device=("cpu", None)), "f32", 0), (Tensor(need), "f32", 1), (Tensor(need, ptr=4096 + 64), "f32", 0),
                        (Tensor(need, contiguous=False), "f32", 0)):
        with pytest.raises(ValueError):
            pkg.track_ratio_args(batch, 44100, True, None, fmt, t, dev)
    with pytest.raises(ValueError):
        pkg.track_ratio_args(batch, 44100, False, None, "f32", Tensor(2 * need - 1), 0)  # stereo takes twice as much
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for kw in (dict(resample=44100, rate=16000), dict(resample=44100, features="logmel", mono=True),
               dict(resample=44100, mono=True, format="f32", out=Tensor(need - 1)), dict(resample=(3, 2)), dict(resample=96000),
               dict(resample=44100, format="s16", scale=np.ones(batch.n_files)), dict(resample=44100, format="f32", scale=[np.nan] * 4),
               dict(resample=44100, mono=True, mix="mono"), dict(resample=44100, format="f64")):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, **kw)
    ms = pkg.MultistreamContext.__new__(pkg.MultistreamContext)
    ms.h, ms.device = None, 0
    for kw in (dict(resample=32000, rate=16000), dict(resample=32000, features="logmel", mix="mono"), dict(resample=(3, 2)),
               dict(resample=32000, mix="stereo", format="f32", out=Tensor(7)), dict(resample=32000, format="s16", scale=np.ones(batch.n_files))):
        with pytest.raises(ValueError):
            ms.decode_files(None, batch=six, **kw)
    # TRACK RATES refuses what it refused
    for kw in (dict(rate=44100), dict(rate=32000)):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, **kw)


def test_kernel_keeps_out_of_scratch():
    """k_tracks_resample_ratio from the built library: no scratch, at most 128 vector registers (four waves per SIMD and more), no
    static LDS -- its window planes, tap groups and results are dynamic, sized per launch, at most 64 KB."""
    meta = _kernel_metadata()
    seen = {k: v for k, v in meta.items() if re.search(r"\d+k_tracks_resample_ratio", k)}
    print({k[:40]: v for k, v in seen.items()})
    assert len(seen) == 1, sorted(meta)[:6]
    vgpr, scratch, lds = next(iter(seen.values()))
    print(f"k_tracks_resample_ratio: {vgpr} VGPRs, {scratch} bytes of scratch, {lds} bytes of static LDS")
    assert vgpr <= 128 and scratch == 0 and lds == 0
