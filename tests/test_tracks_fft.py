"""TRACK STFT by FFT (include/opusgpu.h, TRACK STFT, OPUSGPU_STFT_ALGO_FFT), what needs no GPU: the record and its refusals, the
window and twiddle tables, the float64 reference fft_ref against the matrix definition (tests/test_tracks_stft.py::stft_ref) and
against torch.stft, the float32 yardstick fft_f32 of the GPU test's tolerance, the layout at 2049 and 4097 bins, the refusals that
come before any device work, and the kernel's resources.  fft_ref is what the GPU checks (tests/test_gpu_tracks_fft.py) compare
against; crafted_tracks are the tracks both are measured on.  Every test here fails without the feature: stft_spec has no algo= and
the library no opusgpu_stft_fft_tables."""
import functools
import os
import re
import zlib

import numpy as np
import pytest

from test_stft_batch import good_request
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)
from test_tracks_stft import _kernel_metadata, error_of, finish, frame_count, frames_of, kept_cells, stft_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (sr, n_fft, win, hop, power (None: complex), log, floor, frames): the smallest shapes at which k_tracks_fft can still go wrong
SETS = {
    "fft_tiny": (8000, 64, 48, 24, 2, "ln", 1e-10, "torch"),             # smallest size, win < n_fft, hop no multiple of 8, 33 bins
    "fft_enh": (16000, 512, 400, 128, None, None, 0.0, "torch"),          # M = 256, pairs, frames-major rows of 257 pairs
    "fft_vits": (22050, 1024, 1024, 256, 1, None, 0.0, "torch"),          # M = 512 (odd exponent); the dense "vits" record
    "fft_wide": (44100, 2048, 2048, 960, 2, "log10", 1e-10, "torch"),     # the dense "wide" record
    "fft_sep": (44100, 4096, 4096, 1024, None, None, 0.0, "torch"),       # first size the dense path refuses; Open-Unmix's numbers
    "fft_big": (48000, 8192, 6000, 1000, 2, "log10", 1e-10, "whisper"),   # largest size, zero-padded window, F = n / hop
}
LAYOUTS = {"fft_tiny": ("bands", "frames"), "fft_enh": ("bands", "frames"), "fft_vits": ("bands",), "fft_wide": ("bands", "frames"),
           "fft_sep": ("bands", "frames"), "fft_big": ("bands", "frames")}
# opusgpu_stft_tile of an FFT record: the larger of 16 and 8192 / n_fft
TILES = {"fft_tiny": 128, "fft_enh": 16, "fft_vits": 16, "fft_wide": 16, "fft_sep": 16, "fft_big": 16}


def fft_of(pkg, name, feature_layout="bands", **kw):
    sr, n_fft, win, hop, power, log, floor, frames = SETS[name]
    args = dict(win_length=win, power=power, log=log, floor=floor, frames=frames, feature_layout=feature_layout, algo="fft")
    args.update(kw)
    return pkg.stft_spec(sr, n_fft, hop, **args)


def tile_of(rec):
    return max(16, 8192 // int(rec["n_fft"][0]))


def window64(rec):
    """w[i] of the header's WINDOW in float64, [n_fft]."""
    n_fft, win = int(rec["n_fft"][0]), int(rec["win_length"][0]) or int(rec["n_fft"][0])
    left = (n_fft - win) // 2
    i = np.arange(n_fft)
    return np.where((i >= left) & (i < left + win), 0.5 - 0.5 * np.cos(2.0 * np.pi * (i - left) / float(win)), 0.0)


# ---- the reference and the yardstick ------------------------------------------------------------------------
def fft_ref(y, scale, rec):
    """TRACK STFT in float64 by numpy's FFT: y int16 [n] -> (output [F, bins] float64 or complex128, S [F, bins]).  Frames by
    frames_of, the sample the float32 product (float)y * scale, the window in double, np.fft.rfft (e^{-ia}: torch.stft's sign)."""
    y = np.asarray(y, dtype=np.int16)
    q, inside = frames_of(y, rec)
    x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
    fr = np.where(inside, x[q] if len(y) else 0.0, 0.0)
    Z = np.fft.rfft(fr * window64(rec)[None, :], axis=1)
    return finish(np.ascontiguousarray(Z.real), np.ascontiguousarray(Z.imag), rec)


def fft_f32(y, scale, rec, window, twiddle):
    """The same value in float32 throughout: x * window in float32, then an iterative radix-2 decimation-in-time FFT of n_fft
    complex points with the library's twiddles (cos, sin of 2 pi j / n_fft: the forward factor is cos - i sin), bins 0 .. n_fft / 2
    of it.  The yardstick of the kernel's tolerance (the kernel may differ from float64 by 8 x what this does)."""
    y = np.asarray(y, dtype=np.int16)
    n_fft = int(rec["n_fft"][0])
    q, inside = frames_of(y, rec)
    x = y.astype(np.float32) * np.float32(scale)
    fr = np.where(inside, x[q] if len(y) else np.float32(0), np.float32(0)).astype(np.float32) * window[None, :]
    assert fr.dtype == np.float32
    bits = n_fft.bit_length() - 1
    j = np.arange(n_fft)
    rev = np.zeros(n_fft, dtype=np.int64)
    for b in range(bits):
        rev |= ((j >> b) & 1) << (bits - 1 - b)
    a = fr[:, rev].astype(np.complex64)
    w = (twiddle[:, 0] - 1j * twiddle[:, 1]).astype(np.complex64)
    h = 1
    while h < n_fft:
        a = a.reshape(len(fr), n_fft // (2 * h), 2, h)
        t = a[:, :, 1, :] * w[None, None, ::n_fft // (2 * h)]
        a = np.stack([a[:, :, 0, :] + t, a[:, :, 0, :] - t], axis=2)
        assert a.dtype == np.complex64
        h *= 2
    a = a.reshape(len(fr), n_fft)[:, :n_fft // 2 + 1]
    out = finish(np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag), rec)[0]
    assert out.dtype == (np.complex64 if int(rec["power"][0]) == 0 else np.float32)
    return out


def lengths_of(rec):
    """tests/test_tracks_stft.py::lengths_of's pattern for the record's hop H, n_fft N and the FFT kernel's tile T."""
    H, N, T = int(rec["hop"][0]), int(rec["n_fft"][0]), tile_of(rec)
    want = [0, 1, H - 1, H, H + 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1, N, 2 * H - 1, 2 * H, 32 * H - 1, 32 * H, 32 * H + 1,
            T * H - 1, T * H, T * H + 1, T * H + H + 1]
    return list(dict.fromkeys(want))


_PKG = []


@pytest.fixture(autouse=True)
def _keep_pkg(pkg):
    _PKG[:] = [pkg]


@functools.lru_cache(maxsize=None)
def crafted_tracks(name):
    """(tracks, scales): every length of lengths_of twice, uniform random int16 -- once with the default scale, once with a random
    finite one --, an all-zero track under a negative scale, a track of +-40 noise, and one tone over noise: a sine of amplitude
    6000 plus Gaussian noise of sigma 300, rounded.  No bare tone: an int16 sine leaves most of its cells under 1e-8 x the frame's
    largest, and the 1 % cap on cells not kept is a condition the reference must meet on its own."""
    rng = np.random.default_rng(zlib.crc32(("fft " + name).encode()))
    rec = fft_of(_PKG[0], name)
    H, N = int(rec["hop"][0]), int(rec["n_fft"][0])
    tracks, scales = [], []
    for n in lengths_of(rec):
        for k in range(2):
            tracks.append(rng.integers(-32768, 32768, n, dtype=np.int16))
            scales.append(2.0 ** -15 if k == 0 else float(rng.choice([-1, 1]) * rng.uniform(1, 10) * 10.0 ** rng.integers(-6, 3)))
    tracks.append(np.zeros(H * 5 + 3, dtype=np.int16))
    scales.append(-2.0 ** -15)  # a negative scale: the zero track's cells must still be +0
    tracks.append(rng.integers(-40, 41, H * 9 + 77, dtype=np.int16))
    scales.append(2.0 ** -15)
    m = np.arange(H * 9 + N + 5)
    tone = 6000.0 * np.sin(2 * np.pi * rng.uniform(0.01, 0.45) * m + rng.uniform(0, 6)) + rng.normal(0.0, 300.0, len(m))
    tracks.append(np.rint(tone).astype(np.int16))
    scales.append(2.0 ** -15)
    scales = np.asarray(scales, dtype=np.float32)
    assert np.isfinite(scales).all() and (scales != 0).all()
    return tracks, scales


@functools.lru_cache(maxsize=None)
def crafted_reference(name):
    """fft_ref of crafted_tracks: [(output [F, bins], S [F, bins])], computed once per set and shared."""
    tracks, scales = crafted_tracks(name)
    rec = fft_of(_PKG[0], name)
    refs = [fft_ref(y, s, rec) for y, s in zip(tracks, scales)]
    for out, S in refs:
        out.setflags(write=False), S.setflags(write=False)
    return refs


def yardstick(pkg, name):
    """-> (the largest error of fft_f32 against fft_ref over the kept cells of crafted_tracks, cells, cells not kept)."""
    tracks, scales = crafted_tracks(name)
    rec = fft_of(pkg, name)
    window, twiddle = pkg.stft_fft_tables(rec)
    worst, cells, dropped = 0.0, 0, 0
    for y, s, (ref, S) in zip(tracks, scales, crafted_reference(name)):
        if len(ref):
            keep = kept_cells(S, rec)
            cells, dropped = cells + keep.size, dropped + int((~keep).sum())
            worst = max(worst, float(error_of(fft_f32(y, s, rec, window, twiddle), ref, S, rec)[keep].max(initial=0)))
    return worst, cells, dropped


# ---- record and refusals ------------------------------------------------------------------------------------
def _but(rec, **kw):
    rec = rec.copy()
    for k, v in kw.items():
        rec[k] = v
    return rec


def bad_fft_records(pkg):
    good = pkg.stft_spec(16000, 512, 128, 400, power=2, log="ln", floor=1e-7, algo="fft")
    dense = pkg.stft_spec(16000, 512, 128, 400, power=2, log="ln", floor=1e-7)
    return good, [_but(good, n_fft=32, win_length=32), _but(good, n_fft=16384), _but(good, n_fft=1000), _but(good, n_fft=1536), _but(good, hop=0),
                  _but(good, hop=513), _but(good, reserved=[0, 2, 0, 0, 0, 0, 0]), _but(good, reserved=[0, -1, 0, 0, 0, 0, 0]),
                  _but(good, reserved=[1, 1, 0, 0, 0, 0, 0]), _but(good, reserved=[0, 1, 0, 0, 0, 0, 7]), _but(good, win_length=14),
                  _but(good, win_length=401), _but(good, power=0, log=1), _but(dense, n_fft=4096, win_length=0)]


def test_record_and_refusals(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    assert hasattr(lib, "opusgpu_stft_fft_tables") and "opusgpu_stft_fft_tables" in pkg.EXPORTS and re.search(r"\bopusgpu_stft_fft_tables\s*\(", hdr)
    assert re.search(r"#define OPUSGPU_STFT_ALGO_DENSE 0\b", hdr) and re.search(r"#define OPUSGPU_STFT_ALGO_FFT 1\b", hdr)
    assert (pkg.STFT_ALGO_DENSE, pkg.STFT_ALGO_FFT) == (0, 1)
    BAD = pkg.OPUSGPU_BAD_ARG
    planned = np.array([480, 960], dtype=np.int64)
    for e in range(6, 14):
        rec = pkg.stft_spec(44100, 1 << e, 1 << (e - 2), power=None, algo="fft")
        assert list(rec["reserved"][0]) == [0, 1, 0, 0, 0, 0, 0] and int(rec["n_fft"][0]) == 1 << e
        assert pkg.stft_tile(rec) == lib.opusgpu_stft_tile(rec.ctypes.data) == max(16, 8192 >> e)
        assert pkg.stft_width(rec) == (1 << e) + 2 and lib.opusgpu_stft_fft_tables(rec.ctypes.data, None, None) == 1 << e
        assert list(pkg.stft_frames(rec, [0, 1, 1 << e])) == [0, 1, 5]
    assert list(pkg.stft_spec(44100, 1024, 256)["reserved"][0]) == [0] * 7 == list(pkg.stft_spec(44100, 1024, 256, algo="dense")["reserved"][0])
    assert int(pkg.stft_spec(44100, 2048, 2048, algo="fft")["hop"][0]) == 2048  # 31 * hop + n_fft <= 32768 does not apply
    assert int(pkg.stft_spec(48000, 8192, 8192, algo="fft")["hop"][0]) == 8192
    with pytest.raises(ValueError, match="32768"):
        pkg.stft_spec(44100, 2048, 2048)
    assert {n: pkg.stft_tile(fft_of(pkg, n)) for n in SETS} == TILES == {n: tile_of(fft_of(pkg, n, "frames")) for n in SETS}
    for kw, match in ((dict(n_fft=32), "power of two"), (dict(n_fft=16384), "power of two"), (dict(n_fft=1000), "power of two"),
                      (dict(n_fft=1536), "power of two"), (dict(hop=0), r"hop must be in \[1, n_fft\]"), (dict(hop=513), r"hop must be in \[1, n_fft\]"),
                      (dict(algo="x"), "algo"), (dict(algo=1), "algo"), (dict(algo=None), "algo")):
        args = {"sample_rate": 16000, "n_fft": 512, "hop": 128, "algo": "fft", **kw}
        if "n_fft" in kw:
            args["hop"] = 16
        with pytest.raises(ValueError, match=match):
            pkg.stft_spec(**args)
    with pytest.raises(ValueError, match="multiple of 16"):
        pkg.stft_spec(44100, 4096, 1024)  # without the keyword 4096 stays refused, with today's message
    good, bad = bad_fft_records(pkg)
    assert lib.opusgpu_stft_tile(good.ctypes.data) == 16 and lib.opusgpu_stft_fft_tables(good.ctypes.data, None, None) == 512
    assert lib.opusgpu_stft_layout(2, planned.ctypes.data, 1, 3, good.ctypes.data, None) == pkg.stft_layout(planned, 1, 3, _but(good, reserved=0))[2]
    assert lib.opusgpu_stft_fft_tables(None, None, None) == BAD
    for rec in bad:
        assert lib.opusgpu_stft_tile(rec.ctypes.data) == BAD, rec
        assert lib.opusgpu_stft_layout(2, planned.ctypes.data, 1, 3, rec.ctypes.data, None) == BAD, rec
        assert lib.opusgpu_stft_fft_tables(rec.ctypes.data, None, None) == BAD, rec
        for call in (pkg.stft_tile, pkg.stft_fft_tables, lambda r: pkg.stft_layout(planned, 1, 3, r)):
            with pytest.raises(ValueError):
                call(rec)
    dense = pkg.stft_spec(16000, 512, 128, 400)
    assert lib.opusgpu_stft_fft_tables(dense.ctypes.data, None, None) == BAD  # a DENSE record has no FFT tables
    with pytest.raises(ValueError):
        pkg.stft_fft_tables(dense)
    # opusgpu_stft_basis: the dense tables for any valid record up to 2048, refused above
    sep, vits = fft_of(pkg, "fft_sep"), fft_of(pkg, "fft_vits")
    assert lib.opusgpu_stft_basis(sep.ctypes.data, None, None) == BAD
    with pytest.raises(ValueError):
        pkg.stft_basis(sep)
    wc, ws = pkg.stft_basis(vits)
    dc, ds = pkg.stft_basis(_but(vits, reserved=0))
    assert wc.shape == (1024, 513) and np.array_equal(wc.view(np.uint32), dc.view(np.uint32)) and np.array_equal(ws.view(np.uint32), ds.view(np.uint32))


@pytest.mark.parametrize("name", list(SETS))
def test_fft_tables(pkg, name):
    """Both tables are the header's formulas computed in float64 and rounded once, bit for bit; up to n_fft 2048 the window is column
    0 of Wc (cos 0 = 1)."""
    rec = fft_of(pkg, name)
    n_fft = int(rec["n_fft"][0])
    window, twiddle = pkg.stft_fft_tables(rec)
    assert window.dtype == twiddle.dtype == np.float32 and window.shape == (n_fft,) and twiddle.shape == (n_fft // 2, 2)
    assert np.array_equal(window.view(np.uint32), window64(rec).astype(np.float32).view(np.uint32))
    ang = 2.0 * np.pi * np.arange(n_fft // 2) / float(n_fft)
    assert np.array_equal(twiddle[:, 0].view(np.uint32), np.cos(ang).astype(np.float32).view(np.uint32))
    assert np.array_equal(twiddle[:, 1].view(np.uint32), np.sin(ang).astype(np.float32).view(np.uint32))
    if n_fft <= 2048:
        assert np.array_equal(window.view(np.uint32), np.ascontiguousarray(pkg.stft_basis(rec)[0][:, 0]).view(np.uint32))
    zero_win = _but(rec, win_length=0 if SETS[name][2] == n_fft else SETS[name][2])  # the C record's "0 means n_fft"
    assert np.array_equal(pkg.stft_fft_tables(zero_win)[0].view(np.uint32), window.view(np.uint32))
    assert np.array_equal(pkg.stft_fft_tables(fft_of(pkg, name, "frames"))[1].view(np.uint32), twiddle.view(np.uint32))


def _bound(rec, x):
    """test_reference_is_torch_stft's bound: both sides are float64 sums of the same n_fft products w[i] x[i] per cell in different
    orders, each off by at most n_fft * 2^-53 * sum |terms| with sum w = win / 2, and the tables' own rounding is one more 2^-53
    each: |d| <= 4 * n_fft * 2^-53 * (win / 2) * max |x| holds both differences with room (an FFT's error grows with log n_fft
    only, so it is the matrix sum's term that sets this)."""
    n_fft, win = int(rec["n_fft"][0]), int(rec["win_length"][0]) or int(rec["n_fft"][0])
    return 4 * n_fft * 2.0 ** -53 * (win / 2) * np.abs(x).max()


def test_reference_is_the_definition(pkg):
    """fft_ref's pairs against stft_ref, the matrix definition, at fft_tiny and fft_enh, on lengths that torch refuses too; and
    against torch.stft in float64 at fft_sep."""
    import torch
    rng = np.random.default_rng(4096)
    for name in ("fft_tiny", "fft_enh"):
        rec = fft_of(pkg, name, power=None, log=None, floor=0.0)
        H, N = int(rec["hop"][0]), int(rec["n_fft"][0])
        for n, scale in ((1, 1.0), (H + 1, 2.0 ** -15), (N // 2, 2.0 ** -15), (N, 1.0), (7 * H + 5, 2.0 ** -15), (40 * H, -3.7e-3)):
            y = rng.integers(-32768, 32768, n, dtype=np.int16)
            x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
            got, S = fft_ref(y, scale, rec)
            want, S2 = stft_ref(y, scale, rec)
            assert got.shape == want.shape == (frame_count(rec, n), N // 2 + 1) and got.dtype == np.complex128
            err = max(np.abs((got - want).real).max(), np.abs((got - want).imag).max())
            print(name, n, "max |d| vs stft_ref", err, "bound", _bound(rec, x))
            assert err <= _bound(rec, x) and np.abs(S - S2).max() <= 2 * _bound(rec, x)
        for full in (fft_of(pkg, name), fft_of(pkg, name, power=1, log="log10", floor=1e-9)):  # the outputs are finish()'s
            y = rng.integers(-32768, 32768, 9 * H, dtype=np.int16)
            a, b = fft_ref(y, 2.0 ** -15, full)[0], stft_ref(y, 2.0 ** -15, full)[0]
            assert a.shape == b.shape and np.allclose(a, b, rtol=1e-9, atol=1e-9)
    sr, n_fft, win, hop = SETS["fft_sep"][:4]
    rec = fft_of(pkg, "fft_sep")
    window = torch.hann_window(win, periodic=True, dtype=torch.float64)
    for n, scale in ((n_fft // 2 + 1, 2.0 ** -15), (n_fft, 1.0), (7 * hop + 5, 2.0 ** -15), (20 * hop, -3.7e-3)):
        y = rng.integers(-32768, 32768, n, dtype=np.int16)
        x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
        want = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, win_length=win, window=window, center=True, pad_mode="reflect",
                          return_complex=True).numpy().T
        got, _ = fft_ref(y, scale, rec)
        assert got.shape == want.shape == (n // hop + 1, n_fft // 2 + 1)
        err = max(np.abs((got - want).real).max(), np.abs((got - want).imag).max())
        print("fft_sep", n, "max |d| vs torch.stft", err, "bound", _bound(rec, x))
        assert err <= _bound(rec, x)
        if len(got) > 1:
            assert np.abs(got.imag).max() > 1e3 * _bound(rec, x)  # the sign of Im is seen
    zero, _ = fft_ref(np.zeros(5000, dtype=np.int16), -1.0, rec)
    assert zero.shape == (5, 2049) and (zero == 0).all()


def test_yardstick(pkg):
    """The yardstick of the GPU test's tolerance per set: the largest error of fft_f32 against fft_ref over the kept cells of
    crafted_tracks; and, from fft_ref alone, that at most 1 % of a set's cells are not kept.  A float32 FFT is off by about
    log2(n_fft) 2^-24 of the frame's largest magnitude in Re and Im, which is the pairs' measure; a kept real cell may lie 1e-4 of
    that magnitude up, so its relative error may reach 1e4 times as much."""
    for name in SETS:
        worst, cells, dropped = yardstick(pkg, name)
        n_fft, power = SETS[name][1], SETS[name][4]
        fft = np.log2(n_fft) * 2.0 ** -24
        print(f"{name}: float32 radix-2 FFT, max error {worst:.3g} over {cells - dropped} kept cells of {cells}, "
              f"{100.0 * dropped / cells:.4f} % not kept")
        assert cells > 500 and dropped <= 0.01 * cells, name
        assert 0 < worst < (4 * fft if power is None else 2 * 1e4 * fft), name


# ---- layout -------------------------------------------------------------------------------------------------
def test_layout_at_the_new_widths(pkg):
    planned = np.array([0, 1, 479, 480, 481, 3 * 160 * 64, 0, 7, 48000 * 3 + 5], dtype=np.int64)
    for name, up, down in (("fft_sep", 147, 160), ("fft_big", 1, 1)):
        for layout in ("bands", "frames"):
            for power in (None, 2):
                rec = fft_of(pkg, name, layout, power=power, log=None, floor=0.0)
                bins, hop, c = int(rec["n_fft"][0]) // 2 + 1, int(rec["hop"][0]), 2 if power is None else 1
                assert bins == {"fft_sep": 2049, "fft_big": 4097}[name]
                n = -(-planned * up // down)
                F = n // hop if name == "fft_big" else np.where(n > 0, n // hop + 1, 0)
                plane = (F + 63) // 64 * 64
                offs, planes, total = pkg.stft_layout(planned, up, down, rec)
                want = np.concatenate([[0], np.cumsum(bins * c * plane)])
                assert np.array_equal(planes, plane) and np.array_equal(offs, want[:-1]) and total == want[-1] and (offs % 64 == 0).all()
                assert np.array_equal(pkg.stft_frames(rec, n), F) and pkg.stft_width(rec) == bins * c


# ---- refusals before any device work ------------------------------------------------------------------------
def test_batches_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """STFT BATCHES above 1025 bins (an fft_sep record) and a feature-batch request with any FFT record: OPUSGPU_BAD_ARG from both
    kinds of decoder with NULL buffers, the existing reasons in the decoder's message, the caller's arrays untouched; and ValueError
    from files_request and from decode_files on an object without a decoder."""
    lib = pkg.load_lib()
    sep, vits = fft_of(pkg, "fft_sep"), fft_of(pkg, "fft_vits")
    enh = fft_of(pkg, "fft_enh")
    mix2, mix6 = pkg.mix_matrix("mono", 2), pkg.mix_matrix("mono", 6)
    for b, prefix, h, sep_args, enh_args in ((batch, "opusgpu_", handles[0], (0, 147, 160, 0, mix2.ctypes.data), (16000, 0, 0, 1, None)),
                                             (ms_batch, "opusgpu_ms_", handles[1], (0, 147, 160, mix6.ctypes.data), (16000, 0, 0, mix6.ctypes.data))):
        setter, err, call = getattr(lib, prefix + "set_stft_batch"), getattr(lib, prefix + "last_error"), getattr(lib, prefix + "files_decode_stft")
        arrays = [np.full(b.n_files, -7, dtype=np.int64) for _ in range(3)] + [np.full((b.n_files, 2), -7, dtype=np.int32)]
        tail = [a.ctypes.data for a in arrays]
        try:
            req = good_request(pkg, norm=0, stride_frames=4096)
            assert setter(h, req.ctypes.data, None, None, 0) == 0
            assert call(h, b.h, *sep_args, sep.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            assert b"1 - 1025" in err(h)
            assert setter(h, None, None, None, 0) == 0
            fb = pkg.feature_batch_request([10], 80, feature_stride=3000)
            assert getattr(lib, prefix + "set_feature_batch")(h, fb.rec.ctypes.data, None, None, 80) == 0
            try:
                for args, rec in ((enh_args, enh), (sep_args, sep)):
                    assert call(h, b.h, *args, rec.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
                    assert b"not batched" in err(h)
            finally:
                assert getattr(lib, prefix + "set_feature_batch")(h, None, None, None, 0) == 0
        finally:
            assert setter(h, None, None, None, 0) == 0
        assert all((a == -7).all() for a in arrays)
    how = dict(resample=44100, mono=True)
    assert pkg.files_request(batch, features=sep, **how).entry == "files_decode_stft"
    assert np.array_equal(pkg.files_request(batch, features=sep, **how).params, sep)  # the record carries the choice
    assert pkg.files_request(batch, features=vits, resample=22050, mono=True, stft_stride=256).stft_batch.bins == 513
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for kw in (dict(stft_stride=64), dict(stft_stride=4096), dict(stft_normalize="refmax"), dict(stft_pad=0.0)):
        with pytest.raises(ValueError, match="1025"):
            pkg.files_request(batch, features=sep, **how, **kw)
        with pytest.raises(ValueError, match="1025"):
            ctx.decode_files(None, batch=batch, features=sep, **how, **kw)
    for rec, rate in ((sep, dict(resample=44100)), (enh, dict(rate=16000)), (fft_of(pkg, "fft_tiny"), dict(resample=8000))):
        for kw in (dict(feature_stride=3000), dict(normalize="cmn"), dict(feature_pad=0.0)):
            with pytest.raises(ValueError, match="1 - 128"):
                pkg.files_request(batch, features=rec, mono=True, **rate, **kw)
            with pytest.raises(ValueError, match="1 - 128"):
                ctx.decode_files(None, batch=batch, features=rec, mono=True, **rate, **kw)


# ---- the kernel's resources ---------------------------------------------------------------------------------
def test_kernel_resources():
    """k_tracks_fft, both instantiations (bins-major and frames-major): no scratch, no static LDS (a launch asks for its frames'
    buffers alone, 33,792 bytes at most) and at most 256 registers; and k_tracks_stft's two are still the only ones its own test
    matches."""
    meta = _kernel_metadata()
    seen = {mangled: v for mangled, v in meta.items() if re.search(r"\d+k_tracks_fftILb[01]EE", mangled)}
    print(seen)
    assert len(seen) == 2, sorted(meta)[:6]
    for vgpr, scratch, lds in seen.values():
        assert vgpr <= 256 and scratch == 0 and lds == 0
    assert len([m for m in meta if re.search(r"\d+k_tracks_stftILb[01]EE", m)]) == 2
