"""Linear and complex STFT spectrograms of the whole-file path (include/opusgpu.h, TRACK STFT), what needs no GPU: the exported
symbols and the record, the float64 restatement of the header's definition against torch.stft and against values worked out by
hand where torch refuses the input, the tables, the layout helper, the refusals that the C calls and decode_files raise before any
device work, the yardstick of the GPU test's tolerance, and the kernel's resources.  stft_ref is the float64 numpy restatement that
the GPU checks (tests/test_gpu_tracks_stft.py) compare against; stft_f32 is the same in float32 with the library's tables, the
yardstick their tolerance is taken from; crafted_tracks are the tracks both are measured on."""
import functools
import os
import re
import zlib

import numpy as np
import pytest

from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_stft_basis", "opusgpu_stft_tile", "opusgpu_stft_layout", "opusgpu_tracks_stft_device", "opusgpu_files_decode_stft",
       "opusgpu_ms_files_decode_stft"]
# (sr, n_fft, win, hop, power (None: complex), log, floor, frames): the smallest sets that reach each path of k_tracks_stft
SETS = {
    "tiny": (8000, 64, 48, 24, 2, "ln", 1e-10, "torch"),            # 33 bins: a full block plus the Nyquist bin alone; hop no multiple of 8; win < n_fft
    "enh": (16000, 512, 400, 128, None, None, 0.0, "torch"),        # pairs; frames-major rows of 257 pairs
    "vits": (22050, 1024, 1024, 256, 1, None, 0.0, "torch"),        # 513 bins, magnitude, floor 0
    "wide": (44100, 2048, 2048, 960, 2, "log10", 1e-10, "torch"),   # 1025 bins, 33 blocks, a window of 31,808 samples
    "whisper_lin": (16000, 400, 400, 160, 2, None, 0.0, "whisper"),  # 201 bins; the DFT of k_tracks_melspec's whisper set
}
# the tile each must hit: the largest of 128, 64, 32 frames with (T - 1) hop + n_fft <= 32768 (opusgpu_stft_tile)
TILES = {"tiny": 128, "enh": 128, "vits": 64, "wide": 32, "whisper_lin": 128}
# the layouts each is run in on the GPU ("wide" in both: its rows of 1025 bins are the longest unaligned ones)
LAYOUTS = {"tiny": ("bands", "frames"), "enh": ("bands", "frames"), "vits": ("bands",), "wide": ("bands", "frames"), "whisper_lin": ("bands",)}


def stft_of(pkg, name, feature_layout="bands", **kw):
    sr, n_fft, win, hop, power, log, floor, frames = SETS[name]
    args = dict(win_length=win, power=power, log=log, floor=floor, frames=frames, feature_layout=feature_layout)
    args.update(kw)
    return pkg.stft_spec(sr, n_fft, hop, **args)


def tile_of(rec):
    hop, n_fft = int(rec["hop"][0]), int(rec["n_fft"][0])
    return next(T for T in (128, 64, 32) if (T - 1) * hop + n_fft <= 32768 or T == 32)


# ---- the header's definition, in float64 --------------------------------------------------------------------
def basis64(rec):
    """(Wc, Ws) [n_fft, n_fft / 2 + 1] in float64: w[i] cos(a), w[i] sin(a), a = 2 pi ((i k) mod n_fft) / n_fft."""
    n_fft, win = int(rec["n_fft"][0]), int(rec["win_length"][0]) or int(rec["n_fft"][0])
    left = (n_fft - win) // 2
    i, k = np.arange(n_fft)[:, None], np.arange(n_fft // 2 + 1)[None, :]
    inside = (i >= left) & (i < left + win)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (i - left) / float(win))
    a = 2.0 * np.pi * ((i * k) % n_fft) / float(n_fft)
    return np.where(inside, w * np.cos(a), 0.0), np.where(inside, w * np.sin(a), 0.0)


@functools.lru_cache(maxsize=None)
def _basis64(n_fft, win):
    rec = np.zeros(1, dtype=[("n_fft", "<i4"), ("win_length", "<i4")])
    rec["n_fft"], rec["win_length"] = n_fft, win
    return basis64(rec)


def frame_count(rec, n):
    hop = int(rec["hop"][0])
    return n // hop if int(rec["frames"][0]) == 1 else (n // hop + 1 if n else 0)


def frames_of(y, rec):
    """The windows of TRACK STFT: y [n] -> (q [F, n_fft] reflected indices clipped into [0, n), inside [F, n_fft] bool)."""
    n, hop, n_fft = len(y), int(rec["hop"][0]), int(rec["n_fft"][0])
    F = frame_count(rec, n)
    q = hop * np.arange(F)[:, None] - n_fft // 2 + np.arange(n_fft)[None, :]
    q = np.where(q < 0, -q, np.where(q >= n, 2 * (n - 1) - q, q))  # reflected ONCE
    inside = (q >= 0) & (q < n)
    return np.clip(q, 0, max(n - 1, 0)), inside


def finish(re, im, rec):
    """OUTPUT of TRACK STFT from Re and Im [F, bins], in their dtype -> (output, S): S is what the floor is held against (the
    magnitude for pairs, which have no floor)."""
    power, log = int(rec["power"][0]), int(rec["log"][0])
    S = re * re + im * im
    if power == 0:
        return re + 1j * im if re.dtype == np.float64 else (re + 1j * im).astype(np.complex64), np.sqrt(S)
    if power == 1:
        S = np.sqrt(S)
    v = np.maximum(S, rec["floor"][0].astype(re.dtype))
    with np.errstate(divide="ignore"):
        return (v if log == 0 else np.log10(v) if log == 1 else np.log(v)), S


def stft_ref(y, scale, rec):
    """TRACK STFT in float64: y int16 [n] -> (output [F, bins] float64 or complex128, S [F, bins]).  The sample is the float32
    product (float)y * scale, as the header says; everything behind it is float64 with float64 tables.  Im = -sum Ws x."""
    y = np.asarray(y, dtype=np.int16)
    wc, ws = _basis64(int(rec["n_fft"][0]), int(rec["win_length"][0]) or int(rec["n_fft"][0]))
    q, inside = frames_of(y, rec)
    x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
    fr = np.where(inside, x[q] if len(y) else 0.0, 0.0)
    return finish(fr @ wc, -(fr @ ws), rec)


def stft_f32(y, scale, rec, wc, ws):
    """The same value in float32 throughout, with the library's float32 tables, summed in numpy's order: the yardstick for the
    kernel's tolerance (the kernel may differ from float64 by 8 x what this does)."""
    y = np.asarray(y, dtype=np.int16)
    q, inside = frames_of(y, rec)
    x = y.astype(np.float32) * np.float32(scale)
    fr = np.where(inside, x[q] if len(y) else np.float32(0), np.float32(0)).astype(np.float32)
    re, im = fr @ wc, -(fr @ ws)
    assert re.dtype == im.dtype == np.float32
    out = finish(re, im, rec)[0]
    assert out.dtype == (np.complex64 if int(rec["power"][0]) == 0 else np.float32)
    return out


def error_of(got, ref, S, rec):
    """The error the tolerance is held on, [F, bins]: log outputs, the absolute difference; linear real outputs, the relative one
    (absolute where the reference is 0); pairs, the larger of |d Re| and |d Im| over the frame's largest float64 magnitude."""
    if int(rec["power"][0]) == 0:
        d = np.asarray(got, dtype=np.complex128) - ref
        top = S.max(axis=1, keepdims=True) if S.size else S
        return np.maximum(np.abs(d.real), np.abs(d.imag)) / np.where(top == 0, 1.0, top)
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return d if int(rec["log"][0]) else d / np.where(ref == 0, 1.0, np.abs(ref))


def kept_cells(S, rec):
    """The cells the tolerance is held on: every pair; of real outputs, float64 S at least 1e-8 x its frame's largest."""
    if int(rec["power"][0]) == 0 or not S.size:
        return np.ones(S.shape, dtype=bool)
    return S >= 1e-8 * S.max(axis=1, keepdims=True)


# ---- the tracks the tolerance is measured on ----------------------------------------------------------------
def lengths_of(rec):
    """Every length at which the kernel changes path, for the record's hop H, n_fft N and tile T."""
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
    finite one --, an all-zero track and a track of +-40 noise."""
    rng = np.random.default_rng(zlib.crc32(("stft " + name).encode()))
    rec = stft_of(_PKG[0], name)
    H = int(rec["hop"][0])
    tracks, scales = [], []
    for n in lengths_of(rec):
        for k in range(2):
            tracks.append(rng.integers(-32768, 32768, n, dtype=np.int16))
            scales.append(2.0 ** -15 if k == 0 else float(rng.choice([-1, 1]) * rng.uniform(1, 10) * 10.0 ** rng.integers(-6, 3)))
    tracks.append(np.zeros(H * 5 + 3, dtype=np.int16))
    scales.append(-2.0 ** -15)  # a negative scale: the zero track's cells must still be +0
    tracks.append(rng.integers(-40, 41, H * 9 + 77, dtype=np.int16))
    scales.append(2.0 ** -15)
    scales = np.asarray(scales, dtype=np.float32)
    assert np.isfinite(scales).all() and (scales != 0).all()
    return tracks, scales


@functools.lru_cache(maxsize=None)
def crafted_reference(name):
    """stft_ref of crafted_tracks: [(output [F, bins], S [F, bins])], computed once per set and shared."""
    tracks, scales = crafted_tracks(name)
    rec = stft_of(_PKG[0], name)
    refs = [stft_ref(y, s, rec) for y, s in zip(tracks, scales)]
    for out, S in refs:
        out.setflags(write=False), S.setflags(write=False)
    return refs


def yardstick(pkg, name):
    """-> (the largest error of stft_f32 against stft_ref over the kept cells of crafted_tracks, cells, cells not kept)."""
    tracks, scales = crafted_tracks(name)
    rec = stft_of(pkg, name)
    wc, ws = pkg.stft_basis(rec)
    worst, cells, dropped = 0.0, 0, 0
    for y, s, (ref, S) in zip(tracks, scales, crafted_reference(name)):
        if len(ref):
            keep = kept_cells(S, rec)
            cells, dropped = cells + keep.size, dropped + int((~keep).sum())
            worst = max(worst, float(error_of(stft_f32(y, s, rec, wc, ws), ref, S, rec)[keep].max(initial=0)))
    return worst, cells, dropped


# ---- symbols, record, tables --------------------------------------------------------------------------------
def test_symbols_and_record(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "TRACK STFT" in hdr and "opusgpu_stft_params { /* 64 bytes" in hdr and re.search(r"#define OPUSGPU_STFT_COMPLEX 0\b", hdr)
    d = pkg.STFT_PARAMS_DTYPE
    assert d.itemsize == 64  # sizeof(opusgpu_stft_params), which the library holds with a static_assert
    names = ["sample_rate", "n_fft", "win_length", "hop", "power", "log", "frames", "layout", "floor", "reserved"]
    assert [(n, d.fields[n][1]) for n in d.names] == [(n, 4 * i) for i, n in enumerate(names)]
    assert d.fields["reserved"][0].shape == (7,) and d.fields["floor"][0] == np.float32
    # the struct in the header, field by field: 9 words and 7 reserved ones
    body = re.search(r"typedef struct opusgpu_stft_params \{(.*?)\} opusgpu_stft_params;", hdr, re.S).group(1)
    assert re.findall(r"(?:int32_t|float) (\w+)(?:\[(\d)\])?;", body) == [(n, "") for n in names[:9]] + [("reserved", "7")]
    rec = stft_of(pkg, "tiny", "frames")
    assert [int(rec[n][0]) for n in names[:8]] == [8000, 64, 48, 24, 2, 2, 0, 1] and rec["floor"][0] == np.float32(1e-10)
    enh = stft_of(pkg, "enh")
    assert (int(enh["power"][0]), int(enh["log"][0]), float(enh["floor"][0])) == (pkg.STFT_COMPLEX, 0, 0.0)
    assert int(pkg.stft_spec(44100, 1024, 256)["win_length"][0]) == 1024 and int(pkg.stft_spec(44100, 1024, 256)["power"][0]) == 2
    assert {n: tile_of(stft_of(pkg, n)) for n in TILES} == TILES == {n: pkg.stft_tile(stft_of(pkg, n)) for n in TILES}
    assert pkg.stft_tile(stft_of(pkg, "wide", "frames")) == 32  # the layout does not move the tile: there is no store area
    assert [pkg.stft_width(stft_of(pkg, n)) for n in SETS] == [33, 514, 513, 1025, 201]


@pytest.mark.parametrize("name", list(SETS))
def test_basis_is_the_spectrogram_basis(pkg, name):
    """opusgpu_stft_basis hands out opusgpu_spec_basis' tables bit for bit, which are the header's formulas rounded once."""
    rec = stft_of(pkg, name)
    sr, n_fft, win, hop = SETS[name][:4]
    wc, ws = pkg.stft_basis(rec)
    mc, ms = pkg.spec_basis(pkg.mel_spec(sr, n_fft, hop, win, n_mels=20))
    assert wc.dtype == ws.dtype == np.float32 and wc.shape == ws.shape == (n_fft, n_fft // 2 + 1)
    assert np.array_equal(wc.view(np.uint32), mc.view(np.uint32)) and np.array_equal(ws.view(np.uint32), ms.view(np.uint32))
    want_c, want_s = basis64(rec)
    assert np.array_equal(wc.view(np.uint32), want_c.astype(np.float32).view(np.uint32))
    assert np.array_equal(ws.view(np.uint32), want_s.astype(np.float32).view(np.uint32))
    zero_win = rec.copy()
    zero_win["win_length"] = 0 if win == n_fft else win  # the C record's "0 means n_fft"
    assert np.array_equal(pkg.stft_basis(zero_win)[0].view(np.uint32), wc.view(np.uint32))
    assert pkg.load_lib().opusgpu_stft_basis(rec.ctypes.data, None, None) == wc.size
    assert (ws[:, 0] == 0).all() and np.abs(ws[:, -1]).max() < 2e-16  # Im of bins 0 and n_fft / 2: 0, and sin(pi) as a double has it


# ---- the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_reference_is_torch_stft(pkg, name):
    """stft_ref's pairs against torch.stft(center=True, pad_mode="reflect", window=hann_window(win, periodic=True)) in float64 on the
    CPU, for tracks with n > n_fft / 2 (torch refuses the others).  Both are float64 sums of the same n_fft products per cell in
    different orders, so the bound is set by double rounding alone: a sum of n_fft terms is off by at most n_fft * 2^-53 * sum |terms|
    in either order, the terms are w[i] x[i] with sum w = win / 2, and the tables' own rounding is one more 2^-53 each:
    |d| <= 4 * n_fft * 2^-53 * (win / 2) * max |x| holds both differences with room.  Magnitude, power and the logs follow from the
    pairs by the header's formulas in float64, which finish() is."""
    import torch
    sr, n_fft, win, hop = SETS[name][:4]
    rec = stft_of(pkg, name, power=None, log=None, floor=0.0)
    rng = np.random.default_rng(n_fft)
    window = torch.hann_window(win, periodic=True, dtype=torch.float64)
    for n, scale in ((n_fft // 2 + 1, 2.0 ** -15), (n_fft, 1.0), (7 * hop + 5, 2.0 ** -15), (40 * hop, -3.7e-3)):
        y = rng.integers(-32768, 32768, n, dtype=np.int16)
        x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
        want = torch.stft(torch.from_numpy(x), n_fft, hop_length=hop, win_length=win, window=window, center=True, pad_mode="reflect",
                          return_complex=True).numpy().T  # [n // hop + 1, bins]
        got, S = stft_ref(y, scale, rec)
        assert got.shape == (frame_count(rec, n), n_fft // 2 + 1) and got.dtype == np.complex128
        want = want[:len(got)]  # Whisper's count drops the last frame
        bound = 4 * n_fft * 2.0 ** -53 * (win / 2) * np.abs(x).max()
        err = max(np.abs((got - want).real).max(), np.abs((got - want).imag).max())
        print(name, n, "max |d| vs torch.stft", err, "bound", bound)
        assert err <= bound
        if len(got) > 1:  # (frame 0 alone is a window reflected about its middle: its Im is 0)
            assert np.abs(got.imag).max() > 1e3 * bound  # the sign of Im is seen: -Im would be off by twice that


def _by_hand(y, scale, rec, f, k):
    """Re and Im of one cell by the header's sentences, tap by tap."""
    n, N, H = len(y), int(rec["n_fft"][0]), int(rec["hop"][0])
    L = int(rec["win_length"][0]) or N
    left = (N - L) // 2
    re = im = 0.0
    for i in range(N):
        q = H * f - N // 2 + i
        if q < 0:
            q = -q
        elif q >= n:
            q = 2 * (n - 1) - q
        if not 0 <= q < n or not left <= i < left + L:
            continue
        x = float(np.float32(y[q]) * np.float32(scale))
        w = 0.5 - 0.5 * np.cos(2 * np.pi * (i - left) / L)
        a = 2 * np.pi * ((i * k) % N) / N
        re, im = re + w * np.cos(a) * x, im - w * np.sin(a) * x
    return re, im


def test_reference_where_torch_refuses(pkg):
    """n <= n_fft / 2, which torch.stft's reflect padding refuses: the frame counts, the single reflection and the "still outside"
    zero, worked out by hand; and the outputs' floor and logs."""
    tiny, enh, lin = stft_of(pkg, "tiny"), stft_of(pkg, "enh"), stft_of(pkg, "whisper_lin")
    for rec, cases in ((tiny, ((0, 0), (1, 1), (23, 1), (24, 2), (47, 2), (48, 3))), (lin, ((0, 0), (159, 0), (160, 1), (319, 1), (320, 2)))):
        for n, F in cases:
            out, S = stft_ref(np.zeros(n, dtype=np.int16), 1.0, rec)
            assert out.shape == S.shape == (F, int(rec["n_fft"][0]) // 2 + 1)
    # one sample: only tap n_fft / 2 of frame 0 is inside (q = -1 reflects to 1 and q = 1 to -1, both outside): Re[k] = (-1)^k x, Im = 0
    out, _ = stft_ref(np.array([1000], dtype=np.int16), 2.0 ** -15, enh)
    x = 1000 / 32768
    assert out.shape == (1, 257) and np.allclose(out[0].real, x * (-1.0) ** np.arange(257), rtol=0, atol=1e-15) and np.abs(out.imag).max() < 1e-15
    q, inside = frames_of(np.zeros(100, dtype=np.int16), enh)  # one frame, mostly reflections that stay outside
    assert q.shape == (1, 512) and list(q[0, 255:258]) == [1, 0, 1] and not inside[0, :157].any() and inside[0, 157:455].all() and not inside[0, 455:].any()
    rng = np.random.default_rng(7)
    for rec, n in ((tiny, 3), (tiny, 30), (enh, 100), (enh, 256), (lin, 200)):
        y = rng.integers(-32768, 32768, n, dtype=np.int16)
        pairs = rec.copy()
        pairs["power"], pairs["log"] = 0, 0
        out, _ = stft_ref(y, 2.0 ** -15, pairs)
        bins = out.shape[1]
        for f, k in ((0, 0), (0, 1), (0, bins - 1), (len(out) - 1, bins // 2), (len(out) - 1, bins - 2)):
            re, im = _by_hand(y, 2.0 ** -15, rec, f, k)
            assert abs(out[f, k].real - re) <= 1e-12 and abs(out[f, k].imag - im) <= 1e-12, (n, f, k)
        assert np.abs(out[:, [0, -1]].imag).max() <= 1e-12  # bins 0 and n_fft / 2 are real
    # the outputs: floor and log on top of the pairs
    y = rng.integers(-32768, 32768, 500, dtype=np.int16)
    pairs = tiny.copy()
    pairs["power"], pairs["log"] = 0, 0
    c, mag = stft_ref(y, 2.0 ** -15, pairs)
    out, S = stft_ref(y, 2.0 ** -15, tiny)
    assert np.allclose(S, np.abs(c) ** 2, rtol=1e-14) and np.array_equal(out, np.log(np.maximum(S, float(tiny["floor"][0])))) and np.allclose(mag, np.abs(c))
    m, S1 = stft_ref(y, 2.0 ** -15, stft_of(pkg, "tiny", power=1, log="log10"))
    assert np.allclose(S1, np.abs(c), rtol=1e-14) and np.array_equal(m, np.log10(np.maximum(S1, float(tiny["floor"][0]))))
    zero, _ = stft_ref(np.zeros(200, dtype=np.int16), 1.0, tiny)
    assert (zero == np.log(float(np.float32(1e-10)))).all()
    zero, _ = stft_ref(np.zeros(2000, dtype=np.int16), -1.0, enh)
    assert zero.shape == (16, 257) and (zero == 0).all()


def test_yardstick(pkg):
    """The yardstick of the GPU test's tolerance per set: the largest error of stft_f32 against stft_ref over the kept cells of
    crafted_tracks, and that at most 1 % of a set's cells go unkept (uniform noise has a flat spectrum).  What a float32 DFT can be
    off by: Re and Im by about sqrt(n_fft) 2^-24 of the frame's largest magnitude, which is the pairs' measure itself; a kept real
    cell may lie 1e-4 of that magnitude (1e-8 in power) up, so its relative error may reach 1e4 times as much -- 2.7e-2 of the
    magnitude at n_fft 2048, twice that in power, 0.023 in log10 and 0.054 in ln.  Rare cells near the threshold set the figure."""
    for name in SETS:
        worst, cells, dropped = yardstick(pkg, name)
        n_fft, power = SETS[name][1], SETS[name][4]
        dft = np.sqrt(n_fft) * 2.0 ** -24
        print(f"{name}: float32 restatement, max error {worst:.3g} over {cells - dropped} kept cells of {cells}")
        assert cells > 500 and dropped <= 0.01 * cells, name
        assert 0 < worst < (4 * dft if power is None else 2 * 1e4 * dft), name


# ---- layout -------------------------------------------------------------------------------------------------
def test_layout_helper(pkg):
    planned = np.array([0, 1, 479, 480, 481, 3 * 160 * 64, 3 * 160 * 64 - 3, 0, 7, 48000 * 3 + 5], dtype=np.int64)
    for name, up, down in (("tiny", 1, 6), ("enh", 1, 3), ("vits", 147, 320), ("wide", 147, 160), ("whisper_lin", 1, 3)):
        for layout in ("bands", "frames"):
            rec = stft_of(pkg, name, layout)
            bins, hop, c = int(rec["n_fft"][0]) // 2 + 1, int(rec["hop"][0]), 2 if name == "enh" else 1
            n = -(-planned * up // down)
            F = n // hop if name == "whisper_lin" else np.where(n > 0, n // hop + 1, 0)
            plane = (F + 63) // 64 * 64
            offs, planes, total = pkg.stft_layout(planned, up, down, rec)
            want = np.concatenate([[0], np.cumsum(bins * c * plane)])
            assert np.array_equal(planes, plane) and np.array_equal(offs, want[:-1]) and total == want[-1] and (offs % 64 == 0).all()
            assert np.array_equal(pkg.stft_frames(rec, n), F) and pkg.stft_width(rec) == bins * c
    torch_rec, whisper_rec = (pkg.stft_spec(16000, 400, 160, frames=f) for f in ("torch", "whisper"))
    n = np.array([0, 1, 159, 160, 161, 16000], dtype=np.int64)
    assert list(pkg.stft_frames(whisper_rec, n)) == [0, 0, 0, 1, 1, 100] and list(pkg.stft_frames(torch_rec, n)) == [0, 1, 1, 2, 2, 101]
    assert np.array_equal(pkg.stft_layout(planned, 1, 3, whisper_rec)[1], pkg.mel_layout(planned, 80, "bands")[1])  # TRACK FEATURES' planes
    offs, planes, total = pkg.stft_layout([], 1, 3, torch_rec)
    assert len(offs) == 0 and total == 0
    lib = pkg.load_lib()
    BAD = pkg.OPUSGPU_BAD_ARG
    ok = torch_rec.ctypes.data
    assert lib.opusgpu_stft_layout(planned.size, planned.ctypes.data, 1, 3, ok, None) == pkg.stft_layout(planned, 1, 3, torch_rec)[2]
    for up, down in ((0, 3), (3, 1), (1, 0), (-1, 3), (1, 48001)):
        assert lib.opusgpu_stft_layout(planned.size, planned.ctypes.data, up, down, ok, None) == BAD
    assert lib.opusgpu_stft_layout(2, planned.ctypes.data, 1, 3, None, None) == BAD and lib.opusgpu_stft_layout(-1, planned.ctypes.data, 1, 3, ok, None) == BAD
    assert lib.opusgpu_stft_layout(2, None, 1, 3, ok, None) == BAD
    with pytest.raises(ValueError):
        pkg.stft_layout([5, -1], 1, 3, torch_rec)
    with pytest.raises(ValueError):
        pkg.stft_layout(planned, 1, 3, pkg.mel_spec(16000, 400, 160))  # TRACK SPECTROGRAMS' record is another record


# ---- refusals before any device work ------------------------------------------------------------------------
def bad_records(pkg):
    """Records that break one rule of opusgpu_stft_params each."""
    good = pkg.stft_spec(16000, 512, 128, 400, power=2, log="ln", floor=1e-7)

    def but(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    return good, [but(n_fft=48), but(n_fft=2064), but(n_fft=520), but(n_fft=4096), but(win_length=14), but(win_length=401), but(win_length=514),
                  but(win_length=-2), but(hop=0), but(hop=513), but(hop=-160), but(n_fft=2048, win_length=0, hop=991), but(power=3), but(power=-1),
                  but(power=0), but(power=0, log=1), but(log=3), but(log=-1), but(frames=2), but(frames=-1), but(layout=2), but(layout=-1),
                  but(floor=0.0), but(floor=-1.0), but(floor=np.inf), but(floor=np.nan), but(log=0, floor=-0.5), but(log=0, floor=np.nan),
                  but(sample_rate=0), but(sample_rate=1048577), but(reserved=[1, 0, 0, 0, 0, 0, 0]), but(reserved=[0, 0, 0, 0, 0, 0, 7])]


def test_stft_spec_refuses(pkg):
    """stft_spec raises for every rule of the record, and the C accessors refuse every record that breaks one."""
    assert int(pkg.stft_spec(32000, 2048, 990)["hop"][0]) == 990  # 31 * 990 + 2048 = 32738
    assert pkg.stft_spec(8000, 64, 24, 48, power=1)["floor"][0] == 0 and int(pkg.stft_spec(8000, 64, 24, power=None)["power"][0]) == 0
    for kw in (dict(n_fft=48), dict(n_fft=520), dict(n_fft=4096), dict(n_fft=512.0), dict(win_length=14), dict(win_length=401), dict(win_length=600),
               dict(win_length=400.0), dict(hop=0), dict(hop=513), dict(hop=128.0), dict(n_fft=2048, hop=991), dict(power=3), dict(power=0),
               dict(power=2.5), dict(power=True), dict(power="complex"), dict(log="log2"), dict(log=1), dict(power=None, log="log10"),
               dict(power=None, log="ln", floor=1e-5), dict(frames="librosa"), dict(frames=0), dict(feature_layout="planar"),
               dict(feature_layout=1), dict(log="ln"), dict(log="log10", floor=0), dict(floor=-1), dict(floor=float("inf")),
               dict(floor=float("nan")), dict(floor="x"), dict(sample_rate=0), dict(sample_rate=1048577), dict(sample_rate=16000.0)):
        args = {"sample_rate": 16000, "n_fft": 512, "hop": 128, **kw}
        with pytest.raises(ValueError):
            pkg.stft_spec(**args)
    lib = pkg.load_lib()
    good, bad = bad_records(pkg)
    planned = np.array([480, 960], dtype=np.int64)
    assert lib.opusgpu_stft_basis(good.ctypes.data, None, None) == 512 * 257 and lib.opusgpu_stft_basis(None, None, None) == pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_stft_tile(good.ctypes.data) == 128 and lib.opusgpu_stft_tile(None) == pkg.OPUSGPU_BAD_ARG
    for rec in bad:
        assert lib.opusgpu_stft_basis(rec.ctypes.data, None, None) == pkg.OPUSGPU_BAD_ARG, rec
        assert lib.opusgpu_stft_tile(rec.ctypes.data) == pkg.OPUSGPU_BAD_ARG
        assert lib.opusgpu_stft_layout(2, planned.ctypes.data, 1, 3, rec.ctypes.data, None) == pkg.OPUSGPU_BAD_ARG
        for call in (pkg.stft_basis, pkg.stft_tile, lambda r: pkg.stft_layout(planned, 1, 3, r)):
            with pytest.raises(ValueError):
                call(rec)
    for other in (pkg.mel_spec(16000, 512, 128), pkg.mel_params(80), None, "stft"):
        for call in (pkg.stft_basis, pkg.stft_tile, pkg.stft_width, lambda r: pkg.stft_frames(r, 100)):
            with pytest.raises(ValueError):
                call(other)


def C_VOID(v):
    import ctypes
    return ctypes.c_void_p(v)


def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """Every refusal of the three calls comes back as OPUSGPU_BAD_ARG with d_in / d_out NULL and -- without a device -- from a decoder
    that does not exist (`handles` of tests/test_tracks_resample.py).  A call that got as far as the device would fail otherwise."""
    lib = pkg.load_lib()
    n = batch.n_files
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    good, bad = bad_records(pkg)  # a record for tracks at 16000 Hz
    vits = stft_of(pkg, "vits")
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)
    inf = np.array([np.inf] + [1] * (n - 1), dtype=np.float32)
    mono_mix = pkg.mix_matrix("mono", 2)
    two_rows = pkg.mix_matrix(np.eye(2, dtype=np.int16) * 16384, 2)
    six_mono, six_stereo = pkg.mix_matrix("mono", 6), pkg.mix_matrix("stereo", 6)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]

    def files(rate, up, down, mono, mix, p, scale, ctx=fake, b=batch.h, out=None):
        return lib.opusgpu_files_decode_stft(ctx, b, rate, up, down, mono, None if mix is None else mix.ctypes.data,
                                             None if p is None else p.ctypes.data, None if scale is None else scale.ctypes.data, out,
                                             *[a.ctypes.data for a in arrays])

    def ms_files(rate, up, down, mix, p, scale, ms=fake_ms, b=ms_batch.h):
        return lib.opusgpu_ms_files_decode_stft(ms, b, rate, up, down, None if mix is None else mix.ctypes.data,
                                                None if p is None else p.ctypes.data, None if scale is None else scale.ctypes.data, None,
                                                None, None, None, None)
    assert files(16000, 0, 0, 1, None, good, None, ctx=None) == BAD and files(16000, 0, 0, 1, None, good, None, b=None) == BAD
    assert files(16000, 0, 0, 1, None, None, None) == BAD
    assert ms_files(16000, 0, 0, six_mono, good, None, ms=None) == BAD and ms_files(16000, 0, 0, six_mono, good, None, b=None) == BAD
    assert ms_files(16000, 0, 0, None, good, None) == BAD and ms_files(16000, 0, 0, six_mono, None, None) == BAD
    for p in bad:
        assert files(16000, 0, 0, 1, None, p, None) == BAD and files(0, 1, 3, 0, mono_mix, p, None) == BAD and ms_files(16000, 0, 0, six_mono, p, None) == BAD
    assert files(16000, 0, 0, 0, None, good, None) == BAD      # neither mono nor a mix
    assert files(16000, 0, 0, 1, mono_mix, good, None) == BAD  # both
    assert files(16000, 0, 0, 0, two_rows, good, None) == BAD and ms_files(16000, 0, 0, six_stereo, good, None) == BAD  # a mix of two rows
    assert files(16000, 0, 0, 0, six_mono, good, None) == BAD and ms_files(16000, 0, 0, mono_mix, good, None) == BAD    # a mix for other tracks
    # a sample_rate that is not the track's rate
    assert files(24000, 0, 0, 1, None, good, None) == BAD and files(48000, 0, 0, 1, None, good, None) == BAD and files(0, 1, 2, 1, None, good, None) == BAD
    assert files(0, 147, 320, 1, None, good, None) == BAD and files(16000, 0, 0, 1, None, vits, None) == BAD and ms_files(0, 147, 160, six_mono, vits, None) == BAD
    odd = pkg.stft_spec(6857, 512, 160)  # 48000 / 7 = 6857.14...: a ratio whose rate is no integer
    assert files(0, 1, 7, 1, None, odd, None) == BAD
    # what the rate and ratio calls refuse: unknown rates, a rate together with a ratio, ratios outside TRACK RATIOS
    for rate, up, down in ((44100, 0, 0), (22050, 0, 0), (16000, 1, 3), (16000, 0, 3), (16000, 1, 0), (0, 0, 0), (0, 3, 1), (0, 1, 9), (0, -1, 3), (-16000, 0, 0)):
        assert files(rate, up, down, 1, None, good, None) == BAD and ms_files(rate, up, down, six_mono, good, None) == BAD, (rate, up, down)
    for scale in (nan, inf):
        assert files(16000, 0, 0, 1, None, good, scale) == BAD and files(0, 1, 3, 0, mono_mix, good, scale) == BAD
    assert ms_files(16000, 0, 0, six_mono, good, np.array([np.nan] * ms_batch.n_files, dtype=np.float32)) == BAD
    assert files(16000, 0, 0, 1, None, good, None, out=C_VOID(64)) == BAD  # a d_out off 128 bytes
    assert all((a == -7).all() for a in arrays)  # and the caller's arrays are as they were

    spans = np.zeros(2, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_samples"], spans["scale"], spans["plane"] = 400, 1.0, 64
    spans["in_offset"], spans["out_offset"] = [0, 408], [0, 64 * 257]

    def kernel(s, p, ctx=fake):
        return lib.opusgpu_tracks_stft_device(ctx, len(s), s.ctypes.data, None, None if p is None else p.ctypes.data, None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    assert kernel(spans, good, ctx=None) == BAD and kernel(spans, None) == BAD
    for p in bad:
        assert kernel(spans, p) == BAD
    for s in (but(in_offset=4), but(in_offset=-8), but(in_samples=-1), but(out_offset=32), but(out_offset=-64), but(plane=32),
              but(in_samples=128 * 64), but(scale=np.nan), but(scale=-np.inf), but(reserved=1)):  # 128 * 64 samples: 65 frames in a plane of 64
        assert kernel(s, good) == BAD
    assert kernel(spans, good) == BAD  # these spans are in order: refused for the NULL buffers, still before the device
    none = spans.copy()
    none["in_samples"] = 0
    assert kernel(none, good) == 0 and kernel(spans[:0], good) == 0  # no frame is no error, and no device work
    whisper = good.copy()
    whisper["frames"] = 1
    short = spans.copy()
    short["in_samples"] = [127, 0]
    assert kernel(short, whisper) == 0 and kernel(short, good) == BAD  # F = n / hop + 1 has a frame there


def test_decode_files_refusals_need_no_device(pkg, batch):
    """track_stft_args and files_request, and decode_files raising before it touches its decoder (an object without one is enough to
    see it): feature_stride=, format="s16", neither or both of mono / mix, a record whose rate is not the track's, a log with pairs."""
    enh, vits, wide = stft_of(pkg, "enh"), stft_of(pkg, "vits", "frames"), stft_of(pkg, "wide")
    rec, mrec, scale, offs, planes, total, out, how = pkg.track_stft_args(batch, enh, rate=16000, mono=True)
    assert rec is not enh and np.array_equal(rec, enh) and (mrec, scale, out, how) == (None, None, None, (16000, 0, 0))
    assert total == pkg.stft_layout(batch.info["track_samples"], 1, 3, enh)[2] > 0 and len(offs) == len(planes) == batch.n_files
    assert pkg.track_stft_args(batch, enh, mono=True)[7] == (16000, 0, 0)          # neither: the record's rate is one of TRACK RATES
    assert pkg.track_stft_args(batch, vits, mono=True)[7] == (0, 147, 320)          # or a ratio of TRACK RATIOS
    assert pkg.track_stft_args(batch, wide, resample=(147, 160), mix="mono")[7] == (0, 147, 160)
    assert pkg.track_stft_args(batch, enh, resample=16000, mono=True)[7] == (0, 1, 3)  # the ratio's filter, if asked for
    req = pkg.files_request(batch, features=enh, mono=True)
    assert (req.entry, req.kind, req.channels, req.total) == ("files_decode_stft", "features", 1, total) and req.args[:4] == (16000, 0, 0, 1)
    assert pkg.files_request(batch, features=vits, mix="mono", multistream=True).args[:3] == (0, 147, 320)
    assert pkg.files_request(batch, features=enh, mono=True, loudness=-23.0).loudness is not None
    six = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files, "track_samples": batch.track_samples})()
    assert pkg.track_stft_args(six, vits, mix="mono", allow_mono=False)[1]["in_channels"][0] == 6
    bad = enh.copy()
    bad["log"] = 1  # a log with pairs
    for b, kw in ((batch, dict(rate=24000, mono=True)), (batch, dict(rate=48000, mono=True)), (batch, dict(resample=22050, mono=True)),
                  (batch, dict(rate=16000, resample=16000, mono=True)), (batch, dict(rate=44100, mono=True)), (batch, dict(resample=(3, 1), mono=True)),
                  (batch, dict(format="s16", mono=True)), (batch, dict(format="f32_planar", mono=True)), (batch, dict()), (batch, dict(mix="stereo")),
                  (batch, dict(mix=np.eye(2))), (batch, dict(mix="mono", mono=True)), (six, dict(mono=True)),
                  (six, dict(mono=True, allow_mono=False)), (batch, dict(mono=True, allow_mono=False)), (six, dict(mix="stereo")),
                  (batch, dict(mono=True, scale=[np.nan] * batch.n_files)), (batch, dict(mono=True, scale=np.ones(batch.n_files + 1))),
                  (batch, dict(mono=True, out=Tensor(total - 1))), (batch, dict(mono=True, out=Tensor(total, dtype="torch.int16"))),
                  (batch, dict(mono=True, out=Tensor(total, ptr=4096 + 64))), (batch, dict(mono=True, out=Tensor(total), device=1))):
        with pytest.raises(ValueError):
            pkg.track_stft_args(b, enh, **kw)
    for features in (bad, pkg.mel_spec(16000, 512, 128), pkg.mel_params(80), "logmel", None, np.zeros(2, dtype=pkg.STFT_PARAMS_DTYPE)):
        with pytest.raises(ValueError):
            pkg.track_stft_args(batch, features, mono=True)
    assert pkg.track_stft_args(batch, enh, mono=True, out=Tensor(total))[6] is not None
    for kw in (dict(feature_stride=3000), dict(normalize="cmn"), dict(feature_pad=0.0)):  # feature batches hold widths of 1 - 128
        with pytest.raises(ValueError, match="1 - 128"):
            pkg.files_request(batch, features=enh, mono=True, **kw)
        with pytest.raises(ValueError, match="1 - 128"):
            pkg.files_request(batch, features=stft_of(pkg, "tiny"), mono=True, resample=8000, **kw)  # 33 bins are no exception
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for features, kw in ((enh, dict(rate=24000, mono=True)), (enh, dict(format="s16", mono=True)), (enh, dict(mix=np.eye(2))), (enh, dict()),
                         (enh, dict(mono=True, out=Tensor(total - 1))), (enh, dict(mono=True, mix="mono")), (vits, dict(rate=16000, mono=True)),
                         (vits, dict(resample=44100, mono=True)), (bad, dict(mono=True)), (enh, dict(rate=16000, resample=16000, mono=True)),
                         (enh, dict(mono=True, feature_stride=3000)), (enh, dict(mono=True, normalize="cmvn"))):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, features=features, **kw)
    ms = pkg.MultistreamContext.__new__(pkg.MultistreamContext)
    ms.h, ms.device = None, 0
    for kw in (dict(mix="stereo"), dict(), dict(mix="mono", rate=8000), dict(mix="mono", format="s16"), dict(mix="mono", out=Tensor(3)),
               dict(mix="mono", feature_stride=100)):
        with pytest.raises(ValueError):
            ms.decode_files(None, batch=six, features=enh, **kw)
    # the other records keep their routes
    assert pkg.files_request(batch, features=pkg.mel_spec(16000, 512, 160, 400), mono=True).entry == "files_decode_melspec"
    assert pkg.files_request(batch, features="logmel", mono=True).entry == "files_decode_mel"


def test_kernel_resources():
    """k_tracks_stft, both instantiations (bins-major and frames-major): no scratch (the accumulators are indexed by literals only)
    and no static LDS -- a launch asks for its tile's window alone, at most the 65,536 bytes of the 32,768 samples that the record's
    rules and the tile choice allow (TILES, held in test_symbols_and_record) -- and at most 256 registers, vector and accumulation
    together."""
    meta = _kernel_metadata()
    seen = {mangled: v for mangled, v in meta.items() if re.search(r"\d+k_tracks_stftILb[01]EE", mangled)}
    print(seen)
    assert len(seen) == 2, sorted(meta)[:6]
    for vgpr, scratch, lds in seen.values():
        assert vgpr <= 256 and scratch == 0 and lds == 0
