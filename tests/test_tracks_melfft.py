"""TRACK SPECTROGRAMS by FFT (include/opusgpu.h, TRACK SPECTROGRAMS, OPUSGPU_SPEC_ALGO_FFT), what needs no GPU: the record and its
refusals, the filterbank at the sizes no dense record reaches, the tables it shares with TRACK STFT's FFT records, the float64
reference melfft_ref against the matrix definition (tests/test_tracks_melspec.py::melspec_ref), the float32 yardstick melfft_f32 of
the GPU test's tolerance, the refusals that come before any device work, and the kernels' resources.  melfft_ref is what the GPU
checks (tests/test_gpu_tracks_melfft.py) compare against; crafted_tracks are the tracks both are measured on.  Every test here fails
without the feature: mel_spec has no algo= and the library no opusgpu_spec_fft_tables."""
import functools
import os
import re
import zlib

import numpy as np
import pytest

from test_tracks_fft import fft_f32, window64
from test_tracks_melspec import SETS as DENSE_SETS
from test_tracks_melspec import error_of, filterbank64, frame_count, frames_of, melspec_ref, spec_of
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)
from test_tracks_stft import _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (sr, n_fft, win, hop, n_mels, fmin, fmax, scale, norm, power, log, floor, frames)
SETS = {
    "mf_tiny": (8000, 64, 48, 24, 8, 0, 4000, "htk", None, 1, None, 0, "whisper"),                            # 32 frames in flight, tile 128
    "mf_kaldi": (16000, 512, 400, 160, 80, 20, 8000, "htk", None, 2, "ln", 1.1920929e-7, "torch"),           # 4 in flight
    "mf_tts": (22050, 1024, 1024, 256, 80, 0, 8000, "slaney", "slaney", 1, "ln", 1e-5, "torch"),             # 2 in flight, M = 512 (odd exponent)
    "mf_music": (44100, 2048, 1102, 441, 128, 0, 22050, "slaney", "slaney", 2, "log10", 1e-10, "torch"),     # 1 in flight from here
    "mf_sep": (44100, 4096, 4096, 1024, 128, 0, 22050, "slaney", "slaney", 2, "log10", 1e-10, "torch"),      # first size the dense path refuses
    "mf_big": (48000, 8192, 6000, 1000, 64, 50, 14000, "htk", None, 2, "log10", 1e-10, "whisper"),           # largest size, zero-padded window
}
SMALL = {"mf_tiny": "tiny", "mf_kaldi": "kaldi", "mf_tts": "tts", "mf_music": "music"}  # the dense sets these are, with the word set
TILES = {"mf_tiny": 128, "mf_kaldi": 32, "mf_tts": 32, "mf_music": 32, "mf_sep": 32, "mf_big": 32}  # the larger of 32 and 8192 / n_fft
IN_FLIGHT = {"mf_tiny": 32, "mf_kaldi": 4, "mf_tts": 2, "mf_music": 1, "mf_sep": 1, "mf_big": 1}    # 256 / min(256, n_fft / 8)
# the cells of crafted_tracks' tracks that are not all zero
CELLS = {"mf_tiny": 10000, "mf_kaldi": 28160, "mf_tts": 25600, "mf_music": 42752, "mf_sep": 40960, "mf_big": 21184}
# the largest error of melfft_f32 against melfft_ref on the kept cells of crafted_tracks, measured on a CPU by test_yardstick
YARDSTICK = {"mf_tiny": 7.99e-07, "mf_kaldi": 5.23e-06, "mf_tts": 1.61e-06, "mf_music": 2.92e-06, "mf_sep": 1.48e-06, "mf_big": 2.62e-06}


def mf_of(pkg, name, feature_layout="bands", **kw):
    sr, n_fft, win, hop, n_mels, fmin, fmax, scale, norm, power, log, floor, frames = SETS[name]
    args = dict(win_length=win, n_mels=n_mels, fmin=fmin, fmax=fmax, mel_scale=scale, norm=norm, power=power, log=log, floor=floor,
                frames=frames, feature_layout=feature_layout, algo="fft")
    args.update(kw)
    return pkg.mel_spec(sr, n_fft, hop, **args)


def tile_of(rec):
    return max(32, 8192 // int(rec["n_fft"][0]))


def in_flight(rec):
    return 256 // min(256, int(rec["n_fft"][0]) // 8)


def stft_twin(pkg, rec):
    """The stft_spec(algo="fft") record with the mel record's frames and S: no log, no floor."""
    return pkg.stft_spec(int(rec["sample_rate"][0]), int(rec["n_fft"][0]), int(rec["hop"][0]), int(rec["win_length"][0]) or int(rec["n_fft"][0]),
                         power=int(rec["power"][0]), frames="whisper" if int(rec["frames"][0]) else "torch", algo="fft")


# ---- the reference and the yardstick ------------------------------------------------------------------------
def melfft_ref(y, scale, rec):
    """TRACK SPECTROGRAMS in float64 by numpy's FFT: y int16 [n] -> (output [F, n_mels], mel [F, n_mels]).  Frames by frames_of,
    the sample the float32 product (float)y * scale, the window in double, np.fft.rfft, S, then filterbank64: never the matrix
    basis, which is 537 MB in double at n_fft 8192."""
    y = np.asarray(y, dtype=np.int16)
    q, inside = frames_of(y, rec)
    x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
    fr = np.where(inside, x[q] if len(y) else 0.0, 0.0)
    Z = np.fft.rfft(fr * window64(rec)[None, :], axis=1)
    S = Z.real ** 2 + Z.imag ** 2
    if int(rec["power"][0]) == 1:
        S = np.sqrt(S)
    mel = S @ _bank64(rec).T
    v = np.maximum(mel, float(rec["floor"][0]))
    log = int(rec["log"][0])
    with np.errstate(divide="ignore"):
        return (v if log == 0 else np.log10(v) if log == 1 else np.log(v)), mel


_BANKS = {}


def _bank64(rec):
    key = rec.tobytes()
    if key not in _BANKS:
        _BANKS[key] = filterbank64(rec)
    return _BANKS[key]


def melfft_f32(y, scale, rec, twin, window, twiddle, B):
    """The same value in float32 throughout: tests/test_tracks_fft.py::fft_f32 (a float32 radix-2 FFT with the library's tables)
    with the record's power and no floor -- twin is stft_twin's record --, a float32 product with the library's bank, the floor and
    the log in float32.  The yardstick of the kernel's tolerance (the kernel may differ from float64 by 8 x what this does)."""
    S = fft_f32(y, scale, twin, window, twiddle)
    assert S.dtype == np.float32
    v = np.maximum(S @ np.ascontiguousarray(B.T), rec["floor"][0])
    assert v.dtype == np.float32
    log = int(rec["log"][0])
    with np.errstate(divide="ignore"):
        return v if log == 0 else np.log10(v) if log == 1 else np.log(v)


def kept_cells(mel):
    """The cells the tolerance is held on: float64 mel at least 1e-8 x its frame's largest."""
    return mel >= 1e-8 * mel.max(axis=1, keepdims=True) if mel.size else np.zeros(mel.shape, dtype=bool)


def lengths_of(rec):
    """Every length at which the kernel changes path, for the record's hop H, n_fft N, tile T and frames in flight C."""
    H, N, T, C = int(rec["hop"][0]), int(rec["n_fft"][0]), tile_of(rec), in_flight(rec)
    want = [0, 1, H - 1, H, H + 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1, N, 2 * H - 1, 2 * H, C * H - 1, C * H, C * H + 1,
            T * H - 1, T * H, T * H + 1, T * H + H + 1]
    return list(dict.fromkeys(want))


_PKG = []


@pytest.fixture(autouse=True)
def _keep_pkg(pkg):
    _PKG[:] = [pkg]


@functools.lru_cache(maxsize=None)
def crafted_tracks(name):
    """(tracks, scales), after tests/test_gpu_tracks_melspec.py::crafted_tracks: every length of lengths_of twice, uniform random
    int16 -- once with the default scale, once with a random finite one of either sign --, an all-zero track under a negative scale
    and a track of +-40 noise."""
    rng = np.random.default_rng(zlib.crc32(("melfft " + name).encode()))
    rec = mf_of(_PKG[0], name)
    H = int(rec["hop"][0])
    tracks, scales = [], []
    for n in lengths_of(rec):
        for k in range(2):
            tracks.append(rng.integers(-32768, 32768, n, dtype=np.int16))
            scales.append(2.0 ** -15 if k == 0 else float(rng.choice([-1, 1]) * rng.uniform(1, 10) * 10.0 ** rng.integers(-6, 3)))
    tracks.append(np.zeros(H * 5 + 3, dtype=np.int16))
    scales.append(-2.0 ** -15)  # a negative scale: the zero track's cells must still be the floor's value, +0 for a floor of 0
    tracks.append(rng.integers(-40, 41, H * 9 + 77, dtype=np.int16))
    scales.append(2.0 ** -15)
    scales = np.asarray(scales, dtype=np.float32)
    assert np.isfinite(scales).all() and (scales != 0).all()
    assert max(len(y) for y in tracks) <= 33 * 1024 + 1
    return tracks, scales


@functools.lru_cache(maxsize=None)
def crafted_reference(name):
    """melfft_ref of crafted_tracks: [(output [F, n_mels], mel [F, n_mels])], computed once per set, shared and read-only."""
    tracks, scales = crafted_tracks(name)
    rec = mf_of(_PKG[0], name)
    refs = [melfft_ref(y, s, rec) for y, s in zip(tracks, scales)]
    for out, mel in refs:
        out.setflags(write=False), mel.setflags(write=False)
    return refs


def yardstick(pkg, name):
    """-> (the largest error of melfft_f32 against melfft_ref over the kept cells of crafted_tracks, the cells of the tracks that
    are not all zero, those of them not kept)."""
    tracks, scales = crafted_tracks(name)
    rec = mf_of(pkg, name)
    twin = stft_twin(pkg, rec)
    window, twiddle = pkg.spec_fft_tables(rec)
    B = pkg.spec_filterbank(rec)
    worst, cells, dropped = 0.0, 0, 0
    for y, s, (ref, mel) in zip(tracks, scales, crafted_reference(name)):
        if len(ref):
            keep = kept_cells(mel)
            if y.any():
                cells, dropped = cells + keep.size, dropped + int((~keep).sum())
            worst = max(worst, float(error_of(melfft_f32(y, s, rec, twin, window, twiddle, B), ref, rec)[keep].max(initial=0)))
    return worst, cells, dropped


# ---- record and refusals ------------------------------------------------------------------------------------
def _but(rec, **kw):
    rec = rec.copy()
    for k, v in kw.items():
        rec[k] = v
    return rec


def bad_fft_records(pkg):
    good = pkg.mel_spec(16000, 512, 160, 400, 80, 20.0, 8000.0, "htk", None, 2, "ln", 1e-7, algo="fft")
    return good, [_but(good, n_fft=32, win_length=32, hop=16), _but(good, n_fft=1000), _but(good, n_fft=16384), _but(good, hop=0), _but(good, hop=513),
                  _but(good, reserved=[0, 2]), _but(good, reserved=[1, 1]), _but(good, n_mels=129), _but(good, reserved=[0, -1]),
                  _but(good, win_length=14), _but(good, win_length=514), _but(good, floor=0.0)]


def test_record_and_refusals(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in ("opusgpu_spec_fft_tables", "opusgpu_spec_tile"):
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert re.search(r"#define OPUSGPU_SPEC_ALGO_DENSE 0\b", hdr) and re.search(r"#define OPUSGPU_SPEC_ALGO_FFT 1\b", hdr)
    assert (pkg.SPEC_ALGO_DENSE, pkg.SPEC_ALGO_FFT) == (0, 1) and pkg.SPEC_ALGOS == {"dense": 0, "fft": 1}
    assert pkg.SPEC_PARAMS_DTYPE.itemsize == 64 and "opusgpu_spec_params { /* 64 bytes" in hdr
    BAD = pkg.OPUSGPU_BAD_ARG
    planned = np.array([480, 960], dtype=np.int64)
    # the fields of mel_spec(..., algo="fft")
    rec = mf_of(pkg, "mf_kaldi", "frames")
    names = ["sample_rate", "n_fft", "win_length", "hop", "n_mels", "mel_scale", "norm", "power", "log", "frames", "layout"]
    assert [int(rec[n][0]) for n in names] == [16000, 512, 400, 160, 80, 1, 1, 2, 2, 0, 1] and list(rec["reserved"][0]) == [0, 1]
    assert (float(rec["fmin"][0]), float(rec["fmax"][0]), rec["floor"][0]) == (20.0, 8000.0, np.float32(1.1920929e-7))
    for e in range(6, 14):
        rec = pkg.mel_spec(44100, 1 << e, 1 << (e - 2), algo="fft")
        assert list(rec["reserved"][0]) == [0, 1] and int(rec["n_fft"][0]) == int(rec["win_length"][0]) == 1 << e
        assert pkg.spec_tile(rec) == lib.opusgpu_spec_tile(rec.ctypes.data) == max(32, 8192 >> e) == tile_of(rec)
        assert lib.opusgpu_spec_fft_tables(rec.ctypes.data, None, None) == 1 << e
        assert lib.opusgpu_spec_filterbank(rec.ctypes.data, None) == 80 * ((1 << e) // 2 + 1)
        assert list(pkg.spec_frames(rec, [0, 1, 1 << e])) == [0, 1, 5]
    # algo="dense" is the record without the keyword, byte for byte; the keyword is the last one
    for name in DENSE_SETS:
        sr, n_fft, win, hop, n_mels, fmin, fmax, scale, norm, power, log, floor, frames = DENSE_SETS[name]
        plain = spec_of(pkg, name, "frames")
        assert list(plain["reserved"][0]) == [0, 0]
        assert pkg.mel_spec(sr, n_fft, hop, win, n_mels, fmin, fmax, scale, norm, power, log, floor, frames, "frames", "dense").tobytes() == plain.tobytes()
        assert pkg.mel_spec(sr, n_fft, hop, win, n_mels, fmin, fmax, scale, norm, power, log, floor, frames, "frames", algo="dense").tobytes() == plain.tobytes()
    import inspect
    assert list(inspect.signature(pkg.mel_spec).parameters)[-1] == "algo" and inspect.signature(pkg.mel_spec).parameters["algo"].default == "dense"
    # hop = n_fft = 2048: the dense bound 31 * hop + n_fft <= 32768 does not apply
    assert int(pkg.mel_spec(44100, 2048, 2048, algo="fft")["hop"][0]) == 2048 and int(pkg.mel_spec(48000, 8192, 8192, algo="fft")["hop"][0]) == 8192
    with pytest.raises(ValueError, match="32768"):
        pkg.mel_spec(44100, 2048, 2048)
    with pytest.raises(ValueError, match="multiple of 16"):
        pkg.mel_spec(44100, 4096, 1024)  # without the keyword 4096 stays refused, with today's message
    dense4096 = _but(pkg.mel_spec(44100, 2048, 512), n_fft=4096, win_length=0)
    assert lib.opusgpu_spec_filterbank(dense4096.ctypes.data, None) == BAD and lib.opusgpu_spec_tile(dense4096.ctypes.data) == BAD
    assert {n: pkg.spec_tile(mf_of(pkg, n)) for n in SETS} == TILES == {n: tile_of(mf_of(pkg, n, "frames")) for n in SETS}
    assert {n: in_flight(mf_of(pkg, n)) for n in SETS} == IN_FLIGHT
    for kw, match in ((dict(n_fft=32), "power of two"), (dict(n_fft=1000), "power of two"), (dict(n_fft=16384), "power of two"),
                      (dict(hop=0), r"hop must be in \[1, n_fft\]"), (dict(hop=513), r"hop must be in \[1, n_fft\]"), (dict(n_mels=129), "n_mels"),
                      (dict(algo="x"), "algo"), (dict(algo=1), "algo"), (dict(algo=None), "algo")):
        args = {"sample_rate": 16000, "n_fft": 512, "hop": 128, "algo": "fft", **kw}
        if "n_fft" in kw:
            args["hop"] = 16
        with pytest.raises(ValueError, match=match):
            pkg.mel_spec(**args)
    good, bad = bad_fft_records(pkg)
    assert lib.opusgpu_spec_tile(good.ctypes.data) == 32 and lib.opusgpu_spec_fft_tables(good.ctypes.data, None, None) == 512
    assert lib.opusgpu_spec_filterbank(good.ctypes.data, None) == 80 * 257
    assert lib.opusgpu_spec_layout(2, planned.ctypes.data, 1, 3, good.ctypes.data, None) == pkg.spec_layout(planned, 1, 3, _but(good, reserved=0))[2]
    assert lib.opusgpu_spec_fft_tables(None, None, None) == BAD and lib.opusgpu_spec_tile(None) == BAD
    for rec in bad:
        assert lib.opusgpu_spec_filterbank(rec.ctypes.data, None) == BAD, rec
        assert lib.opusgpu_spec_layout(2, planned.ctypes.data, 1, 3, rec.ctypes.data, None) == BAD, rec
        assert lib.opusgpu_spec_fft_tables(rec.ctypes.data, None, None) == BAD, rec
        assert lib.opusgpu_spec_tile(rec.ctypes.data) == BAD, rec
        assert lib.opusgpu_spec_basis(rec.ctypes.data, None, None) == BAD, rec
        for call in (pkg.spec_tile, pkg.spec_fft_tables, pkg.spec_filterbank, lambda r: pkg.spec_layout(planned, 1, 3, r)):
            with pytest.raises(ValueError):
                call(rec)
    # a dense record has no FFT tables and keeps its tile; an FFT record has no dense basis
    for name, T in (("tts", 64), ("kaldi", 128), ("music", 64), ("tiny", 128), ("whisper", 128)):
        dense = spec_of(pkg, name)
        assert lib.opusgpu_spec_fft_tables(dense.ctypes.data, None, None) == BAD and pkg.spec_tile(dense) == lib.opusgpu_spec_tile(dense.ctypes.data) == T
        with pytest.raises(ValueError):
            pkg.spec_fft_tables(dense)
    assert pkg.spec_tile(pkg.mel_spec(32000, 1024, 1000, 1000, 40, 100, 12000, "htk", "slaney", 1, "log10", 1e-7)) == 32
    for name in SETS:
        rec = mf_of(pkg, name)
        assert lib.opusgpu_spec_basis(rec.ctypes.data, None, None) == BAD
        with pytest.raises(ValueError):
            pkg.spec_basis(rec)


def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """opusgpu_tracks_melspec_device and both whole-file calls with an FFT record that breaks a rule: OPUSGPU_BAD_ARG with NULL
    buffers from a decoder that does not exist, the caller's arrays untouched; a good FFT record passes the record check and is
    refused for what comes next, still before the device."""
    lib = pkg.load_lib()
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    good, bad = bad_fft_records(pkg)  # a record for tracks at 16000 Hz
    six_mono, mono_mix = pkg.mix_matrix("mono", 6), pkg.mix_matrix("mono", 2)
    n = batch.n_files
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]

    def files(rate, up, down, mono, mix, p, out=None):
        return lib.opusgpu_files_decode_melspec(fake, batch.h, rate, up, down, mono, None if mix is None else mix.ctypes.data, p.ctypes.data, None,
                                                out, *[a.ctypes.data for a in arrays])

    def ms_files(rate, up, down, mix, p):
        return lib.opusgpu_ms_files_decode_melspec(fake_ms, ms_batch.h, rate, up, down, mix.ctypes.data, p.ctypes.data, None, None, None, None, None, None)
    for p in bad:
        assert files(16000, 0, 0, 1, None, p) == BAD and files(0, 1, 3, 0, mono_mix, p) == BAD and ms_files(16000, 0, 0, six_mono, p) == BAD
    sep = mf_of(pkg, "mf_sep")
    assert files(16000, 0, 0, 1, None, sep) == BAD and files(0, 147, 320, 1, None, sep) == BAD  # a sample_rate that is not the track's rate
    assert files(16000, 0, 0, 0, None, good) == BAD and files(24000, 0, 0, 1, None, good) == BAD
    import ctypes
    assert files(16000, 0, 0, 1, None, good, out=ctypes.c_void_p(64)) == BAD  # a d_out off 128 bytes
    assert all((a == -7).all() for a in arrays)

    spans = np.zeros(2, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_samples"], spans["scale"], spans["plane"] = 400, 1.0, 64
    spans["in_offset"], spans["out_offset"] = [0, 408], [0, 64 * 80]

    def kernel(s, p):
        return lib.opusgpu_tracks_melspec_device(fake, len(s), s.ctypes.data, None, p.ctypes.data, None, None)
    for p in bad:
        assert kernel(spans, p) == BAD
    for field, v in (("in_offset", 4), ("out_offset", 32), ("plane", 32), ("in_samples", 160 * 64), ("scale", np.nan), ("reserved", 1)):
        s = spans.copy()
        s[field][1] = v
        assert kernel(s, good) == BAD
    assert kernel(spans, good) == BAD  # these spans are in order: refused for the NULL buffers, still before the device
    none = spans.copy()
    none["in_samples"] = 0
    assert kernel(none, good) == 0 and kernel(spans[:0], good) == 0  # no frame is no error, and no device work


def test_decode_files_takes_the_record(pkg, batch):
    """track_spectrogram_args and files_request with an FFT record: the record carries the choice, the grid is spec_layout's, and a
    feature-batch request is shaped as for a dense record (widths of 1 - 128)."""
    sep, tts = mf_of(pkg, "mf_sep"), mf_of(pkg, "mf_tts", "frames")
    rec, mrec, scale, offs, planes, total, out, how = pkg.track_spectrogram_args(batch, sep, resample=44100, mono=True)
    assert np.array_equal(rec, sep) and how == (0, 147, 160) and total == pkg.spec_layout(batch.info["track_samples"], 147, 160, sep)[2] > 0
    assert pkg.track_spectrogram_args(batch, mf_of(pkg, "mf_big"), rate=48000, mono=True)[7] == (48000, 0, 0)
    req = pkg.files_request(batch, features=tts, mono=True)
    assert req.entry == "files_decode_melspec" and np.array_equal(req.params, tts)
    assert pkg.files_request(batch, features=tts, mono=True, feature_stride=3000, normalize="cmvn").entry == "files_decode_melspec"
    with pytest.raises(ValueError):
        pkg.track_spectrogram_args(batch, _but(sep, reserved=[0, 2]), resample=44100, mono=True)
    with pytest.raises(ValueError):
        pkg.track_spectrogram_args(batch, sep, rate=48000, mono=True)  # 44100 is not that rate


# ---- tables -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
def test_tables(pkg, name):
    """The filterbank is the header's formula in double rounded once, at 4096 and 8192 as below; up to 2048 it is the dense record's
    bit for bit; the window and twiddles are stft_fft_tables' for the same n_fft and win_length, bit for bit."""
    rec = mf_of(pkg, name)
    n_fft, n_mels = int(rec["n_fft"][0]), int(rec["n_mels"][0])
    B = pkg.spec_filterbank(rec)
    assert B.dtype == np.float32 and B.shape == (n_mels, n_fft // 2 + 1)
    assert np.array_equal(B.view(np.uint32), filterbank64(rec).astype(np.float32).view(np.uint32))
    assert (B >= 0).all() and (B.max(axis=1) > 0).all()  # no band without a weight
    assert ((B != 0).sum(axis=0) <= 2).all()  # every bin lies under at most two triangles
    if name in SMALL:
        dense = spec_of(pkg, SMALL[name])
        assert _but(rec, reserved=0).tobytes() == dense.tobytes()
        assert np.array_equal(B.view(np.uint32), pkg.spec_filterbank(dense).view(np.uint32))
    else:
        with pytest.raises(ValueError):
            pkg.mel_spec(*SETS[name][:2], SETS[name][3])  # no dense record reaches this size
    nz = [np.nonzero(row)[0] for row in B]
    print(name, "non-zeros", int((B != 0).sum()), "longest run", max(int(k[-1] - k[0] + 1) for k in nz))
    if name in ("mf_tts", "mf_music", "mf_sep", "mf_big"):
        assert (int((B != 0).sum()), max(int(k[-1] - k[0] + 1) for k in nz)) == {"mf_tts": (727, 27), "mf_music": (2014, 64), "mf_sep": (4029, 127),
                                                                                 "mf_big": (4644, 220)}[name]
    window, twiddle = pkg.spec_fft_tables(rec)
    swin, stw = pkg.stft_fft_tables(stft_twin(pkg, rec))
    assert window.dtype == twiddle.dtype == np.float32 and window.shape == (n_fft,) and twiddle.shape == (n_fft // 2, 2)
    assert np.array_equal(window.view(np.uint32), swin.view(np.uint32)) and np.array_equal(twiddle.view(np.uint32), stw.view(np.uint32))
    assert np.array_equal(window.view(np.uint32), window64(rec).astype(np.float32).view(np.uint32))
    zero_win = _but(rec, win_length=0 if SETS[name][2] == n_fft else SETS[name][2])  # the C record's "0 means n_fft"
    assert np.array_equal(pkg.spec_fft_tables(zero_win)[0].view(np.uint32), window.view(np.uint32))
    assert np.array_equal(pkg.spec_filterbank(zero_win).view(np.uint32), B.view(np.uint32))


# ---- the reference and the yardstick ------------------------------------------------------------------------
def test_reference_is_the_definition(pkg):
    """melfft_ref against melspec_ref, the matrix definition, on the four sets small enough for it: both are float64 sums of the
    same terms in other orders.  Per bin Re and Im differ by at most 4 n_fft 2^-53 (win / 2) max |x| (tests/test_tracks_fft.py::
    _bound), so S by a relative 2^-40 or so of the frame's largest S, and the mel cells -- sums of non-negative terms -- with it:
    held as |d mel| <= 1e-10 x the frame's largest mel, and the outputs as finish()'s of those."""
    rng = np.random.default_rng(2048)
    for name in SMALL:
        rec = mf_of(pkg, name)
        H, N = int(rec["hop"][0]), int(rec["n_fft"][0])
        for n, scale in ((1, 1.0), (H + 1, 2.0 ** -15), (N // 2, 2.0 ** -15), (N, 1.0), (7 * H + 5, 2.0 ** -15), (12 * H, -3.7e-3)):
            y = rng.integers(-32768, 32768, n, dtype=np.int16)
            got, mel = melfft_ref(y, scale, rec)
            want, mel2 = melspec_ref(y, scale, _but(rec, reserved=0))
            assert got.shape == want.shape == (frame_count(rec, n), int(rec["n_mels"][0]))
            if not len(got):
                continue
            top = mel2.max(axis=1, keepdims=True)
            err = float((np.abs(mel - mel2) / np.where(top == 0, 1.0, top)).max())
            print(name, n, "max |d mel| over the frame's largest", err)
            assert err <= 1e-10
            keep = kept_cells(mel2)
            assert float(error_of(got, want, rec)[keep].max(initial=0)) <= 1e-2 * YARDSTICK[name]
    zero, _ = melfft_ref(np.zeros(5000, dtype=np.int16), -1.0, mf_of(pkg, "mf_sep"))
    assert zero.shape == (5, 128) and (zero == np.log10(float(np.float32(1e-10)))).all()
    assert (melfft_ref(np.zeros(100, dtype=np.int16), -1.0, mf_of(pkg, "mf_tiny"))[0] == 0).all()


def test_yardstick(pkg):
    """The yardstick of the GPU test's tolerance per set: the largest error of melfft_f32 against melfft_ref over the kept cells of
    crafted_tracks, held to the recorded YARDSTICK -- what this test measured -- within a factor of 2 either way: the value is a
    maximum over tens of thousands of cells of a float32 matmul whose summation order is the BLAS's, so another build of numpy may
    move it, but not to another magnitude; and, from melfft_ref alone, that no cell of a track that is not all zero is left out.  A mel cell is a sum of non-negative float32 terms, each S off by about
    log2(n_fft) 2^-24 relative to its frame's largest magnitude, so the error stays near 1e-6 where the STFT's own kept cells reach
    1e-2."""
    for name in SETS:
        worst, cells, dropped = yardstick(pkg, name)
        print(f"{name}: float32 FFT, S and band product, max error {worst:.3g} over {cells - dropped} kept cells of {cells}, {dropped} not kept, "
              f"recorded {YARDSTICK[name]:.3g}")
        assert (cells, dropped) == (CELLS[name], 0), name
        assert 0 < worst < 1e-4, name
        assert YARDSTICK[name] / 2 <= worst <= 2 * YARDSTICK[name], (name, worst)


# ---- the kernels' resources ---------------------------------------------------------------------------------
def test_kernel_resources():
    """k_tracks_melfft: no scratch, no static LDS (a launch asks for its frames' buffers and the store area, 52,224 bytes at most)
    and at most 128 registers; k_tracks_fft, whose load, passes and split it calls, keeps its own: at most 45 (bins-major) and 50
    (frames-major) registers, no scratch, no static LDS."""
    meta = _kernel_metadata()
    seen = [v for mangled, v in meta.items() if re.search(r"\d+k_tracks_melfft(P|E|v|$)", mangled)]
    print("k_tracks_melfft", seen)
    assert len(seen) == 1, sorted(meta)[:6]
    vgpr, scratch, lds = seen[0]
    assert vgpr <= 128 and scratch == 0 and lds == 0
    fft = {("ILb1EE" in mangled): v for mangled, v in meta.items() if re.search(r"\d+k_tracks_fftILb[01]EE", mangled)}
    print("k_tracks_fft", fft)
    assert set(fft) == {False, True}
    assert fft[False][0] <= 45 and fft[True][0] <= 50 and all(v[1] == 0 and v[2] == 0 for v in fft.values())
    assert len([m for m in meta if re.search(r"\d+k_tracks_melspec(P|E|v|$)", m)]) == 1  # and k_tracks_melspec's own test still matches one


def test_lds_fits(pkg):
    """The launch's dynamic LDS by the header's rule -- the frames in flight times n_fft / 2 + n_fft / 64 float2 places, and a store
    area of n_mels rows of 36 floats -- is at most 65,536 bytes at every size with 128 bands."""
    for e in range(6, 14):
        M, C = (1 << e) // 2, 256 // min(256, (1 << e) // 8)
        assert C * (M + M // 32) * 8 + 128 * 36 * 4 <= 52224 <= 65536
