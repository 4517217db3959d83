"""Kaldi fbank and MFCC features of the whole-file path (include/opusgpu.h, TRACK KALDI FEATURES), what needs no GPU: the exported
symbols and the record, the tables against the header's formulas for the parameter sets of SETS, known answers that do not pass
through the reference's DFT, the frame counts and reflected indices by hand, the refusals of the record, the helpers, the C calls
and decode_files before any device work, the files_request rows, and the kernel's resources.

fbank_ref is the float64 numpy restatement of the header's value that the GPU checks (tests/test_gpu_tracks_fbank.py) compare
against; fbank_f32 is the same in float32 with the library's tables.  YARDSTICK is, per set, the largest error of fbank_f32 against
fbank_ref on the kept cells of crafted_tracks, measured on a CPU; yardstick() recomputes it; TOL = 8 x that (DESIGN.md sections 13d
and 13i).  error_of: the absolute difference of log outputs, a relative one for log = none, an absolute one of MFCC coefficients.

The tables are held bit for bit: the double formulas here go through Python's math module, which is the C library's libm, the one
the library's builders call."""
import functools
import math
import os
import re
import zlib

import numpy as np
import pytest

from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_fbank_window", "opusgpu_fbank_filterbank", "opusgpu_fbank_dct", "opusgpu_fbank_layout", "opusgpu_tracks_fbank_device",
       "opusgpu_files_decode_fbank", "opusgpu_ms_files_decode_fbank"]
# kaldi_fbank / kaldi_mfcc keywords; the milliseconds come to (L, H) samples and n_fft to N as the comments say
SETS = {
    "wenet": dict(sample_rate=16000, num_mel_bins=80),                                                               # 400 / 160 / 512, povey, 0.97, dc
    "mfcc8k": dict(sample_rate=8000, num_mel_bins=23, num_ceps=13, cepstral_lifter=22.0),                            # 200 / 80 / 256
    "nosnip": dict(sample_rate=16000, num_mel_bins=40, window_type="hamming", snip_edges=False),                     # 400 / 160 / 512
    "tiny": dict(sample_rate=8000, frame_length=3.125, frame_shift=0.625, num_mel_bins=4, window_type="rectangular",  # 25 / 5 / 64
                 preemphasis_coefficient=0.0, remove_dc_offset=False, use_power=False, use_log_fbank=False),
    "wide": dict(sample_rate=48000, num_mel_bins=128, window_type="blackman", high_freq=-400.0),                     # 1200 / 480 / 2048
    # under this kernel's LDS bound, (T - 1) H + L <= 32768 samples, `wide` gets the tile of 64 frames (63 * 480 + 1200 = 31440): a
    # sixth set gets the tile of 32 (63 * 1000 + 1024 > 32768), without snip_edges, with as many coefficients as bands, unlifted
    "far": dict(sample_rate=32000, frame_length=32.0, frame_shift=31.25, num_mel_bins=40, window_type="hanning", snip_edges=False,  # 1024 / 1000 / 1024
                num_ceps=40, cepstral_lifter=0.0),
}
SHAPES = {"wenet": (400, 160, 512), "mfcc8k": (200, 80, 256), "nosnip": (400, 160, 512), "tiny": (25, 5, 64), "wide": (1200, 480, 2048),
          "far": (1024, 1000, 1024)}
TILES = {"wenet": 128, "mfcc8k": 128, "nosnip": 128, "tiny": 128, "wide": 64, "far": 32}
# the largest error of fbank_f32 against fbank_ref on the kept cells of crafted_tracks, measured on a CPU (yardstick())
YARDSTICK = {"wenet": 6.89e-05, "mfcc8k": 6.47e-05, "nosnip": 1.42e-05, "tiny": 2.09e-07, "wide": 5.00e-05, "far": 5.32e-05}
TOL = {n: 8 * v for n, v in YARDSTICK.items()}


def spec_of(pkg, name, feature_layout="frames"):
    kw = dict(SETS[name], feature_layout=feature_layout)
    return pkg.kaldi_mfcc(**kw) if "num_ceps" in kw else pkg.kaldi_fbank(**kw)


def dims(rec):
    """(L, H, N, n_mels, n_ceps) of a record, N with the 0 rule."""
    L, N = int(rec["frame_length"][0]), int(rec["n_fft"][0])
    if not N:
        N = 64
        while N < L:
            N *= 2
    return L, int(rec["frame_shift"][0]), N, int(rec["n_mels"][0]), int(rec["n_ceps"][0])


def width_of(rec):
    return int(rec["n_ceps"][0]) or int(rec["n_mels"][0])


def tile_of(rec):
    L, H = dims(rec)[:2]
    return next(T for T in (128, 64, 32) if (T - 1) * H + L <= 32768 or T == 32)


# ---- the header's formulas, in float64 ----------------------------------------------------------------------
def window64(rec):
    L = dims(rec)[0]
    kind = int(rec["window"][0])
    w = []
    for i in range(L):
        a = 2.0 * math.pi * i / float(L - 1)
        w.append({0: lambda: math.pow(0.5 - 0.5 * math.cos(a), 0.85), 1: lambda: 0.5 - 0.5 * math.cos(a), 2: lambda: 0.54 - 0.46 * math.cos(a),
                  3: lambda: 1.0, 4: lambda: 0.42 - 0.5 * math.cos(a) + 0.08 * math.cos(2.0 * a)}[kind]())
    return np.array(w)


def high_of(rec):
    high = float(rec["high_freq"][0])
    return high if high > 0 else int(rec["sample_rate"][0]) / 2.0 + high


def filterbank64(rec):
    """B [n_mels, N / 2] in float64, as the header writes it out: triangles linear in mel."""
    _, _, N, n_mels, _ = dims(rec)
    bw = int(rec["sample_rate"][0]) / float(N)

    def mel(f):
        return 1127.0 * math.log(1.0 + f / 700.0)
    m_lo, m_hi = mel(float(rec["low_freq"][0])), mel(high_of(rec))
    delta = (m_hi - m_lo) / (n_mels + 1)
    B = np.zeros((n_mels, N // 2))
    mk = [mel(k * bw) for k in range(N // 2)]
    for j in range(n_mels):
        left = m_lo + j * delta
        centre = left + delta
        right = centre + delta
        for k in range(N // 2):
            B[j, k] = max(0.0, min((mk[k] - left) / (centre - left), (right - mk[k]) / (right - centre)))
    return B


def dct64(rec):
    """lift[q] D[q][j], [n_ceps, n_mels] in float64."""
    n_mels, n_ceps = dims(rec)[3:]
    Q = float(rec["cepstral_lifter"][0])
    D = np.zeros((n_ceps, n_mels))
    for q in range(n_ceps):
        lift = 1.0 + 0.5 * Q * math.sin(math.pi * q / Q) if Q > 0 else 1.0
        for j in range(n_mels):
            d = math.sqrt(2.0 / n_mels) * math.cos(math.pi * q * (j + 0.5) / n_mels) if q else math.sqrt(1.0 / n_mels)
            D[q, j] = lift * d
    return D


def dft64(rec):
    """(cos, sin) [L, N / 2] of 2 pi i k / N, the angle reduced in integers."""
    L, _, N, _, _ = dims(rec)
    i, k = np.arange(L)[:, None], np.arange(N // 2)[None, :]
    a = 2.0 * np.pi * ((i * k) % N) / float(N)
    return np.cos(a), np.sin(a)


def frame_count(rec, n):
    L, H = dims(rec)[:2]
    if int(rec["snip_edges"][0]):
        return 0 if n < L else 1 + (n - L) // H
    return (n + H // 2) // H


def reflect(q, n):
    """Kaldi's rule one step at a time, as the header words it: q < 0 -> -q - 1, q >= n -> 2 n - 1 - q, until inside."""
    q = np.array(q, dtype=np.int64)
    while ((q < 0) | (q >= n)).any():
        q = np.where(q < 0, -q - 1, np.where(q >= n, 2 * n - 1 - q, q))
    return q


def frames_of(n, rec):
    """The sample indices [F, L] of the frames of a track of n samples."""
    L, H = dims(rec)[:2]
    F = frame_count(rec, n)
    snip = int(rec["snip_edges"][0])
    q = H * np.arange(F)[:, None] + (0 if snip else H // 2 - L // 2) + np.arange(L)[None, :]
    if F and not snip:
        q = reflect(q, n)
    assert not F or (q.min() >= 0 and q.max() < n)
    return q


@functools.lru_cache(maxsize=None)
def _tables64(key):
    rec = np.frombuffer(key, dtype=_tables64.dtype).copy()
    return window64(rec), filterbank64(rec), dct64(rec), dft64(rec)


def tables64(rec):
    _tables64.dtype = rec.dtype
    key = rec.copy()
    key["layout"] = 0
    return _tables64(key.tobytes())


def fbank_ref(y, scale, rec):
    """TRACK KALDI FEATURES in float64: y int16 [n] -> (output [F, width], mel [F, n_mels]).  scale and the record's floats are the
    float32 values they are; everything else is float64."""
    y = np.asarray(y, dtype=np.int16)
    L = dims(rec)[0]
    w, B, D, (co, si) = tables64(rec)
    q = frames_of(len(y), rec)
    x = y.astype(np.float64)[q] if len(q) else np.zeros((0, L))
    if int(rec["remove_dc"][0]):
        x = x - x.sum(axis=1, keepdims=True) / L
    c = float(rec["preemphasis"][0])
    e = x - c * np.concatenate([x[:, :1], x[:, :-1]], axis=1)
    t = e * float(np.float32(scale)) * w
    S = (t @ co) ** 2 + (t @ si) ** 2
    if int(rec["power"][0]) == 1:
        S = np.sqrt(S)
    mel = S @ B.T
    v = np.maximum(mel, float(rec["floor"][0]))
    out = np.log(v) if int(rec["log"][0]) else v
    if int(rec["n_ceps"][0]):
        out = out @ D.T
    return out, mel


def fbank_f32(y, scale, rec, w, B, D):
    """The same value in float32 throughout, with the library's float32 tables, summed in numpy's order: the yardstick for the
    kernel's tolerance."""
    y = np.asarray(y, dtype=np.int16)
    L = dims(rec)[0]
    co, si = (a.astype(np.float32) for a in tables64(rec)[3])
    q = frames_of(len(y), rec)
    x = y.astype(np.float32)[q] if len(q) else np.zeros((0, L), dtype=np.float32)
    if int(rec["remove_dc"][0]):
        x = x - (y.astype(np.int64)[q].sum(axis=1, keepdims=True).astype(np.float32) / np.float32(L))
    c = rec["preemphasis"][0]
    e = x - c * np.concatenate([x[:, :1], x[:, :-1]], axis=1)
    t = e * np.float32(scale) * w
    assert t.dtype == np.float32
    re, im = t @ co, t @ si
    S = re * re + im * im
    if int(rec["power"][0]) == 1:
        S = np.sqrt(S)
    v = np.maximum(S @ np.ascontiguousarray(B.T), rec["floor"][0])
    out = np.log(v) if int(rec["log"][0]) else v
    if int(rec["n_ceps"][0]):
        out = out @ np.ascontiguousarray(D.T)
    assert out.dtype == np.float32
    return out


def error_of(got, ref, rec):
    """The error the tolerance is held on: absolute for log outputs and MFCC coefficients, relative for log = none (absolute where
    the reference is 0)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return d if int(rec["log"][0]) else d / np.where(ref == 0, 1.0, np.abs(ref))


def kept_cells(mel, rec):
    """The cells the tolerance is held on: float64 mel at least 1e-8 x its frame's largest; for MFCC every coefficient of a frame
    whose mels are all kept.  [F, width] bool."""
    if not mel.size:
        return np.zeros((mel.shape[0], width_of(rec)), dtype=bool)
    keep = mel >= 1e-8 * mel.max(axis=1, keepdims=True)
    if int(rec["n_ceps"][0]):
        keep = np.repeat(keep.all(axis=1, keepdims=True), width_of(rec), axis=1)
    return keep


# ---- the crafted tracks of the GPU test, their reference and the yardstick -----------------------------------
def lengths_of(rec):
    """Every length at which the kernel changes path, for the record's L, H and tile T."""
    L, H = dims(rec)[:2]
    T = tile_of(rec)
    want = [0, 1, H // 2 - 1, H // 2, L // 2, L - 1, L, L + 1, L + H - 1, L + H, 31 * H + L - 1, 31 * H + L, 32 * H + L,
            (T - 1) * H + L - 1, (T - 1) * H + L, T * H + L, T * H + L + H + 1]
    return list(dict.fromkeys(n for n in want if n >= 0))


@functools.lru_cache(maxsize=None)
def crafted_tracks(name, rec_bytes):
    """(tracks, scales): every length of lengths_of twice, uniform random int16 -- once with the default scale, once with a random
    finite one --, an all-zero track, a constant -1234 track, a track of +-40 noise and one of 8000 + (+-20) noise (the dc case)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rec = np.frombuffer(rec_bytes, dtype=crafted_tracks.dtype).copy()
    L, H = dims(rec)[:2]
    tracks, scales = [], []
    for n in lengths_of(rec):
        for k in range(2):
            tracks.append(rng.integers(-32768, 32768, n, dtype=np.int16))
            scales.append(2.0 ** -15 if k == 0 else float(rng.choice([-1, 1]) * rng.uniform(1, 10) * 10.0 ** rng.integers(-6, 3)))
    m = L + 5 * H + 3
    tracks += [np.zeros(m, dtype=np.int16), np.full(m, -1234, dtype=np.int16), rng.integers(-40, 41, L + 9 * H + 77, dtype=np.int16),
               (8000 + rng.integers(-20, 21, L + 9 * H + 77)).astype(np.int16)]
    scales += [2.0 ** -15] * 4
    scales = np.asarray(scales, dtype=np.float32)
    assert np.isfinite(scales).all() and (scales != 0).all()
    return tracks, scales


def crafted(pkg, name):
    """(record, tracks, scales, [(output, mel)]) of a set, the reference computed once."""
    rec = spec_of(pkg, name)
    crafted_tracks.dtype = rec.dtype
    tracks, scales = crafted_tracks(name, rec.tobytes())
    return rec, tracks, scales, _crafted_reference(name, rec.tobytes())


@functools.lru_cache(maxsize=None)
def _crafted_reference(name, rec_bytes):
    rec = np.frombuffer(rec_bytes, dtype=crafted_tracks.dtype).copy()
    tracks, scales = crafted_tracks(name, rec_bytes)
    return [fbank_ref(y, s, rec) for y, s in zip(tracks, scales)]


def is_flat(y):
    return len(y) > 0 and (y == y[0]).all()


def yardstick(pkg, name):
    rec, tracks, scales, refs = crafted(pkg, name)
    w, B, D = pkg.fbank_window(rec), pkg.fbank_filterbank(rec), pkg.fbank_dct(rec)
    worst = 0.0
    for y, s, (ref, mel) in zip(tracks, scales, refs):
        if len(ref):
            worst = max(worst, float(error_of(fbank_f32(y, s, rec, w, B, D), ref, rec)[kept_cells(mel, rec)].max(initial=0)))
    return worst


# ---- symbols, records, tables -------------------------------------------------------------------------------
def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "TRACK KALDI FEATURES" in hdr and "opusgpu_fbank_params { /* 64 bytes" in hdr
    d = pkg.FBANK_PARAMS_DTYPE
    assert d.itemsize == 64
    want = [("sample_rate", 0), ("frame_length", 4), ("frame_shift", 8), ("n_fft", 12), ("n_mels", 16), ("n_ceps", 20), ("window", 24),
            ("snip_edges", 28), ("remove_dc", 29), ("power", 30), ("log", 31), ("layout", 32), ("preemphasis", 36), ("low_freq", 40),
            ("high_freq", 44), ("floor", 48), ("cepstral_lifter", 52), ("reserved", 56)]
    assert [(n, d.fields[n][1]) for n in d.names] == want
    assert d.fields["reserved"][0].shape == (2,) and d.fields["floor"][0] == np.float32 and d.fields["power"][0] == np.uint8
    for name, value in (("POVEY", 0), ("HANNING", 1), ("HAMMING", 2), ("RECTANGULAR", 3), ("BLACKMAN", 4), ("LOG_NONE", 0), ("LOG_LN", 1)):
        assert re.search(rf"#define OPUSGPU_FBANK_{name} {value}\b", hdr), name
    fields = re.search(r"typedef struct opusgpu_fbank_params \{(.*?)\} opusgpu_fbank_params;", hdr, re.S).group(1)
    assert re.findall(r"^\s+\w+ (\w+)(?:\[2\])?;", fields, re.M) == list(d.names)
    rec = pkg.kaldi_fbank()  # Kaldi's defaults
    assert [int(rec[n][0]) for n in d.names[:12]] == [16000, 400, 160, 512, 23, 0, 0, 1, 1, 2, 1, pkg.MEL_FRAMES_MAJOR]
    assert [float(rec[n][0]) for n in d.names[12:17]] == [float(np.float32(0.97)), 20.0, 0.0, float(np.float32(1.1920929e-07)), 0.0]
    rec = pkg.kaldi_mfcc()
    assert (int(rec["n_ceps"][0]), float(rec["cepstral_lifter"][0]), int(rec["log"][0]), pkg.fbank_width(rec)) == (13, 22.0, 1, 13)
    for name, shape in SHAPES.items():
        assert dims(spec_of(pkg, name))[:3] == shape, name
    assert {n: tile_of(spec_of(pkg, n)) for n in SETS} == TILES
    assert int(pkg.kaldi_fbank(sample_rate=22050)["frame_length"][0]) == 551 and int(pkg.kaldi_fbank(sample_rate=22050)["n_fft"][0]) == 1024
    assert int(pkg.kaldi_fbank(frame_length=32.0, round_to_power_of_two=False)["n_fft"][0]) == 512
    assert int(pkg.kaldi_fbank(frame_length=20.0, round_to_power_of_two=False)["n_fft"][0]) == 320
    assert pkg.kaldi_fbank(dither=0.0, use_energy=False, htk_compat=False, vtln_warp=1.0, subtract_mean=False, energy_floor=1.0, raw_energy=True,
                           blackman_coeff=0.42, channel=-1, min_duration=0.0) == pkg.kaldi_fbank()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), np.ascontiguousarray(b.astype(np.float32)).view(np.uint32))


@pytest.mark.parametrize("name", list(SETS) + ["n_fft 0", "high_freq 0", "povey odd"])
def test_tables_are_the_formulas_rounded_once(pkg, name):
    """Bit for bit (the module's docstring says why that holds here)."""
    if name in SETS:
        rec = spec_of(pkg, name)
    elif name == "n_fft 0":  # the C record's "0 means the smallest power of two >= max(L, 64)"
        rec = pkg.kaldi_mfcc(sample_rate=22050, num_mel_bins=30, num_ceps=30, cepstral_lifter=7.5)
        same = rec.copy()
        rec["n_fft"] = 0
        assert dims(rec)[2] == 1024 == int(same["n_fft"][0])
        assert same_bits(pkg.fbank_filterbank(rec), pkg.fbank_filterbank(same))
    elif name == "high_freq 0":  # high_freq <= 0 counts from Nyquist: 0 is Nyquist, -400 is 7600 at 16 kHz
        rec = pkg.kaldi_fbank(num_mel_bins=23, high_freq=0.0)
        assert same_bits(pkg.fbank_filterbank(rec), pkg.fbank_filterbank(pkg.kaldi_fbank(num_mel_bins=23, high_freq=8000.0)))
        assert same_bits(pkg.fbank_filterbank(pkg.kaldi_fbank(high_freq=-400.0)), pkg.fbank_filterbank(pkg.kaldi_fbank(high_freq=7600.0)))
        assert not same_bits(pkg.fbank_filterbank(rec), pkg.fbank_filterbank(pkg.kaldi_fbank(high_freq=7600.0)))
    else:
        rec = pkg.kaldi_fbank(sample_rate=11025, num_mel_bins=20)  # L = 275
        assert dims(rec)[0] % 2 == 1
    L, _, N, n_mels, n_ceps = dims(rec)
    w, B, D = pkg.fbank_window(rec), pkg.fbank_filterbank(rec), pkg.fbank_dct(rec)
    assert w.dtype == B.dtype == D.dtype == np.float32 and w.shape == (L,) and B.shape == (n_mels, N // 2) and D.shape == (n_ceps, n_mels)
    assert same_bits(w, window64(rec)) and same_bits(B, filterbank64(rec)) and same_bits(D, dct64(rec))
    assert np.abs(w - w[::-1]).max() <= 2.0 ** -23  # w[i] = w[L - 1 - i] but for the rounding of the double cosines: what the kernel's fold rests on
    assert (B >= 0).all() and (B <= 1).all()
    lib = pkg.load_lib()
    assert lib.opusgpu_fbank_window(rec.ctypes.data, None) == L and lib.opusgpu_fbank_filterbank(rec.ctypes.data, None) == B.size
    assert lib.opusgpu_fbank_dct(rec.ctypes.data, None) == D.size
    kept = [nb for nb in range((N // 2 + 31) // 32) if B[:, 32 * nb:32 * nb + 32].any()]
    print(name, "tile", tile_of(rec), "bin blocks kept", len(kept), "of", (N // 2 + 31) // 32, "empty bands", int((B.max(axis=1) == 0).sum()))


def test_an_unreached_band_is_a_row_of_zeros(pkg):
    """128 bands over 64-point bins at 8 kHz: most triangles lie between two bins.  As in Kaldi they are rows of zeros, and their
    output is the floor."""
    rec = pkg.kaldi_fbank(sample_rate=8000, frame_length=3.125, frame_shift=1.25, num_mel_bins=128)
    B = pkg.fbank_filterbank(rec)
    assert same_bits(B, filterbank64(rec)) and (B.max(axis=1) == 0).sum() > 60
    out, mel = fbank_ref(np.random.default_rng(2).integers(-3000, 3000, 100, dtype=np.int16), 1.0, rec)
    assert (out[:, B.max(axis=1) == 0] == np.log(float(rec["floor"][0]))).all() and (mel[:, B.max(axis=1) > 0] > 0).all()


# ---- known answers that do not pass through the reference's DFT -----------------------------------------------
def test_known_answers(pkg):
    # an impulse in a rectangular window, no dc removal, no pre-emphasis: |X[k]| = a scale for every k, mel[j] = (a scale)^2 sum_k B[j][k]
    rec = pkg.kaldi_fbank(sample_rate=8000, frame_length=3.125, frame_shift=3.125, num_mel_bins=6, window_type="rectangular",
                          preemphasis_coefficient=0.0, remove_dc_offset=False, use_log_fbank=False)
    assert dims(rec)[:3] == (25, 25, 64)
    B = filterbank64(rec)
    for a, at, scale in ((12345, 7, 2.0 ** -15), (-32768, 0, 1.0), (3, 24, 0.37)):
        y = np.zeros(50, dtype=np.int16)
        y[at], y[25 + (at + 11) % 25] = a, a
        out, mel = fbank_ref(y, scale, rec)
        want = (a * float(np.float32(scale))) ** 2 * B.sum(axis=1)
        assert out.shape == (2, 6) and np.allclose(mel, want[None, :], rtol=1e-12, atol=0) and np.array_equal(out, np.maximum(mel, float(rec["floor"][0])))
    mag = rec.copy()
    mag["power"] = 1
    assert np.allclose(fbank_ref(y, 0.37, mag)[1], 3 * float(np.float32(0.37)) * B.sum(axis=1)[None, :], rtol=1e-12, atol=0)
    # a constant track with remove_dc: the floor's value in every cell; MFCC: the DCT of a constant row
    for name in ("wenet", "mfcc8k", "wide", "far"):
        r = spec_of(pkg, name)
        L, H = dims(r)[:2]
        out, mel = fbank_ref(np.full(L + 3 * H, -1234, dtype=np.int16), 1.0, r)
        assert len(out) >= 3 and (mel == 0).all()
        lf = np.log(float(r["floor"][0]))
        if int(r["n_ceps"][0]):
            assert np.allclose(out, (np.full(dims(r)[3], lf) @ dct64(r).T)[None, :], rtol=1e-12, atol=1e-12)
        else:
            assert (out == lf).all()
    # without remove_dc and pre-emphasis a constant is a tone at 0 Hz: energy, in the lowest bands most
    r = pkg.kaldi_fbank(remove_dc_offset=False, preemphasis_coefficient=0.0, low_freq=0.0)
    out, _ = fbank_ref(np.full(1000, 500, dtype=np.int16), 1.0, r)
    assert out[:, 0].min() > out[:, 5].max() > np.log(float(r["floor"][0]))
    # pre-emphasis: the frame's first sample is its own predecessor -- a frame that is a step at its own start has e_0 = (1 - c) d_0
    step = pkg.kaldi_fbank(sample_rate=8000, frame_length=3.125, frame_shift=3.125, num_mel_bins=6, window_type="rectangular",
                           remove_dc_offset=False, use_log_fbank=False, preemphasis_coefficient=1.0)
    y = np.zeros(50, dtype=np.int16)
    y[25:] = 1000  # the second frame is constant: with c = 1 every e is 0, whatever lies in front of the frame
    assert (fbank_ref(y, 1.0, step)[1] == 0).all()


def test_frame_counts_and_reflection_by_hand(pkg):
    snip, nosnip = spec_of(pkg, "wenet"), spec_of(pkg, "nosnip")
    L, H = 400, 160
    for n, F1, F0 in ((0, 0, 0), (1, 0, 0), (79, 0, 0), (80, 0, 1), (L - 1, 0, 2), (L, 1, 3), (L + H - 1, 1, 3), (L + H, 2, 4), (239, 0, 1), (240, 0, 2)):
        assert frame_count(snip, n) == F1 and frame_count(nosnip, n) == F0, n
        assert int(pkg.fbank_frames(snip, n)) == F1 and int(pkg.fbank_frames(nosnip, n)) == F0
        assert fbank_ref(np.zeros(n, dtype=np.int16), 1.0, snip)[0].shape == (F1, 80)
        assert fbank_ref(np.zeros(n, dtype=np.int16), 1.0, nosnip)[0].shape == (F0, 40)
    assert list(pkg.fbank_frames(snip, [0, 399, 400, 559, 560])) == [0, 0, 1, 1, 2]
    q = frames_of(1000, snip)
    assert q.shape == (4, 400) and q[0, 0] == 0 and q[3, 399] == 879
    q = frames_of(1000, nosnip)  # 6 frames, frame f from 160 f - 120
    assert q.shape == (6, 400) and list(q[0, :3]) == [119, 118, 117] and list(q[0, 119:122]) == [0, 0, 1] and q[5, 0] == 680
    assert q[5, 319] == 999 and q[5, 320] == 999 and q[5, 321] == 998 and q[5, 399] == 920
    # n = 3 < L / 2 with an L of 8 and an H of 4 (one frame from 2 - 4 = -2): several reflections, by hand:
    # q = -2 .. 5 -> -2: 1, -1: 0, 0, 1, 2, 3: 2, 4: 1, 5: 0
    small = pkg.kaldi_fbank(sample_rate=8000, frame_length=1.0, frame_shift=0.5, num_mel_bins=3, snip_edges=False)
    assert dims(small)[:2] == (8, 4)
    assert frames_of(3, small).tolist() == [[1, 0, 0, 1, 2, 2, 1, 0]]
    # L = 25, H = 5 (no snip_edges): F = 0, 1 at n = 2, 3; at n = 3 frame 0 runs from 2 - 12 = -10 and the period is 2 n = 6: 0 1 2 2 1 0
    odd = pkg.kaldi_fbank(sample_rate=8000, frame_length=3.125, frame_shift=0.625, num_mel_bins=4, snip_edges=False)
    assert frame_count(odd, 2) == 0 and frame_count(odd, 3) == 1
    assert frames_of(3, odd).tolist() == [[2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2]]
    assert reflect([-7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6], 2).tolist() == [1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1]
    assert np.array_equal(reflect(np.arange(-50, 50), 7), np.where(np.arange(-50, 50) % 14 < 7, np.arange(-50, 50) % 14, 13 - np.arange(-50, 50) % 14))


def test_layout_helper(pkg):
    planned = np.array([0, 1, 479, 480, 1199, 1200, 1201, 3 * 160 * 64 + 3 * 240, 0, 7, 48000 * 3 + 5], dtype=np.int64)
    for name, up, down in (("wenet", 1, 3), ("nosnip", 1, 3), ("mfcc8k", 1, 6), ("wide", 1, 1), ("far", 2, 3)):
        for layout in ("bands", "frames"):
            rec = spec_of(pkg, name, layout)
            n = -(-planned * up // down)
            F = np.array([frame_count(rec, int(x)) for x in n])
            plane = (F + 63) // 64 * 64
            offs, planes, total = pkg.fbank_layout(planned, up, down, rec)
            want = np.concatenate([[0], np.cumsum(width_of(rec) * plane)])
            assert np.array_equal(planes, plane) and np.array_equal(offs, want[:-1]) and total == want[-1] and (offs % 64 == 0).all()
            assert np.array_equal(pkg.fbank_frames(rec, n), F)
    rec = spec_of(pkg, "wenet")
    offs, planes, total = pkg.fbank_layout([], 1, 3, rec)
    assert len(offs) == 0 and total == 0
    lib = pkg.load_lib()
    BAD = pkg.OPUSGPU_BAD_ARG
    ok = rec.ctypes.data
    assert lib.opusgpu_fbank_layout(planned.size, planned.ctypes.data, 1, 3, ok, None) == pkg.fbank_layout(planned, 1, 3, rec)[2]
    for up, down in ((0, 3), (3, 1), (1, 0), (-1, 3), (1, 48001)):
        assert lib.opusgpu_fbank_layout(planned.size, planned.ctypes.data, up, down, ok, None) == BAD
    assert lib.opusgpu_fbank_layout(2, planned.ctypes.data, 1, 3, None, None) == BAD and lib.opusgpu_fbank_layout(-1, planned.ctypes.data, 1, 3, ok, None) == BAD
    assert lib.opusgpu_fbank_layout(2, None, 1, 3, ok, None) == BAD
    with pytest.raises(ValueError):
        pkg.fbank_layout([5, -1], 1, 3, rec)
    for other in (pkg.mel_params(80), pkg.mel_spec(16000, 512, 160)):  # the other sections' records are other records
        with pytest.raises(ValueError):
            pkg.fbank_layout(planned, 1, 3, other)


def test_float32_restatement_is_close_and_the_yardstick_is_recorded(pkg):
    """yardstick() per set next to what the file records: the recorded number is a measurement, within a factor of 4 of this CPU's."""
    for name in SETS:
        rec, tracks, scales, refs = crafted(pkg, name)
        cells = sum(kept_cells(mel, rec).size for _, mel in refs)
        dropped = sum(int((~kept_cells(mel, rec)).sum()) for _, mel in refs)
        got = yardstick(pkg, name)
        print(f"{name}: float32 restatement, max error {got:.3g} (recorded {YARDSTICK[name]:.3g}), {cells} cells, {dropped} not kept")
        assert cells > 500 and dropped == 0  # the float64 statement of the definition leaves out no cell of these tracks
        assert YARDSTICK[name] / 4 <= got <= 4 * YARDSTICK[name] and got < 1e-3


# ---- refusals before any device work ------------------------------------------------------------------------
def bad_records(pkg):
    """Records that break one rule of opusgpu_fbank_params each."""
    good = pkg.kaldi_mfcc(num_mel_bins=80, num_ceps=13)

    def but(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    return good, [but(sample_rate=0), but(sample_rate=1048577), but(frame_length=1), but(frame_length=2049), but(frame_length=513),
                  but(frame_shift=0), but(frame_shift=-160), but(frame_shift=1045), but(n_fft=48), but(n_fft=384), but(n_fft=520),
                  but(n_fft=4096), but(n_fft=-512), but(n_mels=2), but(n_mels=129), but(n_ceps=81), but(n_ceps=-1), but(window=5), but(window=-1),
                  but(snip_edges=2), but(remove_dc=2), but(power=0), but(power=3), but(log=2), but(log=0), but(layout=2), but(layout=-1),
                  but(preemphasis=-0.1), but(preemphasis=1.5), but(preemphasis=np.nan), but(low_freq=-1.0), but(low_freq=8000.0),
                  but(low_freq=np.nan), but(high_freq=8000.5), but(high_freq=-7980.0), but(high_freq=-9000.0), but(high_freq=np.nan),
                  but(high_freq=10.0), but(floor=0.0), but(floor=-1.0), but(floor=np.inf), but(floor=np.nan), but(n_ceps=0, log=0, floor=-0.5),
                  but(cepstral_lifter=-1.0), but(cepstral_lifter=np.inf), but(cepstral_lifter=np.nan), but(reserved=[1, 0]), but(reserved=[0, 7])]


def test_records_refuse(pkg):
    assert int(pkg.kaldi_fbank(sample_rate=32000, frame_length=64.0, frame_shift=30.9375)["frame_shift"][0]) == 990  # 31 * 990 + 2048 = 32738
    with pytest.raises(ValueError):
        pkg.kaldi_fbank(sample_rate=32000, frame_length=64.0, frame_shift=31.0)  # 31 * 992 + 2048 = 32800
    for kw in (dict(sample_rate=0), dict(sample_rate=16000.5), dict(sample_rate="16k"), dict(frame_length=0.1), dict(frame_length=200.0),
               dict(frame_length=float("nan")), dict(frame_shift=0.0), dict(frame_shift=70.0), dict(frame_shift="10"), dict(num_mel_bins=2),
               dict(num_mel_bins=129), dict(num_mel_bins=23.0), dict(num_mel_bins=True), dict(low_freq=-1.0), dict(low_freq=8000.0),
               dict(high_freq=8001.0), dict(high_freq=-8000.0), dict(high_freq=float("nan")), dict(preemphasis_coefficient=1.5),
               dict(preemphasis_coefficient=-0.5), dict(preemphasis_coefficient=None), dict(remove_dc_offset=1), dict(snip_edges="yes"),
               dict(use_power=2), dict(use_log_fbank=0), dict(window_type="sine"), dict(window_type=0), dict(round_to_power_of_two=0),
               dict(round_to_power_of_two=False, sample_rate=22050), dict(feature_layout="planar"), dict(feature_layout=1),
               # not offered, each with its reason
               dict(dither=1.0), dict(dither=1e-5), dict(use_energy=True), dict(raw_energy=False), dict(energy_floor=0.5), dict(htk_compat=True),
               dict(vtln_warp=1.1), dict(vtln_low=60.0), dict(vtln_high=-400.0), dict(subtract_mean=True), dict(blackman_coeff=0.5), dict(channel=1),
               dict(min_duration=1.0), dict(dither=None)):
        with pytest.raises(ValueError):
            pkg.kaldi_fbank(**kw)
    with pytest.raises(ValueError, match="no dither"):
        pkg.kaldi_fbank(dither=1.0)
    with pytest.raises(ValueError, match="energy coefficient"):
        pkg.kaldi_mfcc(use_energy=True)
    with pytest.raises(TypeError):
        pkg.kaldi_fbank(hop=160)
    for kw in (dict(num_ceps=0), dict(num_ceps=24), dict(num_ceps=13.0), dict(num_ceps=True), dict(cepstral_lifter=-1.0), dict(cepstral_lifter=float("inf")),
               dict(cepstral_lifter=None), dict(num_mel_bins=10), dict(dither=0.5), dict(htk_compat=True)):
        with pytest.raises(ValueError):
            pkg.kaldi_mfcc(**kw)
    with pytest.raises(TypeError):
        pkg.kaldi_mfcc(use_log_fbank=False)  # MFCC has no such argument
    lib = pkg.load_lib()
    BAD = pkg.OPUSGPU_BAD_ARG
    good, bad = bad_records(pkg)
    planned = np.array([480, 9600], dtype=np.int64)
    assert lib.opusgpu_fbank_window(good.ctypes.data, None) == 400 and lib.opusgpu_fbank_window(None, None) == BAD
    assert lib.opusgpu_fbank_filterbank(None, None) == BAD and lib.opusgpu_fbank_dct(None, None) == BAD
    for rec in bad:
        assert lib.opusgpu_fbank_window(rec.ctypes.data, None) == BAD, rec
        assert lib.opusgpu_fbank_filterbank(rec.ctypes.data, None) == BAD and lib.opusgpu_fbank_dct(rec.ctypes.data, None) == BAD
        assert lib.opusgpu_fbank_layout(2, planned.ctypes.data, 1, 3, rec.ctypes.data, None) == BAD
        for call in (pkg.fbank_window, pkg.fbank_filterbank, pkg.fbank_dct, lambda r: pkg.fbank_layout(planned, 1, 3, r)):
            with pytest.raises(ValueError):
                call(rec)
    for call in (pkg.fbank_window, pkg.fbank_filterbank, pkg.fbank_dct, pkg.fbank_width, lambda r: pkg.fbank_frames(r, 5)):
        for other in (pkg.mel_spec(16000, 512, 160), pkg.mel_params(80), None, np.zeros(2, dtype=pkg.FBANK_PARAMS_DTYPE)):
            with pytest.raises(ValueError):
                call(other)
    edge = good.copy()  # the bounds themselves are inside
    edge["frame_length"], edge["frame_shift"], edge["n_fft"] = 2048, 990, 2048  # 31 * 990 + 2048 = 32738
    assert lib.opusgpu_fbank_window(edge.ctypes.data, None) == 2048
    edge["frame_shift"] = 991
    assert lib.opusgpu_fbank_window(edge.ctypes.data, None) == BAD


def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """Every refusal of the three calls comes back as OPUSGPU_BAD_ARG with d_in / d_out NULL and -- without a device -- from a decoder
    that does not exist (`handles` of tests/test_tracks_resample.py).  A call that got as far as the device would fail otherwise."""
    import ctypes
    lib = pkg.load_lib()
    n = batch.n_files
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    good, bad = bad_records(pkg)  # a record for tracks at 16000 Hz
    at22k = pkg.kaldi_fbank(sample_rate=22050)
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)
    inf = np.array([np.inf] + [1] * (n - 1), dtype=np.float32)
    mono_mix = pkg.mix_matrix("mono", 2)
    two_rows = pkg.mix_matrix(np.eye(2, dtype=np.int16) * 16384, 2)
    six_mono, six_stereo = pkg.mix_matrix("mono", 6), pkg.mix_matrix("stereo", 6)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]

    def files(rate, up, down, mono, mix, p, scale, ctx=fake, b=batch.h, out=None):
        return lib.opusgpu_files_decode_fbank(ctx, b, rate, up, down, mono, None if mix is None else mix.ctypes.data,
                                              None if p is None else p.ctypes.data, None if scale is None else scale.ctypes.data, out,
                                              *[a.ctypes.data for a in arrays])

    def ms_files(rate, up, down, mix, p, scale, ms=fake_ms, b=ms_batch.h):
        return lib.opusgpu_ms_files_decode_fbank(ms, b, rate, up, down, None if mix is None else mix.ctypes.data,
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
    assert files(0, 147, 320, 1, None, good, None) == BAD and files(16000, 0, 0, 1, None, at22k, None) == BAD and ms_files(0, 147, 160, six_mono, at22k, None) == BAD
    # what the rate and ratio calls refuse
    for rate, up, down in ((44100, 0, 0), (22050, 0, 0), (16000, 1, 3), (16000, 0, 3), (16000, 1, 0), (0, 0, 0), (0, 3, 1), (0, 1, 9), (0, -1, 3), (-16000, 0, 0)):
        assert files(rate, up, down, 1, None, good, None) == BAD and ms_files(rate, up, down, six_mono, good, None) == BAD, (rate, up, down)
    for scale in (nan, inf):
        assert files(16000, 0, 0, 1, None, good, scale) == BAD and files(0, 1, 3, 0, mono_mix, good, scale) == BAD
    assert ms_files(16000, 0, 0, six_mono, good, np.array([np.nan] * ms_batch.n_files, dtype=np.float32)) == BAD
    assert files(16000, 0, 0, 1, None, good, None, out=ctypes.c_void_p(64)) == BAD  # a d_out off 128 bytes
    assert all((a == -7).all() for a in arrays)  # and the caller's arrays are as they were

    spans = np.zeros(2, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_samples"], spans["scale"], spans["plane"] = 800, 1.0, 64
    spans["in_offset"], spans["out_offset"] = [0, 808], [0, 64 * 13]

    def kernel(s, p, ctx=fake):
        return lib.opusgpu_tracks_fbank_device(ctx, len(s), s.ctypes.data, None, None if p is None else p.ctypes.data, None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    assert kernel(spans, good, ctx=None) == BAD and kernel(spans, None) == BAD
    for p in bad:
        assert kernel(spans, p) == BAD
    for s in (but(in_offset=4), but(in_offset=-8), but(in_samples=-1), but(out_offset=32), but(out_offset=-64), but(plane=32),
              but(in_samples=400 + 160 * 64), but(scale=np.nan), but(scale=-np.inf), but(reserved=1)):  # 65 frames in a plane of 64
        assert kernel(s, good) == BAD
    assert kernel(spans, good) == BAD  # these spans are in order: refused for the NULL buffers, still before the device
    short = spans.copy()
    short["in_samples"] = [399, 0]
    assert kernel(short, good) == 0 and kernel(spans[:0], good) == 0  # no frame is no error, and no device work
    nosnip = good.copy()
    nosnip["snip_edges"] = 0
    short["in_samples"] = [79, 0]
    assert kernel(short, nosnip) == 0
    short["in_samples"] = [80, 0]
    assert kernel(short, nosnip) == BAD  # F = (n + H / 2) / H has a frame there


def test_decode_files_refusals_need_no_device(pkg, batch):
    """track_kaldi_args, and decode_files raising before it touches its decoder (an object without one is enough to see it)."""
    wenet, mfcc, at22k = spec_of(pkg, "wenet"), spec_of(pkg, "mfcc8k", "bands"), pkg.kaldi_fbank(sample_rate=22050)
    rec, mrec, scale, offs, planes, total, out, how = pkg.track_kaldi_args(batch, wenet, rate=16000, mono=True)
    assert rec is not wenet and np.array_equal(rec, wenet) and (mrec, scale, out, how) == (None, None, None, (16000, 0, 0))
    assert total == pkg.fbank_layout(batch.info["track_samples"], 1, 3, wenet)[2] > 0 and len(offs) == len(planes) == batch.n_files
    assert pkg.track_kaldi_args(batch, wenet, mono=True)[7] == (16000, 0, 0)       # neither: the record's rate is one of TRACK RATES
    assert pkg.track_kaldi_args(batch, mfcc, mono=True)[7] == (8000, 0, 0)
    assert pkg.track_kaldi_args(batch, at22k, mono=True)[7] == (0, 147, 320)        # or a ratio of TRACK RATIOS
    assert pkg.track_kaldi_args(batch, at22k, resample=(294, 640), mix="mono")[7] == (0, 147, 320)
    assert pkg.track_kaldi_args(batch, wenet, resample=16000, mono=True)[7] == (0, 1, 3)
    got = pkg.track_kaldi_args(batch, wenet, 16000, None, False, "mono", "f32", np.ones(batch.n_files))
    assert got[7] == (16000, 0, 0) and int(got[1]["out_channels"][0]) == 1 and got[2].dtype == np.float32
    one = pkg.track_kaldi_args(batch, wenet, mono=True, scale=1.0)[2]  # one number for every track: Kaldi's int16-range convention
    assert one.dtype == np.float32 and np.array_equal(one, np.ones(batch.n_files)) and pkg.files_request(batch, features=wenet, mono=True, scale=1.0).scale is not None
    for scale in (float("nan"), float("inf"), True, "one"):
        with pytest.raises(ValueError):
            pkg.track_kaldi_args(batch, wenet, mono=True, scale=scale)
    six = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files, "track_samples": batch.track_samples})()
    assert pkg.track_kaldi_args(six, at22k, mix="mono", allow_mono=False)[1]["in_channels"][0] == 6
    bad = wenet.copy()
    bad["n_mels"] = 200
    for b, kw in ((batch, dict(rate=24000, mono=True)), (batch, dict(rate=48000, mono=True)), (batch, dict(resample=22050, mono=True)),
                  (batch, dict(rate=16000, resample=16000, mono=True)), (batch, dict(rate=44100, mono=True)), (batch, dict(resample=(3, 1), mono=True)),
                  (batch, dict(format="s16", mono=True)), (batch, dict(format="f32_planar", mono=True)), (batch, dict()), (batch, dict(mix="stereo")),
                  (batch, dict(mix=np.eye(2))), (batch, dict(mix="mono", mono=True)), (six, dict(mono=True)),
                  (six, dict(mono=True, allow_mono=False)), (batch, dict(mono=True, allow_mono=False)), (six, dict(mix="stereo")),
                  (batch, dict(mono=True, scale=[np.nan] * batch.n_files)), (batch, dict(mono=True, scale=np.ones(batch.n_files + 1))),
                  (batch, dict(mono=True, out=Tensor(total - 1))), (batch, dict(mono=True, out=Tensor(total, dtype="torch.int16"))),
                  (batch, dict(mono=True, out=Tensor(total, ptr=4096 + 64))), (batch, dict(mono=True, out=Tensor(total), device=1))):
        with pytest.raises(ValueError):
            pkg.track_kaldi_args(b, wenet, **kw)
    for features in (bad, pkg.mel_params(80), pkg.mel_spec(16000, 512, 160), "logmel", None, np.zeros(2, dtype=pkg.FBANK_PARAMS_DTYPE)):
        with pytest.raises(ValueError):
            pkg.track_kaldi_args(batch, features, mono=True)
    assert pkg.track_kaldi_args(batch, wenet, mono=True, out=Tensor(total))[6] is not None
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for features, kw in ((wenet, dict(rate=24000, mono=True)), (wenet, dict(format="s16", mono=True)), (wenet, dict(mix=np.eye(2))), (wenet, dict()),
                         (wenet, dict(mono=True, out=Tensor(total - 1))), (wenet, dict(mono=True, mix="mono")), (at22k, dict(rate=16000, mono=True)),
                         (at22k, dict(resample=44100, mono=True)), (bad, dict(mono=True)), (wenet, dict(rate=16000, resample=16000, mono=True)),
                         (wenet, dict(mono=True, loudness="loud")), (mfcc, dict(rate=16000, mono=True))):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, features=features, **kw)
    ms = pkg.MultistreamContext.__new__(pkg.MultistreamContext)
    ms.h, ms.device = None, 0
    for kw in (dict(mix="stereo"), dict(), dict(mix="mono", rate=8000), dict(mix="mono", format="s16"), dict(mix="mono", out=Tensor(3))):
        with pytest.raises(ValueError):
            ms.decode_files(None, batch=six, features=wenet, **kw)


# ---- files_request ------------------------------------------------------------------------------------------
MIX, PARAMS, REFUSED = "mix record", "params record", None
REQUESTS = [
    (dict(features="wenet", mono=True), ("files_decode_fbank", (16000, 0, 0, 1, None, PARAMS), 1, "features"), REFUSED),
    (dict(features="wenet", rate=16000, mono=True, scale="ones"), ("files_decode_fbank", (16000, 0, 0, 1, None, PARAMS), 1, "features"), REFUSED),
    (dict(features="mfcc8k", mix="mono"),
     ("files_decode_fbank", (8000, 0, 0, 0, MIX, PARAMS), 1, "features"), ("files_decode_fbank", (8000, 0, 0, MIX, PARAMS), 1, "features")),
    (dict(features="22050", mono=True), ("files_decode_fbank", (0, 147, 320, 1, None, PARAMS), 1, "features"), REFUSED),
    (dict(features="22050", resample=22050, mix="mono"),
     ("files_decode_fbank", (0, 147, 320, 0, MIX, PARAMS), 1, "features"), ("files_decode_fbank", (0, 147, 320, MIX, PARAMS), 1, "features")),
    (dict(features="wenet", resample=16000, mix="mono", loudness=-23.0),
     ("files_decode_fbank", (0, 1, 3, 0, MIX, PARAMS), 1, "features"), ("files_decode_fbank", (0, 1, 3, MIX, PARAMS), 1, "features")),
    (dict(features="wide", mix="mono", loudness="measure"),
     ("files_decode_fbank", (48000, 0, 0, 0, MIX, PARAMS), 1, "features"), ("files_decode_fbank", (48000, 0, 0, MIX, PARAMS), 1, "features")),
]


@pytest.mark.parametrize("row", range(len(REQUESTS)))
def test_files_request_rows(pkg, batch, ms_batch, row):
    kw, *want = REQUESTS[row]
    kw = dict(kw)
    name = kw["features"]
    kw["features"] = pkg.kaldi_fbank(sample_rate=22050) if name == "22050" else spec_of(pkg, name)
    for b, multistream, expected in ((batch, False, want[0]), (ms_batch, True, want[1])):
        k = dict(kw)
        if k.get("scale") == "ones":
            k["scale"] = np.ones(b.n_files)
        if expected is REFUSED:
            assert k.get("mono")  # a multistream decoder has no mono downmix
            with pytest.raises(ValueError):
                pkg.files_request(b, multistream, 0, **k)
            continue
        req = pkg.files_request(b, multistream, 0, **k)  # no decoder anywhere

        def shown(a):
            if isinstance(a, np.ndarray):
                assert a.shape == (1,) and a.dtype in (pkg.MIX_MATRIX_DTYPE, pkg.FBANK_PARAMS_DTYPE)
                return MIX if a.dtype == pkg.MIX_MATRIX_DTYPE else PARAMS
            assert a is None or type(a) is int
            return a
        assert (req.entry, tuple(shown(a) for a in req.args), req.channels, req.kind) == expected
        assert hasattr(pkg.load_lib(), ("opusgpu_ms_" if multistream else "opusgpu_") + req.entry)
        assert (req.mix is not None) == (MIX in expected[1]) and np.array_equal(req.params, kw["features"])
        assert req.out is None and len(req.offsets) == len(req.planes) == b.n_files and req.fmt == pkg.TRACKS_F32
        assert (req.scale is not None) == ("scale" in k) and (req.scale is None or req.scale.dtype == np.float32)
        assert (req.loudness is not None) == ("loudness" in k)
        how = expected[1][:3]
        up, down = (1, 48000 // how[0]) if how[0] else how[1:]
        offs, planes, total = pkg.fbank_layout(b.info["track_samples"], up, down, kw["features"])
        assert np.array_equal(req.offsets, offs) and np.array_equal(req.planes, planes) and req.total == total
    total = pkg.files_request(batch, False, 0, features=kw["features"], mix="mono").total
    assert pkg.files_request(batch, False, 0, features=kw["features"], mix="mono", out=Tensor(max(total, 1))).out is not None
    with pytest.raises(ValueError):
        pkg.files_request(batch, False, 0, features=kw["features"], mix="mono", out=Tensor(max(total, 1) - 1))


def test_other_requests_are_what_they_were(pkg, batch):
    """features=None, "logmel" and mel_spec records take the entries they took."""
    assert pkg.files_request(batch).entry == "files_decode"
    assert pkg.files_request(batch, features="logmel", mono=True).entry == "files_decode_mel"
    assert pkg.files_request(batch, features=pkg.mel_spec(16000, 512, 160, 400), mono=True).entry == "files_decode_melspec"
    assert pkg.files_request(batch, resample=22050).entry == "files_decode_ratio"


# ---- the kernel's resources ---------------------------------------------------------------------------------
def test_kernel_resources():
    """k_tracks_fbank, which holds the MFCC product too (there is no second kernel): no scratch, no static LDS -- a launch asks for
    its tile's window, at most the 65,536 bytes of 32,768 samples (TILES, held in test_symbols_and_records) -- and at most 256
    registers, vector and accumulation together: two waves per SIMD."""
    meta = _kernel_metadata()
    seen = [v for mangled, v in meta.items() if re.search(r"\d+k_tracks_fbank(P|E|v|$)", mangled)]
    print(seen)
    assert len(seen) == 1, sorted(meta)[:6]
    vgpr, scratch, lds = seen[0]
    assert vgpr <= 256 and scratch == 0 and lds == 0
    assert not [m for m in meta if "mfcc" in m.lower()]
