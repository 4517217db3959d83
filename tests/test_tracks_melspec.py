"""Mel spectrograms of the whole-file path (include/opusgpu.h, TRACK SPECTROGRAMS), what needs no GPU: the exported symbols and the
record, the tables against the header's formulas for the parameter sets of SETS, the layout helper, the refusals that the C calls
and decode_files raise before any device work, and the kernel's resources.  melspec_ref is the float64 numpy restatement of the
header's value that the GPU checks (tests/test_gpu_tracks_melspec.py) compare against; melspec_f32 is the same in float32 with the
library's tables, the yardstick their tolerance is taken from."""
import functools
import os
import re

import numpy as np
import pytest

from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_spec_basis", "opusgpu_spec_filterbank", "opusgpu_spec_layout", "opusgpu_tracks_melspec_device",
       "opusgpu_files_decode_melspec", "opusgpu_ms_files_decode_melspec"]
# (sr, n_fft, win, hop, n_mels, fmin, fmax, scale, norm, power, log, floor, frames); the tile in frames that spec_tile gives each:
# the largest of 128, 64, 32 with (T - 1) hop + n_fft <= 32768
SETS = {
    "tts": (22050, 1024, 1024, 256, 80, 0, 8000, "slaney", "slaney", 1, "ln", 1e-5, "torch"),                 # tile 64
    "kaldi": (16000, 512, 400, 160, 80, 20, 8000, "htk", None, 2, "ln", 1.1920929e-7, "torch"),               # tile 128
    "clap": (48000, 1024, 1024, 480, 64, 50, 14000, "htk", None, 2, "log10", 1e-10, "torch"),                 # tile 64
    "music": (44100, 2048, 1102, 441, 128, 0, 22050, "slaney", "slaney", 2, "log10", 1e-10, "torch"),         # tile 64
    "tiny": (8000, 64, 48, 24, 8, 0, 4000, "htk", None, 1, None, 0, "whisper"),                               # tile 128
    "whisper": (16000, 400, 400, 160, 80, 0, 8000, "slaney", "slaney", 2, "log10", 1e-10, "whisper"),         # tile 128
}
TILES = {"tts": 64, "kaldi": 128, "clap": 64, "music": 64, "tiny": 128, "whisper": 128, "wide": 32}
# not one of the six above gets the tile of 32 under a window of 32,768 samples: a seventh set, for the kernel alone, does -- its
# window of 31 * 1000 + 1024 samples is also the one that fills the LDS but for a few hundred places, rows of unequal length and all
MORE_SETS = {"wide": (32000, 1024, 1000, 1000, 40, 100, 12000, "htk", "slaney", 1, "log10", 1e-7, "torch")}


def spec_of(pkg, name, feature_layout="bands"):
    sr, n_fft, win, hop, n_mels, fmin, fmax, scale, norm, power, log, floor, frames = {**SETS, **MORE_SETS}[name]
    return pkg.mel_spec(sr, n_fft, hop, win, n_mels, fmin, fmax, scale, norm, power, log, floor, frames, feature_layout)


def tile_of(rec):
    hop, n_fft = int(rec["hop"][0]), int(rec["n_fft"][0])
    return next(T for T in (128, 64, 32) if (T - 1) * hop + n_fft <= 32768 or T == 32)


# ---- the header's formulas, in float64 ----------------------------------------------------------------------
def basis64(rec):
    """(Wc, Ws) [n_fft, n_fft / 2 + 1] in float64: w[i] cos(a), w[i] sin(a), a = 2 pi ((i k) mod n_fft) / n_fft."""
    n_fft, win = int(rec["n_fft"][0]), int(rec["win_length"][0]) or int(rec["n_fft"][0])
    left = (n_fft - win) // 2
    i, k = np.arange(n_fft)[:, None], np.arange(n_fft // 2 + 1)[None, :]
    inside = (i >= left) & (i < left + win)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * (i - left) / float(win))
    a = 2.0 * np.pi * ((i * k) % n_fft) / float(n_fft)
    return np.where(inside, w * np.cos(a), 0.0), np.where(inside, w * np.sin(a), 0.0)


def filterbank64(rec):
    """B [n_mels, n_fft / 2 + 1] in float64, as the header writes it out."""
    sr, n_fft, n_mels = int(rec["sample_rate"][0]), int(rec["n_fft"][0]), int(rec["n_mels"][0])
    fmin, fmax, htk = float(rec["fmin"][0]), float(rec["fmax"][0]), int(rec["mel_scale"][0]) == 1
    step = np.log(6.4) / 27.0

    def mel(f):
        if htk:
            return 2595.0 * np.log10(1.0 + f / 700.0)
        return 3.0 * f / 200.0 if f < 1000.0 else 15.0 + np.log(f / 1000.0) / step
    m0, m1 = mel(fmin), mel(fmax)
    m = m0 + np.arange(n_mels + 2) * ((m1 - m0) / (n_mels + 1))
    m[-1] = m1
    if htk:
        p = 700.0 * (np.power(10.0, m / 2595.0) - 1.0)
    else:
        p = np.where(m < 15.0, 200.0 / 3.0 * m, 1000.0 * np.exp(step * (m - 15.0)))
    fr = (sr / n_fft) * np.arange(n_fft // 2 + 1)[None, :]
    lo, ce, hi = p[:-2, None], p[1:-1, None], p[2:, None]
    w = np.maximum(0.0, np.minimum((fr - lo) / (ce - lo), (hi - fr) / (hi - ce)))
    return w * (2.0 / (hi - lo)) if int(rec["norm"][0]) == 0 else w


def frame_count(rec, n):
    hop = int(rec["hop"][0])
    return n // hop if int(rec["frames"][0]) == 1 else (n // hop + 1 if n else 0)


def frames_of(y, rec):
    """The windows of TRACK SPECTROGRAMS: y [n] -> (q [F, n_fft] reflected indices clipped into [0, n), inside [F, n_fft] bool)."""
    n, hop, n_fft = len(y), int(rec["hop"][0]), int(rec["n_fft"][0])
    F = frame_count(rec, n)
    q = hop * np.arange(F)[:, None] - n_fft // 2 + np.arange(n_fft)[None, :]
    q = np.where(q < 0, -q, np.where(q >= n, 2 * (n - 1) - q, q))  # reflected ONCE
    inside = (q >= 0) & (q < n)
    return np.clip(q, 0, max(n - 1, 0)), inside


@functools.lru_cache(maxsize=None)
def _tables64(key):
    rec = np.frombuffer(key, dtype=_tables64.dtype).copy()
    return (*basis64(rec), filterbank64(rec))


def tables64(rec):
    _tables64.dtype = rec.dtype
    return _tables64(rec.tobytes())


def melspec_ref(y, scale, rec, tables=None):
    """TRACK SPECTROGRAMS in float64: y int16 [n] -> (output [F, n_mels], mel [F, n_mels]).  The sample is the float32 product
    (float)y * scale, as the header says; everything behind it is float64 with float64 tables (tables: (Wc, Ws, B) to use others)."""
    y = np.asarray(y, dtype=np.int16)
    wc, ws, B = tables if tables is not None else tables64(rec)
    q, inside = frames_of(y, rec)
    x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
    fr = np.where(inside, x[q] if len(y) else 0.0, 0.0)
    S = (fr @ wc.astype(np.float64)) ** 2 + (fr @ ws.astype(np.float64)) ** 2
    if int(rec["power"][0]) == 1:
        S = np.sqrt(S)
    mel = S @ B.astype(np.float64).T
    v = np.maximum(mel, float(rec["floor"][0]))
    log = int(rec["log"][0])
    with np.errstate(divide="ignore"):
        return (v if log == 0 else np.log10(v) if log == 1 else np.log(v)), mel


def melspec_f32(y, scale, rec, wc, ws, B):
    """The same value in float32 throughout, with the library's float32 tables, summed in numpy's order: the yardstick for the
    kernel's tolerance (the kernel may differ from float64 by 8 x what this does)."""
    y = np.asarray(y, dtype=np.int16)
    q, inside = frames_of(y, rec)
    x = y.astype(np.float32) * np.float32(scale)
    fr = np.where(inside, x[q] if len(y) else np.float32(0), np.float32(0)).astype(np.float32)
    re, im = fr @ wc, fr @ ws
    assert re.dtype == np.float32
    S = re * re + im * im
    if int(rec["power"][0]) == 1:
        S = np.sqrt(S)
    v = np.maximum(S @ np.ascontiguousarray(B.T), rec["floor"][0])
    assert v.dtype == np.float32
    log = int(rec["log"][0])
    with np.errstate(divide="ignore"):
        return v if log == 0 else np.log10(v) if log == 1 else np.log(v)


def error_of(got, ref, rec):
    """The error the tolerance is held on: absolute for the log outputs, relative for log = none (absolute where the reference is 0)."""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return d if int(rec["log"][0]) else d / np.where(ref == 0, 1.0, np.abs(ref))


# ---- symbols, records, tables -------------------------------------------------------------------------------
def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "TRACK SPECTROGRAMS" in hdr and "opusgpu_spec_params { /* 64 bytes" in hdr
    d = pkg.SPEC_PARAMS_DTYPE
    assert d.itemsize == 64
    names = ["sample_rate", "n_fft", "win_length", "hop", "n_mels", "mel_scale", "norm", "power", "log", "frames", "layout", "fmin", "fmax",
             "floor", "reserved"]
    assert [(n, d.fields[n][1]) for n in d.names] == [(n, 4 * i) for i, n in enumerate(names)]
    assert d.fields["reserved"][0].shape == (2,) and d.fields["fmin"][0] == np.float32
    for name, value in (("SLANEY", 0), ("HTK", 1), ("NORM_SLANEY", 0), ("NORM_NONE", 1), ("LOG_NONE", 0), ("LOG10", 1), ("LN", 2),
                        ("FRAMES_TORCH", 0), ("FRAMES_WHISPER", 1)):
        assert re.search(rf"#define OPUSGPU_SPEC_{name} {value}\b", hdr), name
    rec = spec_of(pkg, "kaldi", "frames")
    assert [int(rec[n][0]) for n in names[:11]] == [16000, 512, 400, 160, 80, 1, 1, 2, 2, 0, 1]
    assert (float(rec["fmin"][0]), float(rec["fmax"][0]), rec["floor"][0]) == (20.0, 8000.0, np.float32(1.1920929e-7))
    assert float(pkg.mel_spec(44100, 1024, 256)["fmax"][0]) == 22050.0 and int(pkg.mel_spec(44100, 1024, 256)["win_length"][0]) == 1024
    assert {n: tile_of(spec_of(pkg, n)) for n in TILES} == TILES


@pytest.mark.parametrize("name", list(SETS) + list(MORE_SETS))
def test_tables_are_the_formulas_rounded_once(pkg, name):
    rec = spec_of(pkg, name)
    n_fft, n_mels = int(rec["n_fft"][0]), int(rec["n_mels"][0])
    wc, ws = pkg.spec_basis(rec)
    B = pkg.spec_filterbank(rec)
    assert wc.dtype == ws.dtype == B.dtype == np.float32 and wc.shape == ws.shape == (n_fft, n_fft // 2 + 1) and B.shape == (n_mels, n_fft // 2 + 1)
    want_c, want_s = basis64(rec)
    assert np.array_equal(wc.view(np.uint32), want_c.astype(np.float32).view(np.uint32))
    assert np.array_equal(ws.view(np.uint32), want_s.astype(np.float32).view(np.uint32))
    assert np.array_equal(B.view(np.uint32), filterbank64(rec).astype(np.float32).view(np.uint32))
    assert (B >= 0).all() and (B.max(axis=1) > 0).all()  # no set has an empty band
    # what the kernel's folding rests on: rows i and n_fft - i agree but for the rounding of the double cosines behind them
    h = n_fft // 2
    assert (wc[0] == 0).all() and (ws[0] == 0).all()
    assert np.abs(wc[1:h] - wc[:h:-1]).max() <= 2.0 ** -23 and np.abs(ws[1:h] + ws[:h:-1]).max() <= 2.0 ** -23
    lib = pkg.load_lib()
    assert lib.opusgpu_spec_basis(rec.ctypes.data, None, None) == wc.size and lib.opusgpu_spec_filterbank(rec.ctypes.data, None) == B.size
    # the blocks of 32 bins that no band weights: what the kernel leaves out
    kept = [nb for nb in range((n_fft // 2 + 32) // 32) if B[:, 32 * nb:32 * nb + 32].any()]
    print(name, "tile", tile_of(rec), "bin blocks kept", len(kept), "of", (n_fft // 2 + 32) // 32)
    if name == "tts":
        assert (len(kept), (n_fft // 2 + 32) // 32) == (12, 17)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_whispers_tables_are_the_logmel_tables(pkg, n_mels):
    for win in (None, 400):
        rec = pkg.mel_spec(16000, 400, 160, win, n_mels, 0.0, 8000.0, "slaney", "slaney", 2, "log10", 1e-10, "whisper")
        wc, ws = pkg.spec_basis(rec)
        mc, ms = pkg.mel_basis()
        assert np.array_equal(wc.view(np.uint32), mc.view(np.uint32)) and np.array_equal(ws.view(np.uint32), ms.view(np.uint32))
        assert np.array_equal(pkg.spec_filterbank(rec).view(np.uint32), pkg.mel_filterbank(n_mels).view(np.uint32))
    rec["win_length"] = 0  # the C record's "0 means n_fft"
    assert np.array_equal(pkg.spec_basis(rec)[0].view(np.uint32), pkg.mel_basis()[0].view(np.uint32))


def test_layout_helper(pkg):
    planned = np.array([0, 1, 479, 480, 481, 3 * 160 * 64, 3 * 160 * 64 - 3, 0, 7, 48000 * 3 + 5], dtype=np.int64)
    for name, up, down in (("whisper", 1, 3), ("kaldi", 1, 3), ("tts", 147, 320), ("music", 147, 160), ("clap", 1, 1), ("tiny", 1, 6)):
        for layout in ("bands", "frames"):
            rec = spec_of(pkg, name, layout)
            n_mels, hop = int(rec["n_mels"][0]), int(rec["hop"][0])
            n = -(-planned * up // down)
            F = n // hop if name in ("whisper", "tiny") else np.where(n > 0, n // hop + 1, 0)
            plane = (F + 63) // 64 * 64
            offs, planes, total = pkg.spec_layout(planned, up, down, rec)
            want = np.concatenate([[0], np.cumsum(n_mels * plane)])
            assert np.array_equal(planes, plane) and np.array_equal(offs, want[:-1]) and total == want[-1] and (offs % 64 == 0).all()
            assert np.array_equal(pkg.spec_frames(rec, n), F)
    torch_rec, whisper_rec = (pkg.mel_spec(16000, 400, 160, frames=f) for f in ("torch", "whisper"))
    n = np.array([0, 1, 159, 160, 161, 16000], dtype=np.int64)
    assert list(pkg.spec_frames(whisper_rec, n)) == [0, 0, 0, 1, 1, 100] and list(pkg.spec_frames(torch_rec, n)) == [0, 1, 1, 2, 2, 101]
    assert np.array_equal(pkg.spec_layout(planned, 1, 3, whisper_rec)[1], pkg.mel_layout(planned, 80, "bands")[1])  # TRACK FEATURES' grid
    offs, planes, total = pkg.spec_layout([], 1, 3, torch_rec)
    assert len(offs) == 0 and total == 0
    lib = pkg.load_lib()
    BAD = pkg.OPUSGPU_BAD_ARG
    ok = torch_rec.ctypes.data
    assert lib.opusgpu_spec_layout(planned.size, planned.ctypes.data, 1, 3, ok, None) == pkg.spec_layout(planned, 1, 3, torch_rec)[2]
    for up, down in ((0, 3), (3, 1), (1, 0), (-1, 3), (1, 48001)):
        assert lib.opusgpu_spec_layout(planned.size, planned.ctypes.data, up, down, ok, None) == BAD
    assert lib.opusgpu_spec_layout(2, planned.ctypes.data, 1, 3, None, None) == BAD and lib.opusgpu_spec_layout(-1, planned.ctypes.data, 1, 3, ok, None) == BAD
    assert lib.opusgpu_spec_layout(2, None, 1, 3, ok, None) == BAD
    with pytest.raises(ValueError):
        pkg.spec_layout([5, -1], 1, 3, torch_rec)
    with pytest.raises(ValueError):
        pkg.spec_layout(planned, 1, 3, pkg.mel_params(80))  # TRACK FEATURES' record is another record


def test_reference_by_hand(pkg):
    """melspec_ref on cases small enough to work out: the frame counts, the reflection at both ends and the "still outside" zero,
    a window shorter than the frame, a tone in its band with both powers, the floor."""
    tiny, kaldi = spec_of(pkg, "tiny"), spec_of(pkg, "kaldi")
    for n, F in ((0, 0), (23, 0), (24, 1), (47, 1), (48, 2)):
        assert melspec_ref(np.zeros(n, dtype=np.int16), 1.0, tiny)[0].shape == (F, 8)
    for n, F in ((0, 0), (1, 1), (159, 1), (160, 2), (161, 2)):
        assert melspec_ref(np.zeros(n, dtype=np.int16), 1.0, kaldi)[0].shape == (F, 80)
    y = np.arange(1000, 1500, dtype=np.int16)
    q, inside = frames_of(y, kaldi)  # n_fft 512, hop 160: 4 frames, the last centred on sample 480
    assert q.shape == (4, 512) and inside.all() and list(q[0, :3]) == [256, 255, 254] and q[0, 256] == 0 and q[0, 511] == 255
    assert q[3, 256] == 480 and q[3, 275] == 499 and q[3, 276] == 498 and q[3, 511] == 2 * 499 - (480 + 255)
    q, inside = frames_of(np.zeros(100, dtype=np.int16), kaldi)  # one frame, mostly reflections that stay outside
    assert q.shape == (1, 512) and list(q[0, 255:258]) == [1, 0, 1] and not inside[0, :157].any() and inside[0, 157:455].all() and not inside[0, 455:].any()
    wc, _ = basis64(kaldi)
    assert (wc[:56] == 0).all() and (wc[456:] == 0).all() and wc[256, 0] == 1.0 and wc[57, 0] > 0  # 400 taps centred in 512
    t = np.arange(16000)
    tone = np.round(8000 * np.sin(2 * np.pi * 1000.0 / 16000 * t)).astype(np.int16)  # 1 kHz: bin 32 of 512
    out, mel = melspec_ref(tone, 1.0 / 32768, kaldi)
    B = filterbank64(kaldi)
    want = int(np.argmax(B[:, 32]))
    assert (mel[3:-3].argmax(axis=1) == want).all() and np.array_equal(out, np.log(np.maximum(mel, float(kaldi["floor"][0]))))
    mag = kaldi.copy()
    mag["power"] = 1
    _, mel1 = melspec_ref(tone, 1.0 / 32768, mag)
    amp = 8000 / 32768 * 100  # |X[32]| = amplitude * sum(w) / 2, and sum(w) is 200 for 400 taps
    assert (mel1[3:-3, want] >= B[want, 32] * amp * 0.999).all()                            # the tone's bin alone
    assert (mel1[3:-3, want] ** 2 <= B[want].sum() * mel[3:-3, want] * (1 + 1e-12)).all()   # Cauchy-Schwarz over the band's bins
    zero, _ = melspec_ref(np.zeros(800, dtype=np.int16), 1.0, spec_of(pkg, "tts"))
    assert zero.shape == (4, 80) and (zero == np.log(float(np.float32(1e-5)))).all()
    assert (melspec_ref(np.zeros(100, dtype=np.int16), 1.0, tiny)[0] == 0).all()


def test_float32_restatement_is_close(pkg):
    """The yardstick of the GPU test's tolerance on one white-noise track per set: float32 with the library's tables against float64."""
    rng = np.random.default_rng(1)
    for name in SETS:
        rec = spec_of(pkg, name)
        y = rng.integers(-32768, 32768, int(rec["hop"][0]) * 40 + 7, dtype=np.int16)
        ref, mel = melspec_ref(y, 2.0 ** -15, rec)
        keep = mel >= 1e-8 * mel.max(axis=1, keepdims=True)
        assert keep.all(), name  # on uniform noise the reference leaves out no cell
        err = error_of(melspec_f32(y, 2.0 ** -15, rec, *pkg.spec_basis(rec), pkg.spec_filterbank(rec)), ref, rec)[keep].max()
        print(name, "float32 restatement: max error =", err)
        assert err < 1e-3


# ---- refusals before any device work ------------------------------------------------------------------------
def bad_records(pkg):
    """Records that break one rule of opusgpu_spec_params each."""
    good = pkg.mel_spec(16000, 512, 160, 400, 80, 20.0, 8000.0, "htk", None, 2, "ln", 1e-7)

    def but(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    return good, [but(n_fft=48), but(n_fft=2064), but(n_fft=520), but(n_fft=4096), but(win_length=14), but(win_length=401), but(win_length=514),
                  but(win_length=-2), but(hop=0), but(hop=513), but(hop=-160), but(n_fft=2048, win_length=0, hop=991), but(n_mels=0),
                  but(n_mels=129), but(mel_scale=2), but(mel_scale=-1), but(norm=2), but(power=0), but(power=3), but(log=3), but(log=-1),
                  but(frames=2), but(layout=2), but(layout=-1), but(fmin=-1.0), but(fmin=8000.0), but(fmax=8000.5), but(fmin=np.nan),
                  but(fmax=np.nan), but(floor=0.0), but(floor=-1.0), but(floor=np.inf), but(floor=np.nan), but(log=0, floor=-0.5),
                  but(sample_rate=0), but(reserved=[1, 0]), but(reserved=[0, 7])]


def test_mel_spec_refuses(pkg):
    assert int(pkg.mel_spec(32000, 2048, 990)["hop"][0]) == 990  # 31 * 990 + 2048 = 32738
    assert pkg.mel_spec(8000, 64, 24, 48, 8, 0, 4000, "htk", None, 1, None, 0, "whisper")["floor"][0] == 0
    for kw in (dict(n_fft=48), dict(n_fft=520), dict(n_fft=4096), dict(n_fft=512.0), dict(win_length=14), dict(win_length=401), dict(win_length=600),
               dict(hop=0), dict(hop=513), dict(n_fft=2048, hop=991), dict(n_mels=0), dict(n_mels=129), dict(n_mels=True), dict(mel_scale="mel"),
               dict(mel_scale=1), dict(norm="l2"), dict(power=3), dict(power=2.5), dict(log="log2"), dict(log=1), dict(frames="librosa"),
               dict(feature_layout="planar"), dict(fmin=-1), dict(fmin=8000), dict(fmax=8001), dict(fmax="x"), dict(floor=0), dict(floor=-1),
               dict(floor=float("inf")), dict(log=None, floor=float("nan")), dict(sample_rate=0), dict(sample_rate=16000.0)):
        args = {"sample_rate": 16000, "n_fft": 512, "hop": 160, **kw}
        with pytest.raises(ValueError):
            pkg.mel_spec(**args)
    lib = pkg.load_lib()
    good, bad = bad_records(pkg)
    planned = np.array([480, 960], dtype=np.int64)
    assert lib.opusgpu_spec_basis(good.ctypes.data, None, None) == 512 * 257 and lib.opusgpu_spec_basis(None, None, None) == pkg.OPUSGPU_BAD_ARG
    for rec in bad:
        assert lib.opusgpu_spec_basis(rec.ctypes.data, None, None) == pkg.OPUSGPU_BAD_ARG, rec
        assert lib.opusgpu_spec_filterbank(rec.ctypes.data, None) == pkg.OPUSGPU_BAD_ARG
        assert lib.opusgpu_spec_layout(2, planned.ctypes.data, 1, 3, rec.ctypes.data, None) == pkg.OPUSGPU_BAD_ARG
        for call in (pkg.spec_basis, pkg.spec_filterbank, lambda r: pkg.spec_layout(planned, 1, 3, r)):
            with pytest.raises(ValueError):
                call(rec)


def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """Every refusal of the three calls comes back as OPUSGPU_BAD_ARG with d_in / d_out NULL and -- without a device -- from a decoder
    that does not exist (`handles` of tests/test_tracks_resample.py).  A call that got as far as the device would fail otherwise."""
    lib = pkg.load_lib()
    n = batch.n_files
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    good, bad = bad_records(pkg)  # a record for tracks at 16000 Hz
    tts = pkg.mel_spec(22050, 1024, 256)
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)
    inf = np.array([np.inf] + [1] * (n - 1), dtype=np.float32)
    mono_mix = pkg.mix_matrix("mono", 2)
    two_rows = pkg.mix_matrix(np.eye(2, dtype=np.int16) * 16384, 2)
    six_mono, six_stereo = pkg.mix_matrix("mono", 6), pkg.mix_matrix("stereo", 6)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]

    def files(rate, up, down, mono, mix, p, scale, ctx=fake, b=batch.h, out=None):
        return lib.opusgpu_files_decode_melspec(ctx, b, rate, up, down, mono, None if mix is None else mix.ctypes.data,
                                                None if p is None else p.ctypes.data, None if scale is None else scale.ctypes.data, out,
                                                *[a.ctypes.data for a in arrays])

    def ms_files(rate, up, down, mix, p, scale, ms=fake_ms, b=ms_batch.h):
        return lib.opusgpu_ms_files_decode_melspec(ms, b, rate, up, down, None if mix is None else mix.ctypes.data,
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
    assert files(0, 147, 320, 1, None, good, None) == BAD and files(16000, 0, 0, 1, None, tts, None) == BAD and ms_files(0, 147, 160, six_mono, tts, None) == BAD
    odd = pkg.mel_spec(6857, 512, 160)  # 48000 / 7 = 6857.14...: a ratio whose rate is no integer
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
    spans["in_offset"], spans["out_offset"] = [0, 408], [0, 64 * 80]

    def kernel(s, p, ctx=fake):
        return lib.opusgpu_tracks_melspec_device(ctx, len(s), s.ctypes.data, None, None if p is None else p.ctypes.data, None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    assert kernel(spans, good, ctx=None) == BAD and kernel(spans, None) == BAD
    for p in bad:
        assert kernel(spans, p) == BAD
    for s in (but(in_offset=4), but(in_offset=-8), but(in_samples=-1), but(out_offset=32), but(out_offset=-64), but(plane=32),
              but(in_samples=160 * 64), but(scale=np.nan), but(scale=-np.inf), but(reserved=1)):  # 160 * 64 samples: 65 frames in a plane of 64
        assert kernel(s, good) == BAD
    assert kernel(spans, good) == BAD  # these spans are in order: refused for the NULL buffers, still before the device
    none = spans.copy()
    none["in_samples"] = 0
    assert kernel(none, good) == 0 and kernel(spans[:0], good) == 0  # no frame is no error, and no device work
    whisper = good.copy()
    whisper["frames"] = 1
    short = spans.copy()
    short["in_samples"] = [159, 0]
    assert kernel(short, whisper) == 0 and kernel(short, good) == BAD  # F = n / hop + 1 has a frame there


def C_VOID(v):
    import ctypes
    return ctypes.c_void_p(v)


def test_decode_files_refusals_need_no_device(pkg, batch):
    """track_spectrogram_args, and decode_files raising before it touches its decoder (an object without one is enough to see it);
    track_feature_args and track_ratio_args refuse of strings what they did."""
    kaldi, tts, clap = spec_of(pkg, "kaldi"), spec_of(pkg, "tts", "frames"), spec_of(pkg, "clap")
    rec, mrec, scale, offs, planes, total, out, how = pkg.track_spectrogram_args(batch, kaldi, rate=16000, mono=True)
    assert rec is not kaldi and np.array_equal(rec, kaldi) and (mrec, scale, out, how) == (None, None, None, (16000, 0, 0))
    assert total == pkg.spec_layout(batch.info["track_samples"], 1, 3, kaldi)[2] > 0 and len(offs) == len(planes) == batch.n_files
    assert pkg.track_spectrogram_args(batch, kaldi, mono=True)[7] == (16000, 0, 0)        # neither: the record's rate is one of TRACK RATES
    assert pkg.track_spectrogram_args(batch, tts, mono=True)[7] == (0, 147, 320)           # or a ratio of TRACK RATIOS
    assert pkg.track_spectrogram_args(batch, tts, resample=(294, 640), mix="mono")[7] == (0, 147, 320)
    assert pkg.track_spectrogram_args(batch, kaldi, resample=16000, mono=True)[7] == (0, 1, 3)  # the ratio's filter, if asked for
    got = pkg.track_spectrogram_args(batch, clap, 48000, None, False, "mono", "f32", np.ones(batch.n_files))
    assert got[7] == (48000, 0, 0) and int(got[1]["out_channels"][0]) == 1 and got[2].dtype == np.float32
    six = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files, "track_samples": batch.track_samples})()
    assert pkg.track_spectrogram_args(six, tts, mix="mono", allow_mono=False)[1]["in_channels"][0] == 6
    bad = kaldi.copy()
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
            pkg.track_spectrogram_args(b, kaldi, **kw)
    for features in (bad, pkg.mel_params(80), "logmel", None, np.zeros(2, dtype=pkg.SPEC_PARAMS_DTYPE)):
        with pytest.raises(ValueError):
            pkg.track_spectrogram_args(batch, features, mono=True)
    assert pkg.track_spectrogram_args(batch, kaldi, mono=True, out=Tensor(total))[6] is not None
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for features, kw in ((kaldi, dict(rate=24000, mono=True)), (kaldi, dict(format="s16", mono=True)), (kaldi, dict(mix=np.eye(2))), (kaldi, dict()),
                         (kaldi, dict(mono=True, out=Tensor(total - 1))), (kaldi, dict(mono=True, mix="mono")), (tts, dict(rate=16000, mono=True)),
                         (tts, dict(resample=44100, mono=True)), (bad, dict(mono=True)), (kaldi, dict(rate=16000, resample=16000, mono=True))):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, features=features, **kw)
    ms = pkg.MultistreamContext.__new__(pkg.MultistreamContext)
    ms.h, ms.device = None, 0
    for kw in (dict(mix="stereo"), dict(), dict(mix="mono", rate=8000), dict(mix="mono", format="s16"), dict(mix="mono", out=Tensor(3))):
        with pytest.raises(ValueError):
            ms.decode_files(None, batch=six, features=kaldi, **kw)
    # the string features keep their refusals: other rates, other band counts, other names, resample= next to them
    for kw in (dict(features="logmel", rate=24000, mono=True), dict(features="logmel", n_mels=64, mono=True), dict(features="mfcc", mono=True)):
        with pytest.raises(ValueError):
            pkg.track_feature_args(batch, **kw)
    with pytest.raises(ValueError):
        pkg.track_ratio_args(batch, 22050, mono=True, features="logmel")
    with pytest.raises(ValueError):
        ctx.decode_files(None, batch=batch, features="logmel", resample=22050, mono=True)


def test_kernel_resources():
    """k_tracks_melspec: no scratch (the accumulators are indexed by literals only), no static LDS -- a launch asks for its tile's
    window, at most the 65,536 bytes of the 32,768 samples that the record's rules and the tile choice allow (TILES, held in
    test_symbols_and_records) -- and at most 256 registers, vector and accumulation together: two waves per SIMD."""
    meta = _kernel_metadata()
    seen = [v for mangled, v in meta.items() if re.search(r"\d+k_tracks_melspec(P|E|v|$)", mangled)]
    print(seen)
    assert len(seen) == 1, sorted(meta)[:6]
    vgpr, scratch, lds = seen[0]
    assert vgpr <= 256 and scratch == 0 and lds <= 65536
    assert lds == MEASURED_RESOURCES[1]  # (the register count is the compiler's to move below 256)


MEASURED_RESOURCES = (252, 0)  # (registers, static LDS bytes) of the code object, as tools/kernel_meta.py prints them
