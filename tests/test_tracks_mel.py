"""Log-mel features of the whole-file path (include/opusgpu.h, TRACK FEATURES), what needs no GPU: the exported symbols and the
records, the tables against the header's formulas, the layout helper, and the refusals that the C calls and decode_files raise
before any device work.  logmel_ref is the float64 numpy restatement of the header's value that the GPU checks
(tests/test_gpu_tracks_mel.py) compare against; logmel_f32 is the same in float32 with the library's tables, the yardstick their
tolerance is taken from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_mel_basis", "opusgpu_mel_filterbank", "opusgpu_mel_layout", "opusgpu_tracks_mel_device", "opusgpu_files_decode_mel",
       "opusgpu_ms_files_decode_mel"]
N_FFT, HOP, BINS = 400, 160, 201


# ---- the header's formulas, in float64 ----------------------------------------------------------------------
def basis64():
    """(Wc, Ws) [400, 201] in float64: w[i] cos(a), w[i] sin(a), a = 2 pi ((i k) mod 400) / 400."""
    i, k = np.arange(N_FFT)[:, None], np.arange(BINS)[None, :]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * i / 400.0)
    a = 2.0 * np.pi * ((i * k) % 400) / 400.0
    return w * np.cos(a), w * np.sin(a)


def filterbank64(n_mels):
    """Slaney's filterbank [n_mels, 201] in float64, as the header writes it out."""
    step = np.log(6.4) / 27.0
    mmax = 15.0 + np.log(8000.0 / 1000.0) / step
    m = np.arange(n_mels + 2) * (mmax / (n_mels + 1))
    m[-1] = mmax
    p = np.where(m < 15.0, 200.0 / 3.0 * m, 1000.0 * np.exp(step * (m - 15.0)))
    fr = 40.0 * np.arange(BINS)[None, :]
    lo, ce, hi = p[:-2, None], p[1:-1, None], p[2:, None]
    w = np.maximum(0.0, np.minimum((fr - lo) / (ce - lo), (hi - fr) / (hi - ce)))
    return w * (2.0 / (hi - lo))


def frames_of(y):
    """The windows of TRACK FEATURES: y [n] -> (q [F, 400] reflected indices clipped into [0, n), inside [F, 400] bool)."""
    n = len(y)
    F = n // HOP
    q = HOP * np.arange(F)[:, None] - 200 + np.arange(N_FFT)[None, :]
    q = np.where(q < 0, -q, np.where(q >= n, 2 * (n - 1) - q, q))  # reflected ONCE
    inside = (q >= 0) & (q < n)
    return np.clip(q, 0, max(n - 1, 0)), inside


def logmel_ref(y, scale, n_mels, tables=None):
    """TRACK FEATURES in float64: y int16 [n] -> (log10(max(mel, 1e-10)) [F, n_mels], mel [F, n_mels]).  The sample is the float32
    product (float)y * scale, as the header says; everything behind it is float64 with float64 tables (tables: (Wc, Ws, B) to use
    others, e.g. the library's float32 ones)."""
    y = np.asarray(y, dtype=np.int16)
    wc, ws, B = tables if tables is not None else (*basis64(), filterbank64(n_mels))
    q, inside = frames_of(y)
    x = (y.astype(np.float32) * np.float32(scale)).astype(np.float64)
    fr = np.where(inside, x[q] if len(y) else 0.0, 0.0)
    P = (fr @ wc.astype(np.float64)) ** 2 + (fr @ ws.astype(np.float64)) ** 2
    mel = P @ B.astype(np.float64).T
    return np.log10(np.maximum(mel, 1e-10)), mel


def logmel_f32(y, scale, n_mels, wc, ws, B):
    """The same value in float32 throughout, with the library's float32 tables, summed in numpy's order: the yardstick for the
    kernel's tolerance (the kernel may differ from float64 by 8 x what this does)."""
    y = np.asarray(y, dtype=np.int16)
    q, inside = frames_of(y)
    x = y.astype(np.float32) * np.float32(scale)
    fr = np.where(inside, x[q] if len(y) else np.float32(0), np.float32(0)).astype(np.float32)
    re, im = fr @ wc, fr @ ws
    assert re.dtype == np.float32
    mel = (re * re + im * im) @ np.ascontiguousarray(B.T)
    return np.log10(np.maximum(mel, np.float32(1e-10)))


# ---- symbols, records, tables -------------------------------------------------------------------------------
def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "TRACK FEATURES" in hdr
    d = pkg.MEL_SPAN_DTYPE
    assert d.itemsize == 40 and "opusgpu_mel_span { /* 40 bytes" in hdr
    assert [(n, d.fields[n][1]) for n in d.names] == [("in_offset", 0), ("in_samples", 8), ("out_offset", 16), ("plane", 24), ("scale", 32),
                                                      ("reserved", 36)]
    assert pkg.MEL_PARAMS_DTYPE.itemsize == 32 and "opusgpu_mel_params { /* 32 bytes" in hdr
    for name, value in (("NFFT", 400), ("HOP", 160), ("SR", 16000), ("FMIN", 0), ("FMAX", 8000), ("BINS", 201)):
        assert re.search(rf"#define OPUSGPU_MEL_{name} {value}\b", hdr), name
    assert (pkg.MEL_NFFT, pkg.MEL_HOP, pkg.MEL_SR, pkg.MEL_BINS) == (400, 160, 16000, 201)


def test_basis_is_the_formula_rounded_once(pkg):
    wc, ws = pkg.mel_basis()
    assert wc.dtype == ws.dtype == np.float32 and wc.shape == ws.shape == (400, 201)
    want_c, want_s = basis64()
    assert np.array_equal(wc.view(np.uint32), want_c.astype(np.float32).view(np.uint32))
    assert np.array_equal(ws.view(np.uint32), want_s.astype(np.float32).view(np.uint32))
    assert pkg.load_lib().opusgpu_mel_basis(None, None) == 400 * 201
    assert (wc[0] == 0).all() and (ws[0] == 0).all() and wc[200, 0] == 1.0 and wc[200, 1] == -1.0  # w[0] = 0, w[200] = 1
    # what the kernel's folding rests on: rows i and 400 - i agree but for the rounding of the double cosines behind them
    assert np.abs(wc[1:200] - wc[:200:-1]).max() <= 2.0 ** -23 and np.abs(ws[1:200] + ws[:200:-1]).max() <= 2.0 ** -23


@pytest.mark.parametrize("n_mels", [80, 128])
def test_filterbank_is_slaneys(pkg, n_mels):
    B = pkg.mel_filterbank(n_mels)
    assert B.dtype == np.float32 and B.shape == (n_mels, 201)
    assert np.array_equal(B.view(np.uint32), filterbank64(n_mels).astype(np.float32).view(np.uint32))
    assert (B >= 0).all() and (B.max(axis=1) > 0).all()
    peak = B.argmax(axis=1)
    assert (np.diff(peak) >= 0).all() and peak[0] <= 2 and peak[-1] >= 190  # bands in order, over the whole of [0, 8000] Hz
    assert (B[:, 0] == 0).all() and (B[:, 200] == 0).all()                    # fmin and fmax are the outermost points
    # Slaney's normalisation: a triangle's area is 1 in Hz, so a band that spans many bins sums to about 1 / 40 per Hz-bin
    assert abs(B[-1].sum() * 40.0 - 1.0) < 0.02
    assert pkg.load_lib().opusgpu_mel_filterbank(n_mels, None) == n_mels * 201


def test_filterbank_of_other_sizes(pkg):
    for n in (64, 0, 81, -80, 256):
        assert pkg.load_lib().opusgpu_mel_filterbank(n, None) == pkg.OPUSGPU_BAD_ARG
        with pytest.raises(ValueError):
            pkg.mel_filterbank(n)


def test_layout_helper(pkg):
    planned = np.array([0, 1, 479, 480, 481, 3 * 160 * 64, 3 * 160 * 64 + 1, 0, 7], dtype=np.int64)
    frames = -(-planned // 3) // 160
    assert list(frames[:7]) == [0, 0, 1, 1, 1, 64, 64]  # ceil(479 / 3) = 160: one frame
    plane = (frames + 63) // 64 * 64
    assert list(plane[:7]) == [0, 0, 64, 64, 64, 64, 64]
    more = np.array([3 * 160 * 65 - 2], dtype=np.int64)  # ceil(n / 3) = 160 * 65: the 65th frame, the second 64
    assert pkg.mel_layout(more, 80, "bands")[1][0] == 128
    for n_mels in (80, 128):
        for layout in ("bands", "frames"):
            offs, planes, total = pkg.mel_layout(planned, n_mels, layout)
            want = np.concatenate([[0], np.cumsum(n_mels * plane)])
            assert np.array_equal(planes, plane) and np.array_equal(offs, want[:-1]) and total == want[-1] and (offs % 64 == 0).all()
            assert offs[1] == offs[2] == 0 and offs[3] == 64 * n_mels and offs[8] == offs[7]  # a track without a frame takes no room
    offs, planes, total = pkg.mel_layout([], 80, "frames")
    assert len(offs) == 0 and total == 0
    lib = pkg.load_lib()
    rec = pkg.mel_params(128, "frames")
    assert lib.opusgpu_mel_layout(planned.size, planned.ctypes.data, rec.ctypes.data, None) == pkg.mel_layout(planned, 128, "frames")[2]
    with pytest.raises(ValueError):
        pkg.mel_layout([5, -1], 80)
    for kw in (dict(n_mels=64), dict(n_mels=80.5), dict(feature_layout="band"), dict(feature_layout=2), dict(feature_layout=None)):
        with pytest.raises(ValueError):
            pkg.mel_layout(planned, **kw)


def test_reference_by_hand():
    """logmel_ref on cases small enough to work out: the frame count and the reflection at both ends, the "still outside" zero, a
    constant (all of its power in bin 0, which no band weighs), a tone in its band."""
    for n, F in ((0, 0), (159, 0), (160, 1), (319, 1), (320, 2), (560, 3)):
        assert logmel_ref(np.zeros(n, dtype=np.int16), 1.0, 80)[0].shape == (F, 80)
    y = np.arange(1000, 1500, dtype=np.int16)
    q, inside = frames_of(y)
    assert q.shape == (3, 400) and inside.all() and list(q[0, :3]) == [200, 199, 198] and q[0, 200] == 0 and q[0, 399] == 199
    assert q[2, 399] == 2 * 499 - (320 + 199) and q[2, 379] == 499 and q[2, 200] == 320
    q, inside = frames_of(np.zeros(160, dtype=np.int16))  # one frame that is all reflection, and 41 taps that stay outside
    assert list(q[0, 199:202]) == [1, 0, 1] and inside[0, 41:360].all() and not inside[0, :41].any() and q[0, 359] == 159
    assert list(q[0, 360:363]) == [158, 157, 156] and inside[0, 360:].all()
    out, mel = logmel_ref(np.full(4000, 1000, dtype=np.int16), 1.0 / 32768, 80)
    assert (out[2:-2, 3:] < -9.0).all() and (out[2:-2, 0] > -1.0).all()  # DC under a Hann window: bins 0 and 1, the lowest bands
    t = np.arange(16000)
    tone = np.round(8000 * np.sin(2 * np.pi * 1000.0 / 16000 * t)).astype(np.int16)  # 1 kHz: bin 25
    out, mel = logmel_ref(tone, 1.0 / 32768, 80)
    want = int(np.argmax(filterbank64(80)[:, 25]))
    assert (mel[3:-3].argmax(axis=1) == want).all()
    amp = 8000 / 32768 * 100  # |X[25]| = amplitude * sum(w) / 2 = amplitude * 100
    row = filterbank64(80)[want]  # a Hann window leaves half the amplitude in each neighbouring bin
    assert np.allclose(mel[3:-3, want], (row[25] + (row[24] + row[26]) / 4) * amp ** 2, rtol=1e-3)
    assert (logmel_ref(np.zeros(800, dtype=np.int16), 1.0, 128)[0] == -10.0).all()


def test_float32_restatement_is_close(pkg):
    """The yardstick of the GPU test's tolerance on one white-noise track: float32 with the library's tables against float64."""
    rng = np.random.default_rng(1)
    y = rng.integers(-32768, 32768, 160 * 40 + 7, dtype=np.int16)
    wc, ws = pkg.mel_basis()
    for n_mels in (80, 128):
        B = pkg.mel_filterbank(n_mels)
        ref, mel = logmel_ref(y, 2.0 ** -15, n_mels)
        keep = mel >= 1e-8 * mel.max(axis=1, keepdims=True)
        assert keep.all()
        err = np.abs(logmel_f32(y, 2.0 ** -15, n_mels, wc, ws, B) - ref)[keep].max()
        print(n_mels, "float32 restatement: max |d log10| =", err)
        assert err < 1e-4


# ---- refusals before any device work ------------------------------------------------------------------------
def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """Every refusal of the three calls comes back as OPUSGPU_BAD_ARG with d_in / d_out NULL and -- without a device -- from a decoder
    that does not exist (`handles` of tests/test_tracks_resample.py).  A call that got as far as the device would fail otherwise."""
    lib = pkg.load_lib()
    n = batch.n_files
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    good = pkg.mel_params(80, "bands")
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)
    inf = np.array([np.inf] + [1] * (n - 1), dtype=np.float32)

    def params(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    bad_params = [params(n_mels=64), params(n_mels=0), params(n_mels=256), params(layout=2), params(layout=-1),
                  params(reserved=[0, 0, 1, 0, 0, 0]), params(reserved=[0] * 5 + [7])]
    mono_mix = pkg.mix_matrix("mono", 2)
    two_rows = pkg.mix_matrix(np.eye(2, dtype=np.int16) * 16384, 2)
    six_mono, six_stereo = pkg.mix_matrix("mono", 6), pkg.mix_matrix("stereo", 6)

    def files(mono, mix, p, scale, ctx=fake, b=batch.h):
        return lib.opusgpu_files_decode_mel(ctx, b, mono, None if mix is None else mix.ctypes.data, None if p is None else p.ctypes.data,
                                            None if scale is None else scale.ctypes.data, None, None, None, None, None)

    def ms_files(mix, p, scale, ms=fake_ms, b=ms_batch.h):
        return lib.opusgpu_ms_files_decode_mel(ms, b, None if mix is None else mix.ctypes.data, None if p is None else p.ctypes.data,
                                               None if scale is None else scale.ctypes.data, None, None, None, None, None)
    assert files(1, None, good, None, ctx=None) == BAD and files(1, None, good, None, b=None) == BAD and files(1, None, None, None) == BAD
    assert ms_files(six_mono, good, None, ms=None) == BAD and ms_files(six_mono, good, None, b=None) == BAD
    assert ms_files(None, good, None) == BAD and ms_files(six_mono, None, None) == BAD
    for p in bad_params:
        assert files(1, None, p, None) == BAD and files(0, mono_mix, p, None) == BAD and ms_files(six_mono, p, None) == BAD
    assert files(0, None, good, None) == BAD      # neither mono nor a mix
    assert files(1, mono_mix, good, None) == BAD  # both
    assert files(0, two_rows, good, None) == BAD and ms_files(six_stereo, good, None) == BAD  # a mix of two rows
    assert files(0, six_mono, good, None) == BAD and ms_files(mono_mix, good, None) == BAD    # a mix for other tracks
    for scale in (nan, inf):
        assert files(1, None, good, scale) == BAD and files(0, mono_mix, good, scale) == BAD
    assert ms_files(six_mono, good, np.array([np.nan] * ms_batch.n_files, dtype=np.float32)) == BAD

    spans = np.zeros(2, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_samples"], spans["scale"], spans["plane"] = 400, 1.0, 64
    spans["in_offset"], spans["out_offset"] = [0, 408], [0, 64 * 80]

    def kernel(s, p, ctx=fake):
        return lib.opusgpu_tracks_mel_device(ctx, len(s), s.ctypes.data, None, None if p is None else p.ctypes.data, None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    assert kernel(spans, good, ctx=None) == BAD and kernel(spans, None) == BAD
    for p in bad_params:
        assert kernel(spans, p) == BAD
    for s in (but(in_offset=4), but(in_offset=-8), but(in_samples=-1), but(out_offset=32), but(out_offset=-64), but(plane=32),
              but(in_samples=160 * 65), but(scale=np.nan), but(scale=-np.inf), but(reserved=1)):
        assert kernel(s, good) == BAD
    assert kernel(spans, good) == BAD  # these spans are in order: refused for the NULL buffers, still before the device
    short = spans.copy()
    short["in_samples"] = [159, 0]
    assert kernel(short, good) == 0 and kernel(spans[:0], good) == 0  # no frame is no error, and no device work
    rec = pkg.mel_params(80, "bands")
    planned = np.array([480, 960], dtype=np.int64)
    for p in bad_params:
        assert lib.opusgpu_mel_layout(2, planned.ctypes.data, p.ctypes.data, None) == BAD
    assert lib.opusgpu_mel_layout(2, planned.ctypes.data, None, None) == BAD and lib.opusgpu_mel_layout(-1, planned.ctypes.data, rec.ctypes.data, None) == BAD
    assert lib.opusgpu_mel_layout(2, None, rec.ctypes.data, None) == BAD


def test_decode_files_refusals_need_no_device(pkg, batch):
    """track_feature_args, and decode_files raising before it touches its decoder (an object without one is enough to see it)."""
    assert pkg.track_feature_args(batch) is None and pkg.track_feature_args(batch, None, 64, "nonsense", 24000) is None
    rec, mrec, scale, offs, planes, total, out = pkg.track_feature_args(batch, "logmel", 80, "bands", mono=True)
    assert (int(rec["n_mels"][0]), int(rec["layout"][0]), mrec, scale, out) == (80, 0, None, None, None)
    assert total == pkg.mel_layout(batch.info["track_samples"], 80, "bands")[2] > 0 and len(offs) == len(planes) == batch.n_files
    got = pkg.track_feature_args(batch, "logmel", 128, "frames", 16000, False, "mono", "f32", np.ones(batch.n_files))
    assert int(got[0]["layout"][0]) == 1 and int(got[1]["out_channels"][0]) == 1 and got[2].dtype == np.float32
    assert pkg.track_feature_args(batch, "logmel", mix=[[0.25, 0.75]])[1]["m"][0, 0, 1] == 12288
    six = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files, "track_samples": batch.track_samples})()
    assert pkg.track_feature_args(six, "logmel", mix="mono", allow_mono=False)[1]["in_channels"][0] == 6
    for b, kw in ((batch, dict(features="mfcc", mono=True)), (batch, dict(n_mels=64, mono=True)), (batch, dict(feature_layout="planar", mono=True)),
                  (batch, dict(rate=24000, mono=True)), (batch, dict(rate=48000, mono=True)), (batch, dict(format="s16", mono=True)),
                  (batch, dict(format="f32_planar", mono=True)), (batch, dict()), (batch, dict(mix="stereo")),
                  (batch, dict(mix=np.eye(2))), (batch, dict(mix="mono", mono=True)), (six, dict(mono=True)),
                  (six, dict(mono=True, allow_mono=False)), (batch, dict(mono=True, allow_mono=False)), (six, dict(mix="stereo")),
                  (batch, dict(mono=True, scale=[np.nan] * batch.n_files)), (batch, dict(mono=True, scale=np.ones(batch.n_files + 1))),
                  (batch, dict(mono=True, out=Tensor(total - 1))), (batch, dict(mono=True, out=Tensor(total, dtype="torch.int16"))),
                  (batch, dict(mono=True, out=Tensor(total, ptr=4096 + 64))), (batch, dict(mono=True, out=Tensor(total), device=1))):
        with pytest.raises(ValueError):
            pkg.track_feature_args(b, **{"features": "logmel", **kw})
    assert pkg.track_feature_args(batch, "logmel", mono=True, out=Tensor(total))[6] is not None
    assert pkg.track_feature_args(batch, "logmel", 128, mono=True)[5] * 80 == total * 128
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for kw in (dict(n_mels=64, mono=True), dict(feature_layout="x", mono=True), dict(rate=24000, mono=True), dict(format="s16", mono=True),
               dict(mix=np.eye(2)), dict(), dict(mono=True, out=Tensor(total - 1)), dict(mono=True, mix="mono")):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, features="logmel", **kw)
    ms = pkg.MultistreamContext.__new__(pkg.MultistreamContext)
    ms.h, ms.device = None, 0
    for kw in (dict(mix="stereo"), dict(), dict(mix="mono", n_mels=100), dict(mix="mono", rate=8000), dict(mix="mono", format="s16"),
               dict(mix="mono", out=Tensor(total - 1))):
        with pytest.raises(ValueError):
            ms.decode_files(None, batch=six, features="logmel", **kw)
    with pytest.raises(TypeError):
        ms.decode_files(None, batch=six, features="logmel", mono=True)  # there is still no such argument


def test_kernel_resources():
    """k_tracks_mel<3> and <4>: no scratch (the accumulators are indexed by literals only), its samples' 41,600 bytes of LDS --
    three workgroups to a CU -- and at most 256 registers, vector and accumulation together: two waves per SIMD."""
    meta = _kernel_metadata()
    seen = {}
    for mangled, (vgpr, scratch, lds) in meta.items():
        m = re.search(r"\d+k_tracks_melILi(\d+)E", mangled)
        if m:
            seen[int(m.group(1))] = (vgpr, scratch, lds)
    print(seen)
    assert sorted(seen) == [3, 4], sorted(meta)[:6]
    assert all(v[0] <= 256 and v[1] == 0 and v[2] == 160 * 130 * 2 for v in seen.values()), seen
