"""Track rates of the whole-file path (include/opusgpu.h, TRACK RATES), what needs no GPU: the exported symbols and the span record,
the taps, the quality of the integer filter against scipy's resample_poly, the layout helper, and the refusals that the C calls
and decode_files raise before any device work.  resample_ref is the numpy restatement of the header's VALUE rule that every
bit-for-bit check (tests/test_gpu_tracks_resample.py) compares against."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS
from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_resample_taps", "opusgpu_resample_layout", "opusgpu_tracks_resample_device", "opusgpu_files_decode_resampled",
       "opusgpu_ms_files_decode_resampled"]
FACTORS = {24000: 2, 16000: 3, 12000: 4, 8000: 6}


def resample_ref(x, rate, taps=None, mono=False):
    """TRACK RATES, VALUE: x int16 [n, channels], all of it signal (the FINAL length), zeros outside -> int16 [ceil(n / D), 1 if mono
    else channels].  taps: opusgpu_resample_taps(rate) (none for 48000).  int64 throughout."""
    x = np.asarray(x).astype(np.int64)
    x = x[:, None] if x.ndim == 1 else x
    if mono:
        assert x.shape[1] <= 2
        x = (x.sum(axis=1, keepdims=True) + 1) >> 1 if x.shape[1] == 2 else x
    if rate == 48000:
        assert mono
        return x.astype(np.int16)
    D = 48000 // rate
    h = np.asarray(taps).astype(np.int64)
    L = len(h)
    assert L == 24 * D + 1
    n = len(x)
    m = -(-n // D)
    pad = np.zeros((m * D + L, x.shape[1]), dtype=np.int64)  # pad[i] = x[i - (L - 1) / 2]
    pad[(L - 1) // 2:(L - 1) // 2 + n] = x
    idx = np.arange(m)[:, None] * D + np.arange(L)[None, :]
    acc = np.stack([pad[:, c][idx] @ h for c in range(x.shape[1])], axis=1) if m else np.zeros((0, x.shape[1]), dtype=np.int64)
    assert np.abs(acc).max(initial=0) + 16384 < 2 ** 31
    return np.clip((acc + 16384) >> 15, -32768, 32767).astype(np.int16)


def test_symbols_and_span_record(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "TRACK RATES" in hdr
    d = pkg.RESAMPLE_SPAN_DTYPE
    assert d.itemsize == 40 and "opusgpu_resample_span { /* 40 bytes" in hdr
    assert [(n, d.fields[n][1]) for n in d.names] == [("in_offset", 0), ("in_samples", 8), ("out_offset", 16), ("out_plane", 24), ("scale", 32),
                                                      ("reserved", 36)]
    assert pkg.TRACK_RATES == {**FACTORS, 48000: 1}


@pytest.mark.parametrize("rate", list(FACTORS))
def test_taps(pkg, rate):
    D = FACTORS[rate]
    h = pkg.resample_taps(rate).astype(np.int64)
    assert pkg.load_lib().opusgpu_resample_taps(rate, None) == len(h) == 24 * D + 1
    assert np.array_equal(h, h[::-1]) and h.sum() == 32768 and np.abs(h).sum() <= 65535
    print(rate, "sum |h| =", np.abs(h).sum(), "centre", h[12 * D])


def test_taps_of_other_rates(pkg):
    for rate in (48000, 44100, 0, -8000, 32000):
        assert pkg.load_lib().opusgpu_resample_taps(rate, None) == pkg.OPUSGPU_BAD_ARG
        with pytest.raises(ValueError):
            pkg.resample_taps(rate)


def test_tables_are_what_the_tool_generates(pkg):
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_resample_taps as g
    assert g.build_text() == open(os.path.join(ROOT, g.REL)).read()
    for rate, D in FACTORS.items():
        assert g.taps(D) == list(pkg.resample_taps(rate))


def test_quality_against_resample_poly(pkg):
    """The integer filter is no worse than scipy's default polyphase decimator: on sines of amplitude 16000, one second at 48 kHz,
    the first and last 200 output samples left out -- pass band: worst RMS error against the ideal decimated sine over the tones
    {0.05, 0.2, 0.35} fs_out; stop band: worst output RMS over the tones {0.6, 0.65, 0.8, 0.95} fs_out, which a decimator must
    remove (they alias)."""
    signal = pytest.importorskip("scipy.signal")
    n = np.arange(48000)
    for rate, D in FACTORS.items():
        h = pkg.resample_taps(rate)
        m = np.arange(48000 // D)[200:-200]
        rms = lambda e: float(np.sqrt(np.mean(np.square(e))))
        ours_pass, poly_pass, ours_stop, poly_stop = [], [], [], []
        for f in (0.05, 0.2, 0.35):  # in units of fs_out: f / D of the input rate
            x = 16000 * np.sin(2 * np.pi * f / D * n)
            ideal = 16000 * np.sin(2 * np.pi * f * m)
            ours_pass.append(rms(resample_ref(np.round(x).astype(np.int16), rate, h)[200:-200, 0] - ideal))
            poly_pass.append(rms(signal.resample_poly(np.round(x), 1, D)[200:-200] - ideal))
        for f in (0.6, 0.65, 0.8, 0.95):
            x = np.round(16000 * np.sin(2 * np.pi * f / D * n))
            ours_stop.append(rms(resample_ref(x.astype(np.int16), rate, h)[200:-200, 0]))
            poly_stop.append(rms(signal.resample_poly(x, 1, D)[200:-200]))
        print(f"D={D}: pass-band error {max(ours_pass):.2f} LSB (resample_poly {max(poly_pass):.2f}), "
              f"alias residue {max(ours_stop):.2f} LSB (resample_poly {max(poly_stop):.2f})")
        assert max(ours_pass) <= max(poly_pass), (D, ours_pass, poly_pass)
        assert max(ours_stop) <= max(poly_stop), (D, ours_stop, poly_stop)


def test_layout_helper(pkg):
    planned = np.array([0, 1, 63, 64, 65, 64 * 6, 64 * 6 + 1, 0, 100000, 7], dtype=np.int64)
    for rate, D in {**FACTORS, 48000: 1}.items():
        offs, total = pkg.resample_layout(planned, rate)
        lens = -(-planned // D)
        want = np.concatenate([[0], np.cumsum((lens + 63) // 64 * 64)])
        assert (offs % 64 == 0).all() and np.array_equal(offs, want[:-1]) and total == want[-1], rate
        assert offs[1] == 0 and offs[8] == offs[7]  # an empty track takes no room
    offs, total = pkg.resample_layout([], 16000)
    assert len(offs) == 0 and total == 0
    lib = pkg.load_lib()
    assert lib.opusgpu_resample_layout(planned.size, planned.ctypes.data, 16000, None) == pkg.resample_layout(planned, 16000)[1]
    for bad_rate in (44100, 0, 96000):
        with pytest.raises(ValueError):
            pkg.resample_layout(planned, bad_rate)
    with pytest.raises(ValueError):
        pkg.resample_layout([5, -1], 16000)


def test_reference_restatement_by_hand(pkg):
    """resample_ref on cases small enough to work out: an impulse hands out the taps, a constant the DC gain of exactly 1 away
    from the ends, the downmix rounds towards +infinity."""
    for rate, D in FACTORS.items():
        h = pkg.resample_taps(rate)
        x = np.zeros((30 * D, 1), dtype=np.int16)
        x[12 * D] = 32767  # meets tap k = 12 D - m D + 12 D at output m
        want = [int((32767 * int(h[24 * D - m * D]) + 16384) >> 15) for m in range(25)]
        assert list(resample_ref(x, rate, h)[:25, 0]) == want
        assert (resample_ref(np.full((40 * D, 2), -1234, dtype=np.int16), rate, h)[13:-13] == -1234).all()
        assert len(resample_ref(np.zeros((D + 1, 1), dtype=np.int16), rate, h)) == 2
    lr = np.array([[1, 2], [-1, -2], [32767, 32767], [-32768, -32768], [-3, 0]], dtype=np.int16)
    assert list(resample_ref(lr, 48000, mono=True)[:, 0]) == [2, -1, 32767, -32768, -1]


@pytest.fixture(scope="module")
def batch(pkg):
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    b = pkg.FileBatch(files, channels=2)
    yield b
    b.close()


@pytest.fixture(scope="module")
def ms_batch(pkg):
    layout = LAYOUTS["5.1"]
    b = pkg.MsFileBatch([c[0] for c in mf.corpus(pkg, np.random.default_rng(5), layout, 2, 3)], layout)
    yield b
    b.close()


@pytest.fixture(scope="module")
def handles(pkg, ms_batch):
    """(opusgpu_ctx *, opusgpu_ms *) for calls that must refuse: real decoders where there is a device, so that a refusal that
    slipped behind device work would show as a wrong code and nothing worse.  Without a device there is no decoder to be had:
    zeroed memory stands in, of which the calls read the device number and the stream before their checks, and a call that got
    as far as the device would come back with a HIP error -- there is no device to work on."""
    try:
        ctx = pkg.Context(0)
    except pkg.OpusGpuError:
        blank = np.zeros(1 << 20, dtype=np.uint8)
        yield C.c_void_p(blank.ctypes.data), C.c_void_p(blank.ctypes.data)
        return
    ms = pkg.MultistreamContext(0, ms_batch.n_files, *LAYOUTS["5.1"])
    yield ctx.h, ms.h
    ms.close()
    ctx.close()


def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """Every refusal of the three calls comes back as OPUSGPU_BAD_ARG, with d_in / d_out NULL and -- without a device -- from a
    decoder that does not exist (`handles`).  A call that got as far as the device would fail in another way."""
    lib = pkg.load_lib()
    n = batch.n_files
    assert ms_batch.n_files <= n
    S16, F32, PL = pkg.TRACKS_S16, pkg.TRACKS_F32, pkg.TRACKS_F32_PLANAR
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    one = np.ones(n, dtype=np.float32)
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)
    inf = np.array([np.inf] + [1] * (n - 1), dtype=np.float32)

    def files(rate, mono, fmt, scale):
        return lib.opusgpu_files_decode_resampled(fake, batch.h, rate, mono, fmt, None if scale is None else scale.ctypes.data, None, None,
                                                  None, None, None)

    def ms_files(rate, fmt, scale):
        return lib.opusgpu_ms_files_decode_resampled(fake_ms, ms_batch.h, rate, fmt, None if scale is None else scale.ctypes.data, None, None,
                                                     None, None, None)
    assert lib.opusgpu_files_decode_resampled(None, batch.h, 16000, 1, S16, None, None, None, None, None, None) == BAD
    assert lib.opusgpu_files_decode_resampled(fake, None, 16000, 1, S16, None, None, None, None, None, None) == BAD
    assert lib.opusgpu_ms_files_decode_resampled(None, ms_batch.h, 16000, S16, None, None, None, None, None, None) == BAD
    assert lib.opusgpu_ms_files_decode_resampled(fake_ms, None, 16000, S16, None, None, None, None, None, None) == BAD
    for rate, mono, fmt, scale in ((44100, 0, S16, None), (0, 1, F32, None), (48000, 0, F32, None),  # unknown rates, 48000 without mono
                                   (16000, 0, 3, None), (16000, 1, -1, None),                        # unknown formats
                                   (16000, 0, S16, one), (48000, 1, S16, one),                       # a scale with S16
                                   (24000, 0, F32, nan), (8000, 1, PL, inf)):                        # a scale that is not finite
        assert files(rate, mono, fmt, scale) == BAD, (rate, mono, fmt)
    for rate, fmt, scale in ((44100, S16, None), (48000, F32, None), (16000, 3, None), (16000, S16, one), (12000, PL, nan)):
        assert ms_files(rate, fmt, scale) == BAD, (rate, fmt)

    spans = np.zeros(2, dtype=pkg.RESAMPLE_SPAN_DTYPE)
    spans["in_samples"], spans["scale"], spans["out_plane"] = 100, 1.0, 64
    spans["in_offset"], spans["out_offset"] = [0, 128], [0, 64]

    def kernel(s, channels, rate, mono, fmt, ctx=fake):
        return lib.opusgpu_tracks_resample_device(ctx, len(s), s.ctypes.data, None, channels, rate, mono, fmt, None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    assert kernel(spans, 2, 16000, 0, S16, ctx=None) == BAD
    for channels, rate, mono, fmt in ((2, 44100, 0, S16), (2, 48000, 0, F32), (3, 16000, 1, F32), (6, 48000, 1, S16), (0, 16000, 0, S16),
                                      (9, 16000, 0, S16), (2, 16000, 0, 3)):
        assert kernel(spans, channels, rate, mono, fmt) == BAD, (channels, rate, mono, fmt)
    for s, fmt in ((but(in_offset=4), S16), (but(in_offset=-8), S16), (but(in_samples=-1), S16), (but(out_offset=32), S16),
                   (but(out_offset=-64), S16), (but(out_plane=32), PL), (but(in_samples=64 * 3 + 1), PL), (but(scale=np.nan), F32),
                   (but(scale=np.inf), PL)):
        assert kernel(s, 2, 16000, 0, fmt) == BAD
    assert kernel(spans, 2, 16000, 0, PL) == BAD  # these spans are in order: refused for the NULL buffers, still before the device
    assert kernel(but(scale=np.nan), 2, 16000, 0, S16) == BAD  # (the scale is not read for S16: the NULL buffers again)
    empty = spans.copy()
    empty["in_samples"] = 0
    assert kernel(empty, 2, 16000, 0, S16) == 0 and kernel(spans[:0], 2, 16000, 0, S16) == 0  # nothing to do is no error, and no device work


def test_decode_files_refusals_need_no_device(pkg, batch):
    """track_rate_args, and decode_files raising before it touches its decoder (an object without one is enough to see it)."""
    assert pkg.track_rate_args(batch) is None and pkg.track_rate_args(batch, 48000, False, "f32") is None
    D, ch, offs, total, out = pkg.track_rate_args(batch, 16000, True, "f32")
    assert (D, ch, out) == (3, 1, None) and total == pkg.resample_layout(batch.info["track_samples"], 16000)[1] and len(offs) == batch.n_files
    assert pkg.track_rate_args(batch, 24000)[:2] == (2, 2) and pkg.track_rate_args(batch, 48000, True)[:2] == (1, 1)
    for kw in (dict(rate=44100), dict(rate=0), dict(rate=16000.5), dict(rate="16000"), dict(rate=96000, mono=True),
               dict(rate=16000, format="f64"), dict(rate=16000, mono=True, allow_mono=False)):
        with pytest.raises(ValueError):
            pkg.track_rate_args(batch, **kw)
    six = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files})()
    with pytest.raises(ValueError):
        pkg.track_rate_args(six, 16000, True)
    assert pkg.track_rate_args(six, 16000)[:2] == (3, 6)
    # `out` is held against the RESAMPLED size
    need = total * 1
    assert pkg.track_rate_args(batch, 16000, True, "f32", Tensor(need), 0)[4] is not None
    assert int(batch.track_samples) * 2 > need + 64
    for t, fmt, dev in ((Tensor(need - 1), "f32", 0), (Tensor(need, dtype="torch.int16"), "f32", 0), (Tensor(need), "s16", 0),
                        (Tensor(need, device=("cpu", None)), "f32", 0), (Tensor(need), "f32", 1), (Tensor(need, ptr=4096 + 64), "f32", 0),
                        (Tensor(need, contiguous=False), "f32", 0)):
        with pytest.raises(ValueError):
            pkg.track_rate_args(batch, 16000, True, fmt, t, dev)
    with pytest.raises(ValueError):
        pkg.track_rate_args(batch, 16000, False, "f32", Tensor(2 * need - 1), 0)  # stereo takes twice as much
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for kw in (dict(rate=44100), dict(rate=16000, format="s16", scale=np.ones(batch.n_files)), dict(rate=16000, format="f32", scale=[np.nan] * 4),
               dict(rate=16000, mono=True, format="f32", out=Tensor(need - 1)), dict(rate=48000, mono=True, format="f64")):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, **kw)
    ms = pkg.MultistreamContext.__new__(pkg.MultistreamContext)
    ms.h, ms.device = None, 0
    ms_batch = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files, "track_samples": batch.track_samples})()
    for kw in (dict(rate=44100), dict(rate=16000, format="s16", scale=np.ones(batch.n_files))):
        with pytest.raises(ValueError):
            ms.decode_files(None, batch=ms_batch, **kw)
    with pytest.raises(TypeError):
        ms.decode_files(None, batch=ms_batch, rate=16000, mono=True)  # there is no such argument


def test_kernel_keeps_out_of_scratch():
    """k_tracks_resample<D>, every D: no scratch and no static LDS, and at most 128 vector registers (four waves per SIMD, the
    workgroup's own).  The tap pairs are read from constant tables with indices the unrolled loops make constant; were they not
    folded into the instructions, or the 14 words of a phase indexed at run time, the arrays would land in scratch."""
    meta = _kernel_metadata()
    seen = {}
    for mangled, (vgpr, scratch, lds) in meta.items():
        m = re.search(r"\d+k_tracks_resampleILi(\d+)E", mangled)
        if m:
            seen[int(m.group(1))] = (vgpr, scratch, lds)
    print(seen)
    assert sorted(seen) == [1, 2, 3, 4, 6], sorted(meta)[:6]
    assert all(v[0] <= 128 and v[1] == 0 and v[2] == 0 for v in seen.values()), seen
