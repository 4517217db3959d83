"""Linear and complex STFT spectrograms of the whole-file path on the GPU (include/opusgpu.h TRACK STFT: k_tracks_stft,
opusgpu_files_decode_stft, opusgpu_ms_files_decode_stft).  The kernel alone on crafted tracks in buffers of guard words against
tests/test_tracks_stft.py::stft_ref (float64) within TOL, and its exact properties, for the five parameter sets of SETS in the
layouts of LAYOUTS; the whisper_lin set under Whisper's filterbank against k_tracks_melspec; whole files bit for bit against the
kernel alone run over the int16 mono tracks of the same planned batch (which the rate, ratio and mix tests hold against their
integer references).

TOL: 8 x the largest error of stft_f32 -- float32 numpy with the library's tables -- against stft_ref over the kept cells of
crafted_tracks, per set: an absolute difference of the log outputs, a relative one of the linear real outputs, |d Re| and |d Im|
over the frame's largest float64 magnitude for pairs.  Kept cells: every pair; real cells whose float64 S is at least 1e-8 x its
frame's largest.  YARDSTICK holds what a CPU measured (tests/test_tracks_stft.py::test_yardstick recomputes and prints it);
test_kernel_alone prints the recomputed value, the recorded one and the kernel's own worst error.
On an MI355X the kernel's own worst error on those cells, both layouts alike: tiny 1.13e-04, enh 4.83e-07, vits 9.39e-04, wide
6.16e-04, whisper_lin 5.97e-04.
Tiles (opusgpu_stft_tile): tiny 128, enh 128, vits 64, wide 32, whisper_lin 128."""
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
import test_tracks_stft as cpu
from ms_util import LAYOUTS as MS_LAYOUTS
from test_gpu_tracks_melspec import YARDSTICK as MELSPEC_YARDSTICK
from test_gpu_tracks_resample import stereo_files
from test_tracks_melspec import melspec_ref, spec_of
from test_tracks_stft import LAYOUTS, SETS, TILES, crafted_reference, crafted_tracks, error_of, frame_count, kept_cells, stft_of, yardstick

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32 = 0x5A5A5A5A
# the largest error of stft_f32 against stft_ref on the kept cells of crafted_tracks, measured on a CPU
YARDSTICK = {"tiny": 2.84e-04, "enh": 1.10e-06, "vits": 9.40e-04, "wide": 1.77e-03, "whisper_lin": 7.65e-04}
TOL = {n: 8 * v for n, v in YARDSTICK.items()}
MELSPEC_TOL = 8 * MELSPEC_YARDSTICK["whisper"]  # tests/test_gpu_tracks_melspec.py


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _keep_pkg(pkg):
    cpu._PKG[:] = [pkg]


def width_of(rec):
    return (int(rec["n_fft"][0]) // 2 + 1) * (2 if int(rec["power"][0]) == 0 else 1)


def lay_out(pkg, rng, tracks, scales, frames, width):
    """The input buffer -- garbage everywhere, every track at a multiple of 8 samples with garbage behind its length -- the spans,
    and the size of the output buffer: tracks of `width` floats a frame at multiples of 64 floats, with room between them that
    must stay guard.  frames(n): a track's F."""
    spans = np.zeros(len(tracks), dtype=pkg.MEL_SPAN_DTYPE)
    at_in = at_out = 0
    for i, y in enumerate(tracks):
        plane = (frames(len(y)) + 63) // 64 * 64 + 64 * int(rng.integers(0, 2))
        spans[i] = (at_in, len(y), at_out, plane, scales[i], 0)
        at_in = (at_in + len(y) + int(rng.integers(0, 40)) + 7) // 8 * 8
        at_out += width * plane + 64 * int(rng.integers(0, 2))
    buf = rng.integers(-32768, 32768, at_in + 64, dtype=np.int16)
    for sp, y in zip(spans, tracks):
        buf[sp["in_offset"]:sp["in_offset"] + len(y)] = y
    return buf, spans, at_out + 64


def cells_of(sp, F, bins, c, frames_major):
    """Indices [F, bins] of the first float of every cell of a spectrogram track in the output buffer (c floats a cell)."""
    f, k = np.arange(F)[:, None], np.arange(bins)[None, :]
    return sp["out_offset"] + (f * bins + k if frames_major else k * sp["plane"] + f) * c


def values_at(words, at, c):
    """The cells at `at` of a buffer of uint32 words: float32, or complex64 from the pairs."""
    re = words[at].view(np.float32)
    return re if c == 1 else re + 1j * words[at + 1].view(np.float32)


def run_kernel(ctx, buf, spans, total, rec, runs=1, run=None):
    run = run or (lambda s, d_in, d_out: ctx.tracks_stft_device(s, d_in, rec, d_out))
    fill = np.full(total, GUARD32, dtype=np.uint32)
    d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
    got = []
    try:
        ctx.h2d(d_in, buf)
        ctx.h2d(d_out, fill)
        run(spans[:0], d_in, d_out)  # no track: nothing
        none = np.zeros_like(fill)
        ctx.d2h(none, d_out)
        assert (none == GUARD32).all()
        for _ in range(runs):
            run(spans, d_in, d_out)
            g = np.zeros_like(fill)
            ctx.d2h(g, d_out)
            got.append(g)
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    return got


# ---- the kernel alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", [(n, lay) for n in SETS for lay in LAYOUTS[n]])
def test_kernel_alone(pkg, ctx, name, layout):
    """k_tracks_stft on crafted_tracks in one launch: every kept cell within TOL of stft_ref, at most 1 % of the cells not kept,
    every word outside the tracks' cells an untouched guard word, the all-zero track (whose scale is negative) one bit pattern of
    the right value -- +0 for pairs and for a floor of 0, never -0 --, a launch with no track nothing, a second run the same bits."""
    tracks, scales = crafted_tracks(name)
    refs = crafted_reference(name)
    rec = stft_of(pkg, name, layout)
    assert pkg.stft_tile(rec) == TILES[name]
    bins, c, frames_major = int(rec["n_fft"][0]) // 2 + 1, 2 if int(rec["power"][0]) == 0 else 1, layout == "frames"
    rng = np.random.default_rng(len(name) + frames_major)
    buf, spans, total = lay_out(pkg, rng, tracks, scales, lambda n: frame_count(rec, n), bins * c)
    first, second = run_kernel(ctx, buf, spans, total, rec, runs=2)
    assert np.array_equal(first, second)  # the same bits
    written = np.zeros(total, dtype=bool)
    cells = dropped = zero_tracks = 0
    worst = 0.0
    floor_value = cpu.stft_ref(np.zeros(4 * int(rec["n_fft"][0]), dtype=np.int16), 1.0, rec)[0][0, 0]
    for i, (sp, y, (ref, S)) in enumerate(zip(spans, tracks, refs)):
        F = frame_count(rec, len(y))
        assert ref.shape == (F, bins)
        if not F:
            continue  # no frame: no cell, nothing written (the guards below)
        at = cells_of(sp, F, bins, c, frames_major)
        for h in range(c):
            assert not written[at + h].any()
            written[at + h] = True
        got = values_at(first, at, c)
        assert np.isfinite(got).all(), i
        keep = kept_cells(S, rec)
        cells, dropped = cells + keep.size, dropped + int((~keep).sum())
        err = error_of(got, ref, S, rec)
        worst = max(worst, float(err[keep].max(initial=0)))
        assert (err[keep] <= TOL[name]).all(), (i, len(y), float(sp["scale"]), float(err[keep].max()), TOL[name], np.argwhere(err * keep > TOL[name])[:4])
        if not y.any():  # the all-zero track: one bit pattern, the value of the floor (pairs: +0)
            zero_tracks += 1
            words = np.concatenate([first[at + h].ravel() for h in range(c)])
            assert len(np.unique(words)) == 1, np.unique(words)[:4]
            if c == 2 or floor_value == 0:
                assert words[0] == 0  # +0.0f: -0.0f is 0x80000000
            else:
                assert abs(float(words[:1].view(np.float32)[0]) - floor_value) <= 1e-6 * max(1.0, abs(floor_value))
    print(f"{name} {layout}: tile {TILES[name]}, {cells} cells, {dropped} not kept, worst error {worst:.3g} (allowed {TOL[name]:.3g}, "
          f"float32 numpy {yardstick(pkg, name)[0]:.3g}, recorded {YARDSTICK[name]:.3g})")
    assert cells > 500 and dropped <= 0.01 * cells and zero_tracks >= 1
    assert (first[~written] == GUARD32).all(), np.nonzero(first[~written] != GUARD32)[0][:8]  # padding is never written


def test_no_frame_writes_nothing(pkg, ctx):
    """Tracks without a frame alone -- n < hop with F = n / hop, n = 0 with F = n / hop + 1 --: not a word of the output changes."""
    rng = np.random.default_rng(3)
    for name, layout, ns in (("whisper_lin", "bands", (0, 1, 8, 159)), ("tiny", "frames", (0, 0)), ("enh", "bands", (0, 0))):
        rec = stft_of(pkg, name, layout)
        tracks = [rng.integers(-32768, 32768, n, dtype=np.int16) for n in ns]
        buf, spans, total = lay_out(pkg, rng, tracks, np.ones(len(ns), dtype=np.float32), lambda n: frame_count(rec, n), width_of(rec))
        spans["plane"] = 64
        (got,) = run_kernel(ctx, buf, spans, total + 64 * width_of(rec) * 4, rec)
        assert (got == GUARD32).all()


def test_whisper_lin_feeds_the_mel_kernel(pkg, ctx):
    """One DFT, two consumers: Whisper's filterbank (spec_filterbank) applied in float64 to k_tracks_stft's whisper_lin power, then
    the floor and log10, lies within the sum of the two kernels' tolerances of k_tracks_melspec's whisper set over the same tracks."""
    tracks, scales = crafted_tracks("whisper_lin")
    lin, mel_rec = stft_of(pkg, "whisper_lin"), spec_of(pkg, "whisper")
    B = pkg.spec_filterbank(mel_rec).astype(np.float64)
    floor = float(mel_rec["floor"][0])
    buf, spans, total = lay_out(pkg, np.random.default_rng(16), tracks, scales, lambda n: n // 160, 201)
    (new,) = run_kernel(ctx, buf, spans, total, lin)
    mbuf, mspans, mtotal = lay_out(pkg, np.random.default_rng(17), tracks, scales, lambda n: n // 160, 80)
    (old,) = run_kernel(ctx, mbuf, mspans, mtotal, mel_rec, run=lambda s, d_in, d_out: ctx.tracks_melspec_device(s, d_in, mel_rec, d_out))
    cells = 0
    worst = 0.0
    for sp, msp, y, s in zip(spans, mspans, tracks, scales):
        F = len(y) // 160
        if F:
            power = values_at(new, cells_of(sp, F, 201, 1, False), 1).astype(np.float64)
            mine = np.log10(np.maximum(power @ B.T, floor))
            theirs = values_at(old, cells_of(msp, F, 80, 1, False), 1).astype(np.float64)
            mel = melspec_ref(y, s, mel_rec)[1]
            keep = mel >= 1e-8 * mel.max(axis=1, keepdims=True)
            d = np.abs(mine - theirs)[keep]
            worst = max(worst, float(d.max(initial=0)))
            assert (d <= TOL["whisper_lin"] + MELSPEC_TOL).all(), (len(y), float(d.max()))
            cells += int(keep.sum())
    print(f"whisper_lin under Whisper's filterbank vs k_tracks_melspec: worst difference {worst:.3g} over {cells} cells "
          f"(allowed {TOL['whisper_lin'] + MELSPEC_TOL:.3g})")
    assert cells > 10000


# ---- whole files --------------------------------------------------------------------------------------------
def kernel_over_tracks(pkg, ctx, tracks16, scales, offsets, planes, total, rec):
    """tracks_stft_device over int16 tracks [m, 1] laid out on the grid decode_files reports -> the packed float32 buffer (as uint32)."""
    spans = np.zeros(len(tracks16), dtype=pkg.MEL_SPAN_DTYPE)
    at = 0
    for i, y in enumerate(tracks16):
        spans[i] = (at, len(y), offsets[i], planes[i], scales[i], 0)
        at = (at + len(y) + 63) // 64 * 64
    buf = np.full(at + 64, -12345, dtype=np.int16)
    for sp, y in zip(spans, tracks16):
        buf[sp["in_offset"]:sp["in_offset"] + len(y)] = y[:, 0]
    return run_kernel(ctx, buf, spans, max(total, 1), rec)[0]


def same_as_kernel_alone(pkg, ctx, tracks16, feats, info, planned, scales, rec, up, down):
    """feats, info = decode_files(features=rec) of the batch whose int16 mono tracks at up / down of 48 kHz are tracks16: the grid
    stft_layout gives, frames equal to stft_frames of the final lengths, and every cell bit for bit.  -> the number of cells."""
    bins, c, frames_major = int(rec["n_fft"][0]) // 2 + 1, 2 if int(rec["power"][0]) == 0 else 1, int(rec["layout"][0]) == 1
    offs, planes, total = pkg.stft_layout(planned, up, down, rec)
    assert np.array_equal(info["feat_offset"], offs) and (offs % 64 == 0).all()
    assert np.array_equal(info["frames"], [frame_count(rec, len(y)) for y in tracks16])
    assert np.array_equal(info["frames"], pkg.stft_frames(rec, -(-info["track_samples"] * up // down)))
    want = kernel_over_tracks(pkg, ctx, tracks16, scales, offs, planes, total, rec)
    cells = 0
    for sp_off, plane, F, g in zip(offs, planes, info["frames"], feats):
        assert g.dtype == (np.complex64 if c == 2 else np.float32) and g.shape == ((F, bins) if frames_major else (bins, F))
        at = cells_of({"out_offset": sp_off, "plane": plane}, F, bins, c, frames_major)
        g = g if frames_major else g.T
        halves = [g] if c == 1 else [g.real, g.imag]
        for h, part in enumerate(halves):
            assert np.array_equal(np.ascontiguousarray(part).view(np.uint32), want[at + h])
        cells += g.size
    return cells


@pytest.mark.parametrize("name,layout,how,pipeline", [("enh", "frames", dict(rate=16000, mono=True), 1),
                                                      ("vits", "bands", dict(resample=22050, mono=True), 0)])
def test_files_stft(pkg, ctx, name, layout, how, pipeline):
    """decode_files(features=record, mono=True) of the stereo corpus and the files whose frame fails on the device equals
    tracks_stft_device over the int16 tracks of decode_files with the same rate or ratio, bit for bit; a failed track reports its
    shorter F and keeps its planned plane; scale= reaches the samples; loudness= folds its gain into the scale."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    planned = b.info["track_samples"].copy()
    rec = stft_of(pkg, name, layout)
    up, down = {"enh": (1, 3), "vits": (147, 320)}[name]
    t16, i16 = ctx.decode_files(None, batch=b, **how)
    scales = np.full(len(files), 2.0 ** -15, dtype=np.float32)
    feats, info = ctx.decode_files(None, batch=b, features=rec, **how)
    for field in i16.dtype.names:
        if field not in ("out_samples", "out_offset", "frames"):  # (`frames` is F here, the plan's count of Opus frames there)
            assert np.array_equal(i16[field], info[field]), field
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, up, down) > 10000
    assert any(x is not None for x in bad)
    _, planes, _ = pkg.stft_layout(planned, up, down, rec)
    for i, seq in enumerate(bad):
        if seq is not None:
            final = b.packet_start(i, seq)
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, seq)
            assert info["track_samples"][i] == final < planned[i]
            assert info["frames"][i] == frame_count(rec, -(-final * up // down)) < frame_count(rec, -(-int(planned[i]) * up // down))
            assert planes[i] == (frame_count(rec, -(-int(planned[i]) * up // down)) + 63) // 64 * 64
    if name == "enh":  # the record's rate alone names the track; loudness=-23.0: every track's gain on top of scale=, in the kernel's scale
        again, ainfo = ctx.decode_files(None, batch=b, features=rec, mono=True, format="f32")
        assert np.array_equal(ainfo, info) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(again, feats))
        loud, linfo = ctx.decode_files(None, batch=b, features=rec, loudness=-23.0, **how)
        gains = (scales.astype(np.float64) * linfo["gain"]).astype(np.float32)
        plain = np.zeros(len(files), dtype=info.dtype)
        for field in info.dtype.names:
            plain[field] = linfo[field]
        assert np.array_equal(plain, info) and (linfo["gain"] != 1.0).any()
        assert same_as_kernel_alone(pkg, ctx, t16, loud, plain, planned, gains, rec, up, down) > 10000
    else:
        gains = np.linspace(0.5, 2.0, len(files)).astype(np.float32) / 32768
        scaled, sinfo = ctx.decode_files(None, batch=b, features=rec, scale=gains, **how)
        assert same_as_kernel_alone(pkg, ctx, t16, scaled, sinfo, planned, gains, rec, up, down) > 10000
        assert not all(np.array_equal(x, y) for x, y in zip(scaled, feats))
    b.close()


def test_files_stft_of_cuts(pkg, ctx):
    """A packed batch of cuts is a batch like any other: pairs, bins-major, equal to the kernel alone over the cuts' int16 tracks."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)]
    cuts = [(0, 0, None), (1, 100, 3000), (2, 960, 6000), (3, 0, 1), (1, 4000, 2500)]
    ctx.streams_alloc(len(cuts), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
    planned = b.info["track_samples"].copy()
    rec = stft_of(pkg, "enh", "bands")
    t16, _ = ctx.decode_files(None, batch=b, rate=16000, mono=True)
    feats, info = ctx.decode_files(None, batch=b, features=rec, mono=True)
    assert np.array_equal(info["cut_start"], b.cut_info["start"])
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, np.full(len(cuts), 2.0 ** -15, dtype=np.float32), rec, 1, 3) > 5000
    b.close()


def test_surround_stft(pkg, ctx):
    """A 5.1 layout, the wide set via resample=44100 and mix="mono": equal to the kernel alone over decode_files(resample=44100,
    mix="mono")."""
    layout = MS_LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    planned = b.info["track_samples"].copy()
    rec = stft_of(pkg, "wide", "bands")
    t16, _ = ms.decode_files(None, batch=b, resample=44100, mix="mono")
    feats, info = ms.decode_files(None, batch=b, features=rec, resample=44100, mix="mono")
    scales = np.full(n, 2.0 ** -15, dtype=np.float32)
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, 147, 160) > 5000
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, features=rec, resample=44100, mix="stereo")
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, features=rec, resample=44100, mix="mono", feature_stride=64)
    b.close()
    ms.close()


def test_refusals_leave_the_gpu_alone(pkg, ctx):
    """decode_files raises ValueError for feature_stride=, format="s16", neither or both of mono / mix, a record whose rate is not the
    track's and a log with pairs; opusgpu_files_decode_stft with a real context, a real batch and real buffers answers
    OPUSGPU_BAD_ARG -- a feature-batch request on the context among the reasons -- and leaves the output buffer and the caller's
    arrays as they were; then a call in order works."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2)
    n = b.n_files
    good, vits = stft_of(pkg, "enh"), stft_of(pkg, "vits")
    logged = good.copy()
    logged["log"], logged["floor"] = 1, 1e-5  # a log with pairs
    with pytest.raises(ValueError):
        pkg.stft_spec(16000, 512, 128, 400, power=None, log="log10", floor=1e-5)
    for features, kw in ((good, dict(mono=True, feature_stride=3000)), (good, dict(mono=True, normalize="cmn")), (good, dict(mono=True, format="s16")),
                         (good, dict()), (good, dict(mono=True, mix="mono")), (good, dict(rate=24000, mono=True)), (vits, dict(rate=16000, mono=True)),
                         (vits, dict(resample=44100, mono=True)), (logged, dict(mono=True))):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=b, features=features, **kw)
    total = max(pkg.stft_layout(b.info["track_samples"], 1, 3, good)[2], pkg.stft_layout(b.info["track_samples"], 147, 320, vits)[2])
    fill = np.full(total + 64, GUARD32, dtype=np.uint32)
    d_out = ctx.dev_alloc(fill.nbytes)
    mono_mix, two = pkg.mix_matrix("mono", 2), pkg.mix_matrix("stereo", 2)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)

    def call(rate, up, down, mono, mix, p, scale, out):
        return ctx.lib.opusgpu_files_decode_stft(ctx.h, b.h, rate, up, down, mono, None if mix is None else mix.ctypes.data, p.ctypes.data,
                                                 None if scale is None else scale.ctypes.data, out, *[a.ctypes.data for a in arrays])

    def params(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    try:
        ctx.h2d(d_out, fill)
        for rate, up, down, mono, mix, p, scale, out in (
                (16000, 0, 0, 1, None, logged, None, d_out), (16000, 0, 0, 1, None, params(layout=3), None, d_out),
                (16000, 0, 0, 1, None, params(reserved=[0, 0, 0, 1, 0, 0, 0]), None, d_out), (16000, 0, 0, 1, None, params(n_fft=500), None, d_out),
                (16000, 0, 0, 1, None, params(hop=0), None, d_out), (16000, 0, 0, 1, None, params(power=3), None, d_out),
                (16000, 0, 0, 1, None, params(floor=-1.0), None, d_out), (16000, 0, 0, 1, None, params(win_length=402 + 1), None, d_out),
                (16000, 0, 0, 0, None, good, None, d_out), (16000, 0, 0, 1, mono_mix, good, None, d_out), (16000, 0, 0, 0, two, good, None, d_out),
                (16000, 0, 0, 1, None, good, nan, d_out), (16000, 0, 0, 1, None, good, None, d_out.value + 64),
                (24000, 0, 0, 1, None, good, None, d_out), (16000, 0, 0, 1, None, vits, None, d_out), (0, 147, 320, 1, None, good, None, d_out),
                (16000, 1, 3, 1, None, good, None, d_out), (22050, 0, 0, 1, None, vits, None, d_out), (0, 3, 1, 1, None, good, None, d_out),
                (0, 0, 0, 1, None, good, None, d_out)):
            assert call(rate, up, down, mono, mix, p, scale, out) == pkg.OPUSGPU_BAD_ARG
        fb = pkg.feature_batch_request([10] * n, 80, feature_stride=3000)  # a feature-batch request on the context
        ctx._chk(ctx.lib.opusgpu_set_feature_batch(ctx.h, fb.rec.ctypes.data, None, None, fb.width), "opusgpu_set_feature_batch")
        try:
            assert call(16000, 0, 0, 1, None, good, None, d_out) == pkg.OPUSGPU_BAD_ARG
            assert b"not batched" in ctx.lib.opusgpu_last_error(ctx.h)
        finally:
            ctx.lib.opusgpu_set_feature_batch(ctx.h, None, None, None, 0)
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all() and all((a == -7).all() for a in arrays)
        assert call(16000, 0, 0, 1, None, good, None, d_out) == 0 and (arrays[1] == -(-arrays[2] // 3) // 128 + 1).all()  # and the call in order works
        assert call(0, 147, 320, 0, mono_mix, vits, None, d_out) == 0 and (arrays[1] == -(-arrays[2] * 147 // 320) // 256 + 1).all()
    finally:
        ctx.dev_free(d_out)
        b.close()


OUT_SCRIPT = r"""
import importlib.util, os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "tests"))
spec = importlib.util.spec_from_file_location("esp32_opus_player_amd", os.path.join(root, "esp32-opus-player_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pkg)
import files_util as fu
import torch
files = [c[1] for c in fu.corpus20(2, channel_switches=False) if c[2] is not None]
ctx = pkg.Context(0)
ctx.streams_alloc(len(files), 2)
b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE)
FILL = 12345.5
for rec, dtype in ((pkg.stft_spec(16000, 512, 128, 400, power=None), torch.complex64), (pkg.stft_spec(16000, 400, 160, power=1, frames="whisper"), torch.float32)):
    bins, c = int(rec["n_fft"][0]) // 2 + 1, 2 if dtype == torch.complex64 else 1
    want, winfo = ctx.decode_files(None, batch=b, features=rec, mono=True)
    offs, planes, total = pkg.stft_layout(b.info["track_samples"], 1, 3, rec)
    out = torch.full((total + 256,), FILL, dtype=torch.float32, device="cuda:0")
    feats, info = ctx.decode_files(None, batch=b, features=rec, mono=True, out=out)
    assert np.array_equal(info, winfo) and len(feats) == len(files) and sum(w.size for w in want) > 5000
    untouched = torch.ones(total + 256, dtype=torch.bool)
    for t, w, o, p in zip(feats, want, offs, planes):
        assert t.is_cuda and t.dtype == dtype and tuple(t.shape) == w.shape and w.shape[0] == bins
        assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
        assert np.array_equal(np.ascontiguousarray(t.cpu().numpy()).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
        for k in range(bins):
            untouched[int(o) + k * int(p) * c:int(o) + (k * int(p) + w.shape[1]) * c] = False
    host = out.cpu()
    assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
    frec = rec.copy()
    frec["layout"] = pkg.MEL_FRAMES_MAJOR
    fm, _ = ctx.decode_files(None, batch=b, features=frec, rate=16000, mono=True, out=out)
    assert all(t.dtype == dtype and np.array_equal(t.cpu().numpy().T.copy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32)) for t, w in zip(fm, want))
    before = out.clone()
    for bad in (out[1:], out.to(torch.float64), out[:total - 1], out[::2], out.cpu()):
        try:
            ctx.decode_files(None, batch=b, features=frec, mono=True, out=bad)
        except ValueError:
            continue
        raise AssertionError("accepted a tensor that does not fit")
    assert bool((out == before).all())  # a short `out` raises and leaves no device work behind
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(features=record, out=tensor): straight into a float32 torch tensor of stft_layout's size, the spectrograms views
    of it (complex64 views of the pairs for the complex STFT) equal to the numpy route, every element outside them as it was; a
    tensor that does not fit raises before any device work.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
