"""TRACK SPECTROGRAMS by FFT on the GPU (include/opusgpu.h TRACK SPECTROGRAMS, OPUSGPU_SPEC_ALGO_FFT: k_tracks_melfft behind
opusgpu_tracks_melspec_device, opusgpu_files_decode_melspec and opusgpu_ms_files_decode_melspec).  The kernel alone on crafted tracks
in buffers of guard words against tests/test_tracks_melfft.py::melfft_ref (float64) within TOL, and its exact properties, for the six
parameter sets of SETS in both layouts; every n_fft from 64 to 8192; widths that are no multiple of 4; a frame's bits wherever it sits;
the FFT against the dense kernel where both run; whole files bit for bit against the kernel alone over the int16 mono tracks of the
same planned batch; feature batches over an FFT record.

TOL: 8 x the largest error of melfft_f32 -- a float32 radix-2 FFT in numpy with the library's tables, a float32 S and a float32
product with the library's bank -- against melfft_ref over the kept cells of crafted_tracks, per set: an absolute difference of the
log outputs, a relative one for log = none.  Kept cells: float64 mel at least 1e-8 x its frame's largest; on these sets and lengths
the reference leaves out no cell of a track that is not all zero.  YARDSTICK holds what a CPU measured
(tests/test_tracks_melfft.py::test_yardstick recomputes and holds it); test_kernel_alone prints the recomputed value, the recorded one
and the kernel's own worst error.  On an MI355X the kernel's own worst error on those cells: KERNEL_WORST below.
Tiles (opusgpu_spec_tile): mf_tiny 128, every other set 32."""
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
import test_gpu_tracks_melspec as dense_gpu
import test_tracks_melfft as cpu
from ms_util import LAYOUTS as MS_LAYOUTS
from test_gpu_feat_batch import dense_equals
from test_gpu_tracks_melspec import GUARD32, cells_of, lay_out, run_kernel, same_as_kernel_alone
from test_gpu_tracks_resample import stereo_files
from test_tracks_melfft import (CELLS, SETS, SMALL, TILES, YARDSTICK, crafted_reference, crafted_tracks, kept_cells, melfft_f32, melfft_ref, mf_of,
                                stft_twin, yardstick)
from test_tracks_melspec import error_of, frame_count, spec_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {n: 8 * v for n, v in YARDSTICK.items()}
# the kernel's own worst error on the same cells, measured on an MI355X (both layouts alike)
KERNEL_WORST = {"mf_tiny": 7.79e-07, "mf_kaldi": 2.96e-05, "mf_tts": 2.11e-06, "mf_music": 3.39e-06, "mf_sep": 1.71e-06, "mf_big": 3.02e-06}


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _keep_pkg(pkg):
    cpu._PKG[:] = [pkg]
    dense_gpu._PKG[:] = [pkg]


def f32_of(pkg, y, scale, rec):
    return melfft_f32(y, scale, rec, stft_twin(pkg, rec), *pkg.spec_fft_tables(rec), pkg.spec_filterbank(rec))


# ---- the kernel alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bands", "frames"])
@pytest.mark.parametrize("name", list(SETS))
def test_kernel_alone(pkg, ctx, name, layout):
    """k_tracks_melfft on crafted_tracks in one launch: every kept cell within TOL of melfft_ref, at most 1 % of the cells not kept
    (the reference leaves out none), every word outside the tracks' cells an untouched guard word, the all-zero track (whose scale
    is negative) one bit pattern of the floor's value -- +0 for a floor of 0, never -0 --, a launch with no track nothing, a second
    run the same bits."""
    tracks, scales = crafted_tracks(name)
    refs = crafted_reference(name)
    rec = mf_of(pkg, name, layout)
    assert pkg.spec_tile(rec) == TILES[name]
    n_mels, frames_major = int(rec["n_mels"][0]), layout == "frames"
    rng = np.random.default_rng(len(name) + frames_major)
    buf, spans, total = lay_out(pkg, rng, tracks, scales, rec)
    first, second = run_kernel(ctx, buf, spans, total, rec, runs=2)
    assert np.array_equal(first, second)  # the same bits
    written = np.zeros(total, dtype=bool)
    cells = dropped = zero_tracks = 0
    worst = 0.0
    floor_value = melfft_ref(np.zeros(4 * int(rec["n_fft"][0]), dtype=np.int16), 1.0, rec)[0][0, 0]
    for i, (sp, y, (ref, mel)) in enumerate(zip(spans, tracks, refs)):
        F = frame_count(rec, len(y))
        assert ref.shape == (F, n_mels)
        if not F:
            continue  # no frame: no cell, nothing written (the guards below)
        at = cells_of(sp, F, n_mels, frames_major)
        assert not written[at].any()
        written[at] = True
        got = first[at].view(np.float32)
        assert np.isfinite(got).all(), i
        keep = kept_cells(mel)
        err = error_of(got, ref, rec)
        worst = max(worst, float(err[keep].max(initial=0)))
        assert (err[keep] <= TOL[name]).all(), (i, len(y), float(sp["scale"]), float(err[keep].max()), TOL[name], np.argwhere(err * keep > TOL[name])[:4])
        if not y.any():  # the all-zero track: one bit pattern, the value of the floor
            zero_tracks += 1
            assert float(sp["scale"]) < 0 and len(np.unique(first[at])) == 1, np.unique(first[at])[:4]
            if floor_value == 0:
                assert first[at].ravel()[0] == 0  # +0.0f: -0.0f is 0x80000000
            else:
                assert abs(float(got[0, 0]) - floor_value) <= 1e-6 * max(1.0, abs(floor_value))
        else:
            cells, dropped = cells + keep.size, dropped + int((~keep).sum())
    print(f"{name} {layout}: tile {TILES[name]}, {cells} cells, {dropped} not kept, worst error {worst:.3g} (allowed {TOL[name]:.3g}, "
          f"float32 numpy {yardstick(pkg, name)[0]:.3g}, recorded {YARDSTICK[name]:.3g}, kernel recorded {KERNEL_WORST[name]:.3g})")
    assert cells == CELLS[name] and dropped <= 0.01 * cells and zero_tracks == 1
    assert (first[~written] == GUARD32).all(), np.nonzero(first[~written] != GUARD32)[0][:8]  # padding is never written


def test_every_size(pkg, ctx):
    """Every n_fft from 64 to 8192 -- each exponent is a pass schedule of its own --, one launch per size and layout: a full-scale
    noise track of 3 n_fft + 5 samples, hop n_fft / 4, 48000 Hz, 40 Slaney bands, power 2, no log, floor 0, against melfft_ref within
    8 x melfft_f32's error on that track, recomputed here; a band without a weight (the small sizes have some) is exactly +0; guards
    as above."""
    for e in range(6, 14):
        n_fft = 1 << e
        y = np.random.default_rng(e).integers(-32768, 32768, 3 * n_fft + 5, dtype=np.int16)
        for layout in ("bands", "frames"):
            rec = pkg.mel_spec(48000, n_fft, n_fft // 4, n_mels=40, power=2, log=None, floor=0.0, feature_layout=layout, algo="fft")
            ref, mel = melfft_ref(y, 2.0 ** -15, rec)
            assert ref.shape == (13, 40)
            empty = ~pkg.spec_filterbank(rec).any(axis=1)
            keep = kept_cells(mel)
            assert (keep == ~empty[None, :]).all()  # every cell of a band that has a weight is kept
            tol = 8 * float(error_of(f32_of(pkg, y, 2.0 ** -15, rec), ref, rec)[keep].max())
            assert 0 < tol < 8 * 1e-5
            buf, spans, total = lay_out(pkg, np.random.default_rng(100 + e), [y], np.array([2.0 ** -15], dtype=np.float32), rec)
            (got,) = run_kernel(ctx, buf, spans, total, rec)
            at = cells_of(spans[0], 13, 40, layout == "frames")
            err = float(error_of(got[at].view(np.float32), ref, rec)[keep].max())
            print(f"n_fft {n_fft} {layout}: {int(empty.sum())} bands without a weight, worst error {err:.3g} (allowed {tol:.3g})")
            assert err <= tol, (n_fft, layout)
            assert (got[at][:, empty] == 0).all()  # max(0, floor) = +0
            written = np.zeros(total, dtype=bool)
            written[at] = True
            assert (got[~written] == GUARD32).all()


ODD_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 2047, 2048, 2049, 2113]


@pytest.mark.parametrize("layout", ["bands", "frames"])
@pytest.mark.parametrize("n_mels", [1, 5, 31])
def test_odd_widths(pkg, ctx, n_mels, layout):
    """Widths that are no multiple of 4 -- the frames-major run of a group then ends in element stores -- and ragged ends in both
    layouts: (16000, 256, 256, 64), HTK, no norm, power 2, no log, floor 0, noise tracks of ODD_LENGTHS, within 8 x melfft_f32's
    error on these tracks, recomputed here.  No band is without a weight and the reference leaves out no cell."""
    rec = pkg.mel_spec(16000, 256, 64, 256, n_mels, 0.0, 8000.0, "htk", None, 2, None, 0.0, "torch", layout, algo="fft")
    assert pkg.spec_filterbank(rec).any(axis=1).all()
    rng = np.random.default_rng(31 * n_mels)
    tracks = [rng.integers(-32768, 32768, n, dtype=np.int16) | 1 for n in ODD_LENGTHS]  # (no sample is 0: a track of 1 has a spectrum)
    scales = np.full(len(tracks), 2.0 ** -15, dtype=np.float32)
    refs = [melfft_ref(y, 2.0 ** -15, rec) for y in tracks]
    assert all(kept_cells(mel).all() for _, mel in refs)
    tol = 8 * max(float(error_of(f32_of(pkg, y, 2.0 ** -15, rec), ref, rec).max()) for y, (ref, _) in zip(tracks, refs))
    assert 0 < tol < 8 * 1e-5
    buf, spans, total = lay_out(pkg, rng, tracks, scales, rec)
    (got,) = run_kernel(ctx, buf, spans, total, rec)
    written = np.zeros(total, dtype=bool)
    worst = 0.0
    for sp, y, (ref, _) in zip(spans, tracks, refs):
        F = len(y) // 64 + 1
        assert ref.shape == (F, n_mels)
        at = cells_of(sp, F, n_mels, layout == "frames")
        written[at] = True
        worst = max(worst, float(error_of(got[at].view(np.float32), ref, rec).max()))
    print(f"n_mels {n_mels} {layout}: worst error {worst:.3g} (allowed {tol:.3g})")
    assert worst <= tol
    assert (got[~written] == GUARD32).all()


@pytest.mark.parametrize("name", ["mf_tts", "mf_sep"])
def test_position_independence(pkg, ctx, name):
    """A frame's cells depend on the record, the scale and the n_fft samples it reads alone: one noise track y of 40 H + 7 samples
    alone, as the third track of a batch behind two others, and as concat(noise[3 H], y) -- there frame f is frame f + 3, in another
    slot and another tile.  Every frame whose samples lie wholly inside y has the same bits in all three."""
    rec = mf_of(pkg, name)
    H, N, n_mels = int(rec["hop"][0]), int(rec["n_fft"][0]), int(rec["n_mels"][0])
    rng = np.random.default_rng(N)
    y = rng.integers(-32768, 32768, 40 * H + 7, dtype=np.int16)
    others = [rng.integers(-32768, 32768, n, dtype=np.int16) for n in (5 * H + 1, 33 * H)]
    shifted = np.concatenate([rng.integers(-32768, 32768, 3 * H, dtype=np.int16), y])
    inside = [f for f in range(frame_count(rec, len(y))) if f * H - N // 2 >= 0 and f * H + N // 2 <= len(y)]
    assert len(inside) > 30 and TILES[name] == 32  # frames 32 .. of y are in its second tile, frames 29 .. of y in the shifted track's
    runs = []
    for tracks, t, shift in (([y], 0, 0), (others + [y], 2, 0), ([shifted], 0, 3)):
        buf, spans, total = lay_out(pkg, np.random.default_rng(len(tracks) + shift), tracks, np.full(len(tracks), 2.0 ** -15, dtype=np.float32), rec)
        (got,) = run_kernel(ctx, buf, spans, total, rec)
        at = cells_of(spans[t], frame_count(rec, len(tracks[t])), n_mels, False)
        runs.append(got[at][np.array(inside) + shift])
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    assert len(np.unique(runs[0])) > 1000


@pytest.mark.parametrize("name", ["mf_tts", "mf_music"])
def test_fft_against_dense(pkg, ctx, name):
    """mf_tts and mf_music against k_tracks_melspec over the same tracks in the same process: each kernel is within its own tolerance
    of the float64 value, so on every kept cell they differ by at most the sum of the two (both sets have a log: |d|); and they
    write the same cells."""
    tracks, scales = crafted_tracks(name)
    refs = crafted_reference(name)
    frec, drec = mf_of(pkg, name), spec_of(pkg, SMALL[name])
    n_mels = int(frec["n_mels"][0])
    assert int(frec["log"][0]) and drec.tobytes() == cpu._but(frec, reserved=0).tobytes()
    buf, spans, total = lay_out(pkg, np.random.default_rng(5), tracks, scales, frec)
    (fast,) = run_kernel(ctx, buf, spans, total, frec)
    (slow,) = run_kernel(ctx, buf, spans, total, drec)
    assert np.array_equal(fast == GUARD32, slow == GUARD32)  # the same cells
    tol = TOL[name] + dense_gpu.TOL[SMALL[name]]
    cells, worst = 0, 0.0
    for sp, y, (ref, mel) in zip(spans, tracks, refs):
        F = frame_count(frec, len(y))
        if F:
            at = cells_of(sp, F, n_mels, False)
            a, b = fast[at].view(np.float32).astype(np.float64), slow[at].view(np.float32).astype(np.float64)
            keep = kept_cells(mel)
            d = np.abs(a - b)
            worst = max(worst, float(d[keep].max(initial=0)))
            assert (d[keep] <= tol).all(), (len(y), float(d[keep].max()), tol)
            cells += int(keep.sum())
    print(f"{name} vs {SMALL[name]}: worst difference {worst:.3g} over {cells} kept cells (allowed {tol:.3g})")
    assert cells > 10000


# ---- whole files --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout,how,ratio", [("mf_sep", "bands", dict(resample=44100, mono=True), (147, 160)),
                                                   ("mf_big", "frames", dict(rate=48000, mono=True), (1, 1))])
def test_files_melfft(pkg, ctx, name, layout, how, ratio):
    """decode_files(features=record, mono=True) of the stereo corpus and the files whose frame fails on the device equals
    tracks_melspec_device over the int16 tracks of decode_files with the same rate or ratio, bit for bit; a failed track reports its
    shorter F and keeps its planned plane; scale= reaches the samples; loudness= folds its gain into the scale."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    planned = b.info["track_samples"].copy()
    rec = mf_of(pkg, name, layout)
    up, down = ratio
    t16, i16 = ctx.decode_files(None, batch=b, **how)
    scales = np.full(len(files), 2.0 ** -15, dtype=np.float32)
    feats, info = ctx.decode_files(None, batch=b, features=rec, **how)
    for field in i16.dtype.names:
        if field not in ("out_samples", "out_offset", "frames"):
            assert np.array_equal(i16[field], info[field]), field
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, up, down) > 5000
    assert any(x is not None for x in bad)
    _, planes, _ = pkg.spec_layout(planned, up, down, rec)
    for i, seq in enumerate(bad):
        if seq is not None:
            final = b.packet_start(i, seq)
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, seq)
            assert info["track_samples"][i] == final < planned[i]
            assert info["frames"][i] == frame_count(rec, -(-final * up // down)) <= frame_count(rec, -(-int(planned[i]) * up // down))
            assert planes[i] == (frame_count(rec, -(-int(planned[i]) * up // down)) + 63) // 64 * 64
    if name == "mf_sep":
        loud, linfo = ctx.decode_files(None, batch=b, features=rec, loudness=-23.0, **how)
        gains = (scales.astype(np.float64) * linfo["gain"]).astype(np.float32)
        plain = np.zeros(len(files), dtype=info.dtype)
        for field in info.dtype.names:
            plain[field] = linfo[field]
        assert np.array_equal(plain, info) and (linfo["gain"] != 1.0).any()
        assert same_as_kernel_alone(pkg, ctx, t16, loud, plain, planned, gains, rec, up, down) > 5000
    else:
        gains = np.linspace(0.5, 2.0, len(files)).astype(np.float32) / 32768
        scaled, sinfo = ctx.decode_files(None, batch=b, features=rec, scale=gains, **how)
        assert same_as_kernel_alone(pkg, ctx, t16, scaled, sinfo, planned, gains, rec, up, down) > 5000
        assert not all(np.array_equal(x, y) for x, y in zip(scaled, feats))
    b.close()


def test_files_melfft_of_cuts(pkg, ctx):
    """A packed batch of cuts is a batch like any other: mf_sep, frames-major, equal to the kernel alone over the cuts' int16 tracks."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)]
    cuts = [(0, 0, None), (1, 100, 3000), (2, 960, 6000), (3, 0, 1), (1, 4000, 2500)]
    ctx.streams_alloc(len(cuts), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
    planned = b.info["track_samples"].copy()
    rec = mf_of(pkg, "mf_sep", "frames")
    t16, _ = ctx.decode_files(None, batch=b, resample=44100, mono=True)
    feats, info = ctx.decode_files(None, batch=b, features=rec, resample=44100, mono=True)
    assert np.array_equal(info["cut_start"], b.cut_info["start"])
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, np.full(len(cuts), 2.0 ** -15, dtype=np.float32), rec, 147, 160) > 500
    b.close()


def test_surround_melfft(pkg, ctx):
    """A 5.1 layout, mf_sep via resample=44100 and mix="mono": equal to the kernel alone over decode_files(resample=44100, mix="mono")."""
    layout = MS_LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    planned = b.info["track_samples"].copy()
    rec = mf_of(pkg, "mf_sep", "bands")
    t16, _ = ms.decode_files(None, batch=b, resample=44100, mix="mono")
    feats, info = ms.decode_files(None, batch=b, features=rec, resample=44100, mix="mono")
    scales = np.full(n, 2.0 ** -15, dtype=np.float32)
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, 147, 160) > 500
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, features=rec, resample=44100, mix="stereo")
    b.close()
    ms.close()


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
rec = pkg.mel_spec(44100, 4096, 1024, n_mels=128, algo="fft")
want, winfo = ctx.decode_files(None, batch=b, features=rec, resample=44100, mono=True)
offs, planes, total = pkg.spec_layout(b.info["track_samples"], 147, 160, rec)
out = torch.full((total + 256,), FILL, dtype=torch.float32, device="cuda:0")
feats, info = ctx.decode_files(None, batch=b, features=rec, resample=44100, mono=True, out=out)
assert np.array_equal(info, winfo) and len(feats) == len(files) and sum(w.size for w in want) > 2000
untouched = torch.ones(total + 256, dtype=torch.bool)
for t, w, o, p in zip(feats, want, offs, planes):
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == w.shape and w.shape[0] == 128
    assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
    assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    for j in range(128):
        untouched[int(o) + j * int(p):int(o) + j * int(p) + w.shape[1]] = False
host = out.cpu()
assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
frec = rec.copy()
frec["layout"] = pkg.MEL_FRAMES_MAJOR
fm, _ = ctx.decode_files(None, batch=b, features=frec, resample=44100, mono=True, out=out)
assert all(np.array_equal(t.cpu().numpy().T.copy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32)) for t, w in zip(fm, want))
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(features=mf_sep's record, out=tensor): straight into a float32 torch tensor of spec_layout's size, the
    spectrograms views of it equal to the numpy route, every element outside them as it was; frames-major the transpose.  In a
    process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout


# ---- feature batches ----------------------------------------------------------------------------------------
def test_feature_batch_over_fft(pkg, ctx):
    """FEATURE BATCHES with the mf_tts record: feature_stride= with normalize="cmvn" and "whisper" equal the same request applied to
    the packed FFT grid (tests/test_gpu_feat_batch.py::dense_equals: bits for "whisper", the derived bound for "cmvn"), in both
    layouts; the packed call returns the same before and after (the request is gone)."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    for layout in ("bands", "frames"):
        rec = mf_of(pkg, "mf_tts", layout)
        kw = dict(batch=b, features=rec, resample=22050, mono=True)
        packed, pinfo = ctx.decode_files(None, **kw)
        S = int(pkg.spec_frames(rec, -(-b.info["track_samples"] * 147 // 320)).max()) + 3
        for norm in ("cmvn", "whisper"):
            req = pkg.files_request(b, features=rec, resample=22050, mono=True, feature_stride=S, normalize=norm)
            dense, dinfo = ctx.decode_files(None, feature_stride=S, normalize=norm, **kw)
            assert dense_equals(pkg, dense, dinfo, packed, pinfo, 80, layout == "frames", req.feature_batch, norm) > 10000, (layout, norm)
        again, ainfo = ctx.decode_files(None, **kw)  # the request is gone
        assert np.array_equal(ainfo, pinfo) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(again, packed))
    b.close()
