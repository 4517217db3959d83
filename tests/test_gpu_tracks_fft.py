"""TRACK STFT by FFT on the GPU (include/opusgpu.h TRACK STFT, OPUSGPU_STFT_ALGO_FFT: k_tracks_fft behind opusgpu_tracks_stft_device,
opusgpu_files_decode_stft and opusgpu_ms_files_decode_stft).  The kernel alone on crafted tracks in buffers of guard words against
tests/test_tracks_fft.py::fft_ref (float64) within TOL, and its exact properties, for the six parameter sets of SETS in the layouts
of LAYOUTS; every n_fft from 64 to 8192, each a pass schedule of its own; the FFT against the dense kernel where both run; whole
files bit for bit against the kernel alone over the int16 mono tracks of the same planned batch; STFT batches over an FFT record.

TOL: 8 x the largest error of fft_f32 -- a float32 radix-2 FFT in numpy with the library's tables -- against fft_ref over the kept
cells of crafted_tracks, per set: an absolute difference of the log outputs, a relative one of the linear real outputs, |d Re| and
|d Im| over the frame's largest float64 magnitude for pairs.  Kept cells: every pair; real cells whose float64 S is at least 1e-8 x
its frame's largest.  YARDSTICK holds what a CPU measured (tests/test_tracks_fft.py::test_yardstick recomputes and prints it);
test_kernel_alone prints the recomputed value, the recorded one and the kernel's own worst error.
On an MI355X the kernel's own worst error on those cells: KERNEL_WORST below.
Tiles (opusgpu_stft_tile): fft_tiny 128, every other set 16."""
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
import test_gpu_tracks_stft as dense_gpu
import test_tracks_fft as cpu
from ms_util import LAYOUTS as MS_LAYOUTS
from test_gpu_stft_batch import dense_equals, strides_for
from test_gpu_tracks_resample import stereo_files
from test_gpu_tracks_stft import GUARD32, cells_of, lay_out, run_kernel, same_as_kernel_alone, values_at
from test_tracks_fft import LAYOUTS, SETS, TILES, crafted_reference, crafted_tracks, fft_f32, fft_of, fft_ref, yardstick
from test_tracks_stft import error_of, frame_count, kept_cells, stft_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the largest error of fft_f32 against fft_ref on the kept cells of crafted_tracks, measured on a CPU
YARDSTICK = {"fft_tiny": 3.00e-04, "fft_enh": 1.85e-07, "fft_vits": 9.99e-03, "fft_wide": 2.59e-04, "fft_sep": 2.66e-07, "fft_big": 4.57e-04}
TOL = {n: 8 * v for n, v in YARDSTICK.items()}
# the kernel's own worst error on the same cells, measured on an MI355X (both layouts alike)
KERNEL_WORST = {"fft_tiny": 3.00e-04, "fft_enh": 2.48e-07, "fft_vits": 4.89e-03, "fft_wide": 1.94e-04, "fft_sep": 2.30e-07, "fft_big": 3.05e-04}


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _keep_pkg(pkg):
    cpu._PKG[:] = [pkg]
    dense_gpu.cpu._PKG[:] = [pkg]


# ---- the kernel alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout", [(n, lay) for n in SETS for lay in LAYOUTS[n]])
def test_kernel_alone(pkg, ctx, name, layout):
    """k_tracks_fft on crafted_tracks in one launch: every kept cell within TOL of fft_ref, at most 1 % of the cells not kept, every
    word outside the tracks' cells an untouched guard word, the all-zero track (whose scale is negative) one bit pattern of the
    right value -- +0 for pairs and for a floor of 0, never -0 --, a launch with no track nothing, a second run the same bits."""
    tracks, scales = crafted_tracks(name)
    refs = crafted_reference(name)
    rec = fft_of(pkg, name, layout)
    assert pkg.stft_tile(rec) == TILES[name]
    bins, c, frames_major = int(rec["n_fft"][0]) // 2 + 1, 2 if int(rec["power"][0]) == 0 else 1, layout == "frames"
    rng = np.random.default_rng(len(name) + frames_major)
    buf, spans, total = lay_out(pkg, rng, tracks, scales, lambda n: frame_count(rec, n), bins * c)
    first, second = run_kernel(ctx, buf, spans, total, rec, runs=2)
    assert np.array_equal(first, second)  # the same bits
    written = np.zeros(total, dtype=bool)
    cells = dropped = zero_tracks = 0
    worst = 0.0
    floor_value = fft_ref(np.zeros(4 * int(rec["n_fft"][0]), dtype=np.int16), 1.0, rec)[0][0, 0]
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
        if not y.any():  # the all-zero track: one bit pattern, the value of the floor (pairs: +0)
            zero_tracks += 1
            words = np.concatenate([first[at + h].ravel() for h in range(c)])
            assert len(np.unique(words)) == 1, np.unique(words)[:4]
            if c == 2 or floor_value == 0:
                assert words[0] == 0  # +0.0f: -0.0f is 0x80000000
            else:
                assert abs(float(words[:1].view(np.float32)[0]) - floor_value) <= 1e-6 * max(1.0, abs(floor_value))
        assert (err[keep] <= TOL[name]).all(), (i, len(y), float(sp["scale"]), float(err[keep].max()), TOL[name], np.argwhere(err * keep > TOL[name])[:4])
    print(f"{name} {layout}: tile {TILES[name]}, {cells} cells, {dropped} not kept, worst error {worst:.3g} (allowed {TOL[name]:.3g}, "
          f"float32 numpy {yardstick(pkg, name)[0]:.3g}, recorded {YARDSTICK[name]:.3g})")
    assert cells > 500 and dropped <= 0.01 * cells and zero_tracks >= 1
    assert (first[~written] == GUARD32).all(), np.nonzero(first[~written] != GUARD32)[0][:8]  # padding is never written


def test_every_size(pkg, ctx):
    """Every n_fft from 64 to 8192 -- each exponent is a pass schedule of its own --, one launch per size and layout (a record has one
    size): a full-scale noise track of 3 n_fft + 5 samples, hop n_fft / 4, pairs, against fft_ref within 8 x fft_f32's error on that
    track, recomputed here; guards as above."""
    for e in range(6, 14):
        n_fft = 1 << e
        y = np.random.default_rng(e).integers(-32768, 32768, 3 * n_fft + 5, dtype=np.int16)
        for layout in ("bands", "frames"):
            rec = pkg.stft_spec(48000, n_fft, n_fft // 4, power=None, feature_layout=layout, algo="fft")
            ref, S = fft_ref(y, 2.0 ** -15, rec)
            F, bins = ref.shape
            assert (F, bins) == (13, n_fft // 2 + 1)
            window, twiddle = pkg.stft_fft_tables(rec)
            tol = 8 * float(error_of(fft_f32(y, 2.0 ** -15, rec, window, twiddle), ref, S, rec).max())
            assert 0 < tol < 8 * 4 * e * 2.0 ** -24
            buf, spans, total = lay_out(pkg, np.random.default_rng(100 + e), [y], np.array([2.0 ** -15], dtype=np.float32),
                                        lambda n: frame_count(rec, n), bins * 2)
            (got,) = run_kernel(ctx, buf, spans, total, rec)
            at = cells_of(spans[0], F, bins, 2, layout == "frames")
            err = float(error_of(values_at(got, at, 2), ref, S, rec).max())
            print(f"n_fft {n_fft} {layout}: worst error {err:.3g} (allowed {tol:.3g})")
            assert err <= tol, (n_fft, layout)
            written = np.zeros(total, dtype=bool)
            written[at], written[at + 1] = True, True
            assert (got[~written] == GUARD32).all()


@pytest.mark.parametrize("name", ["vits", "wide"])
def test_fft_against_dense(pkg, ctx, name):
    """fft_vits and fft_wide against k_tracks_stft over the same tracks in the same process: each kernel is within its own tolerance
    of the float64 value, so on every kept cell they differ by at most the sum of the two -- as |d| of the log outputs, as |d| over
    the float64 reference of the linear ones."""
    fname = "fft_" + name
    assert SETS[fname] == cpu_dense_set(name)
    tracks, scales = crafted_tracks(fname)
    refs = crafted_reference(fname)
    frec, drec = fft_of(pkg, fname), stft_of(pkg, name)
    bins = int(frec["n_fft"][0]) // 2 + 1
    buf, spans, total = lay_out(pkg, np.random.default_rng(5), tracks, scales, lambda n: frame_count(frec, n), bins)
    (fast,) = run_kernel(ctx, buf, spans, total, frec)
    (slow,) = run_kernel(ctx, buf, spans, total, drec)
    tol = TOL[fname] + dense_gpu.TOL[name]
    cells, worst = 0, 0.0
    for sp, y, (ref, S) in zip(spans, tracks, refs):
        F = frame_count(frec, len(y))
        if F:
            at = cells_of(sp, F, bins, 1, False)
            a, b = values_at(fast, at, 1).astype(np.float64), values_at(slow, at, 1).astype(np.float64)
            keep = kept_cells(S, frec)
            d = np.abs(a - b) if int(frec["log"][0]) else np.abs(a - b) / np.where(ref == 0, 1.0, np.abs(ref))
            worst = max(worst, float(d[keep].max(initial=0)))
            assert (d[keep] <= tol).all(), (len(y), float(d[keep].max()), tol)
            cells += int(keep.sum())
    print(f"{fname} vs {name}: worst difference {worst:.3g} over {cells} kept cells (allowed {tol:.3g})")
    assert cells > 10000


def cpu_dense_set(name):
    from test_tracks_stft import SETS as DENSE_SETS
    return DENSE_SETS[name]


# ---- whole files --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layout,how,ratio", [("fft_sep", "bands", dict(resample=44100, mono=True), (147, 160)),
                                                   ("fft_big", "frames", dict(rate=48000, mono=True), (1, 1))])
def test_files_fft(pkg, ctx, name, layout, how, ratio):
    """decode_files(features=record, mono=True) of the stereo corpus and the files whose frame fails on the device equals
    tracks_stft_device over the int16 tracks of decode_files with the same rate or ratio, bit for bit; a failed track reports its
    shorter F and keeps its planned plane, the others are what they are without it; scale= reaches the samples; loudness= folds
    its gain into the scale."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    planned = b.info["track_samples"].copy()
    rec = fft_of(pkg, name, layout)
    up, down = ratio
    t16, i16 = ctx.decode_files(None, batch=b, **how)
    scales = np.full(len(files), 2.0 ** -15, dtype=np.float32)
    feats, info = ctx.decode_files(None, batch=b, features=rec, **how)
    for field in i16.dtype.names:
        if field not in ("out_samples", "out_offset", "frames"):
            assert np.array_equal(i16[field], info[field]), field
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, up, down) > 10000
    assert any(x is not None for x in bad)
    _, planes, _ = pkg.stft_layout(planned, up, down, rec)
    for i, seq in enumerate(bad):
        if seq is not None:
            final = b.packet_start(i, seq)
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, seq)
            assert info["track_samples"][i] == final < planned[i]
            assert info["frames"][i] == frame_count(rec, -(-final * up // down)) <= frame_count(rec, -(-int(planned[i]) * up // down))
            assert planes[i] == (frame_count(rec, -(-int(planned[i]) * up // down)) + 63) // 64 * 64
    if name == "fft_sep":
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


def test_files_fft_of_cuts(pkg, ctx):
    """A packed batch of cuts is a batch like any other: fft_sep, frames-major, equal to the kernel alone over the cuts' int16 tracks."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)]
    cuts = [(0, 0, None), (1, 100, 3000), (2, 960, 6000), (3, 0, 1), (1, 4000, 2500)]
    ctx.streams_alloc(len(cuts), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
    planned = b.info["track_samples"].copy()
    rec = fft_of(pkg, "fft_sep", "frames")
    t16, _ = ctx.decode_files(None, batch=b, resample=44100, mono=True)
    feats, info = ctx.decode_files(None, batch=b, features=rec, resample=44100, mono=True)
    assert np.array_equal(info["cut_start"], b.cut_info["start"])
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, np.full(len(cuts), 2.0 ** -15, dtype=np.float32), rec, 147, 160) > 5000
    b.close()


def test_surround_fft(pkg, ctx):
    """A 5.1 layout, fft_sep via resample=44100 and mix="mono": equal to the kernel alone over decode_files(resample=44100, mix="mono")."""
    layout = MS_LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    planned = b.info["track_samples"].copy()
    rec = fft_of(pkg, "fft_sep", "bands")
    t16, _ = ms.decode_files(None, batch=b, resample=44100, mix="mono")
    feats, info = ms.decode_files(None, batch=b, features=rec, resample=44100, mix="mono")
    scales = np.full(n, 2.0 ** -15, dtype=np.float32)
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, 147, 160) > 5000
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, features=rec, resample=44100, mix="mono", stft_stride=64)  # 2049 bins: no STFT batch
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
rec = pkg.stft_spec(44100, 4096, 1024, power=None, algo="fft")
bins, c = 2049, 2
want, winfo = ctx.decode_files(None, batch=b, features=rec, resample=44100, mono=True)
offs, planes, total = pkg.stft_layout(b.info["track_samples"], 147, 160, rec)
out = torch.full((total + 256,), FILL, dtype=torch.float32, device="cuda:0")
feats, info = ctx.decode_files(None, batch=b, features=rec, resample=44100, mono=True, out=out)
assert np.array_equal(info, winfo) and len(feats) == len(files) and sum(w.size for w in want) > 5000
untouched = torch.ones(total + 256, dtype=torch.bool)
for t, w, o, p in zip(feats, want, offs, planes):
    assert t.is_cuda and t.dtype == torch.complex64 and tuple(t.shape) == w.shape and w.shape[0] == bins
    assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
    assert np.array_equal(np.ascontiguousarray(t.cpu().numpy()).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    for k in range(bins):
        untouched[int(o) + k * int(p) * c:int(o) + (k * int(p) + w.shape[1]) * c] = False
host = out.cpu()
assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
frec = rec.copy()
frec["layout"] = pkg.MEL_FRAMES_MAJOR
fm, _ = ctx.decode_files(None, batch=b, features=frec, resample=44100, mono=True, out=out)
assert all(t.dtype == torch.complex64 and np.array_equal(t.cpu().numpy().T.copy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32)) for t, w in zip(fm, want))
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(features=fft_sep's record, out=tensor): straight into a float32 torch tensor of stft_layout's size, the
    spectrograms complex64 views of it equal to the numpy route, every element outside them as it was; frames-major the transpose.
    In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout


# ---- STFT batches -------------------------------------------------------------------------------------------
def test_stft_batches_over_fft(pkg, ctx):
    """STFT BATCHES with an fft_vits record: the direct path (a stride of a multiple of 64, no norm: k_tracks_fft writes the tensor as
    its grid) and the path through the scratch grid (an odd stride) both equal the packed call collated in numpy, bit for bit, so
    they give the same tensor over the frames both hold; a "refmax" request equals the same request over the packed FFT grid."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    for layout in ("bands", "frames"):
        rec = fft_of(pkg, "fft_vits", layout)
        planned_f = pkg.stft_frames(rec, -(-b.info["track_samples"] * 147 // 320))
        kw = dict(batch=b, features=rec, resample=22050, mono=True)
        packed, pinfo = ctx.decode_files(None, **kw)
        direct, odd = strides_for(planned_f)
        tensors = []
        for extra in (dict(stft_stride=direct), dict(stft_stride=odd), dict(stft_stride=odd, stft_normalize="refmax")):
            req = pkg.files_request(b, features=rec, resample=22050, mono=True, **extra)
            dense, dinfo = ctx.decode_files(None, **kw, **extra)
            assert dense_equals(pkg, dense, dinfo, packed, pinfo, rec, req.stft_batch) > 10000, extra
            tensors.append(dense if layout == "frames" else dense.transpose(0, 2, 1))
        m = min(direct, odd)
        assert tensors[0].shape[1] == direct and tensors[1].shape[1] == odd
        assert np.array_equal(np.ascontiguousarray(tensors[0][:, :m]).view(np.uint32), np.ascontiguousarray(tensors[1][:, :m]).view(np.uint32))
        again, ainfo = ctx.decode_files(None, **kw)  # the request is gone
        assert np.array_equal(ainfo, pinfo) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(again, packed))
    b.close()
