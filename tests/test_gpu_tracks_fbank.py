"""Kaldi fbank and MFCC features of the whole-file path on the GPU (include/opusgpu.h TRACK KALDI FEATURES: k_tracks_fbank,
opusgpu_files_decode_fbank, opusgpu_ms_files_decode_fbank).  The kernel alone on crafted tracks in buffers of guard words against
tests/test_tracks_fbank.py::fbank_ref (float64) within TOL, and its exact properties, for the six parameter sets of SETS; whole files
bit for bit against the kernel alone run over the int16 mono tracks of the same planned batch (which the rate, ratio and mix tests
hold against their integer references).

TOL: 8 x YARDSTICK of tests/test_tracks_fbank.py, the largest error of fbank_f32 against fbank_ref over the kept cells of
crafted_tracks, per set; test_kernel_alone prints it next to the kernel's own worst error.
On an MI355X the kernel's own worst error on those cells, both layouts alike: wenet 2.57e-04, mfcc8k 9.92e-05, nosnip 2.15e-05,
tiny 2.69e-07, wide 5.94e-05, far 4.94e-05.
Tiles (the largest of 128, 64, 32 frames whose window fits 32,768 samples): wenet, mfcc8k, nosnip and tiny 128, wide 64, far 32."""
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import stereo_files
from test_tracks_fbank import SETS, TILES, TOL, YARDSTICK, crafted, dct64, dims, error_of, fbank_ref, frame_count, is_flat, kept_cells, spec_of, tile_of, \
    width_of, yardstick

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32 = 0x5A5A5A5A


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def lay_out(pkg, rng, tracks, scales, rec):
    """The input buffer -- garbage everywhere, every track at a multiple of 8 samples with garbage behind its length -- the spans,
    and the size of the output buffer: tracks at multiples of 64 floats with room between them that must stay guard."""
    width = width_of(rec)
    spans = np.zeros(len(tracks), dtype=pkg.MEL_SPAN_DTYPE)
    at_in = at_out = 0
    for i, y in enumerate(tracks):
        F = frame_count(rec, len(y))
        plane = (F + 63) // 64 * 64 + 64 * int(rng.integers(0, 2))
        spans[i] = (at_in, len(y), at_out, plane, scales[i], 0)
        at_in = (at_in + len(y) + int(rng.integers(0, 40)) + 7) // 8 * 8
        at_out += width * plane + 64 * int(rng.integers(0, 2))
    buf = rng.integers(-32768, 32768, at_in + 64, dtype=np.int16)
    for sp, y in zip(spans, tracks):
        buf[sp["in_offset"]:sp["in_offset"] + len(y)] = y
    return buf, spans, at_out + 64


def cells_of(sp, F, width, frames_major):
    """Indices [F, width] of a feature track's cells in the output buffer."""
    f, j = np.arange(F)[:, None], np.arange(width)[None, :]
    return sp["out_offset"] + (f * width + j if frames_major else j * sp["plane"] + f)


def run_kernel(ctx, buf, spans, total, rec, runs=1):
    fill = np.full(total, GUARD32, dtype=np.uint32)
    d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
    got = []
    try:
        ctx.h2d(d_in, buf)
        ctx.h2d(d_out, fill)
        ctx.tracks_fbank_device(spans[:0], d_in, rec, d_out)  # no track: nothing
        none = np.zeros_like(fill)
        ctx.d2h(none, d_out)
        assert (none == GUARD32).all()
        for _ in range(runs):
            ctx.tracks_fbank_device(spans, d_in, rec, d_out)
            g = np.zeros_like(fill)
            ctx.d2h(g, d_out)
            got.append(g)
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    return got


# ---- the kernel alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["bands", "frames"])
@pytest.mark.parametrize("name", list(SETS))
def test_kernel_alone(pkg, ctx, name, layout):
    """k_tracks_fbank on crafted_tracks in one launch: every kept cell within TOL of fbank_ref, at most 1 % of the cells not kept and
    more than 500 judged, every element outside the tracks' cells an untouched guard word, the all-zero track and (with remove_dc)
    the constant track one bit pattern per feature at the floor's value, a second run the same bits."""
    _, tracks, scales, refs = crafted(pkg, name)
    rec = spec_of(pkg, name, layout)
    assert tile_of(rec) == TILES[name]
    width, frames_major = width_of(rec), layout == "frames"
    rng = np.random.default_rng(len(name) + frames_major)
    buf, spans, total = lay_out(pkg, rng, tracks, scales, rec)
    first, second = run_kernel(ctx, buf, spans, total, rec, runs=2)
    assert np.array_equal(first, second)  # the same bits
    written = np.zeros(total, dtype=bool)
    cells = dropped = flat = 0
    worst = 0.0
    L, H = dims(rec)[:2]
    floor_row = fbank_ref(np.zeros(L + H, dtype=np.int16), 1.0, rec)[0][0]  # what an all-zero frame gives, per feature
    # how far a float32 result may lie from it: a few ulp of logf(floor); for MFCC the worst case of a float32 sum of n_mels
    # products of that size, the table's rounding included
    flat_tol = 1e-6 * max(1.0, np.abs(floor_row).max())
    if int(rec["n_ceps"][0]):
        flat_tol = 2 * dims(rec)[3] * 2.0 ** -24 * np.abs(dct64(rec) * np.log(float(rec["floor"][0]))).sum(axis=1).max()
    for i, (sp, y, (ref, mel)) in enumerate(zip(spans, tracks, refs)):
        F = frame_count(rec, len(y))
        assert ref.shape == (F, width)
        if not F:
            continue  # no frame: no cell, nothing written (the guards below)
        at = cells_of(sp, F, width, frames_major)
        assert not written[at].any()
        written[at] = True
        got = first[at].view(np.float32)
        assert np.isfinite(got).all(), i
        keep = kept_cells(mel, rec)
        cells, dropped = cells + keep.size, dropped + int((~keep).sum())
        err = error_of(got, ref, rec)
        worst = max(worst, float(err[keep].max(initial=0)))
        assert (err[keep] <= TOL[name]).all(), (i, len(y), float(sp["scale"]), float(err[keep].max()), TOL[name], np.argwhere(err * keep > TOL[name])[:4])
        if not y.any() or (is_flat(y) and int(rec["remove_dc"][0])):  # one bit pattern per feature, the value of the floor
            flat += 1
            assert (first[at] == first[at][:1]).all()
            assert np.abs(got[0].astype(np.float64) - floor_row).max() <= flat_tol
            if not int(rec["n_ceps"][0]):
                assert len(np.unique(first[at])) == 1
    print(f"{name} {layout}: tile {TILES[name]}, {cells} cells, {dropped} not kept, worst error {worst:.3g} (allowed {TOL[name]:.3g}, "
          f"float32 numpy {yardstick(pkg, name):.3g}, recorded {YARDSTICK[name]:.3g})")
    assert cells > 500 and dropped <= 0.01 * cells
    assert flat == (2 if int(rec["remove_dc"][0]) else 1)
    assert (first[~written] == GUARD32).all(), np.nonzero(first[~written] != GUARD32)[0][:8]  # padding is never written


def test_no_frame_writes_nothing(pkg, ctx):
    """Tracks without a frame alone -- n < L with snip_edges, n < H - H / 2 without --: not a word of the output changes."""
    rng = np.random.default_rng(3)
    for name, ns in (("wenet", (0, 1, 8, 399)), ("nosnip", (0, 79)), ("tiny", (0, 24)), ("far", (0, 1, 499))):
        rec = spec_of(pkg, name)
        tracks = [rng.integers(-32768, 32768, n, dtype=np.int16) for n in ns]
        buf, spans, total = lay_out(pkg, rng, tracks, np.ones(len(ns), dtype=np.float32), rec)
        spans["plane"] = 64
        (got,) = run_kernel(ctx, buf, spans, total + 64 * 80 * 4, rec)
        assert (got == GUARD32).all()


# ---- whole files --------------------------------------------------------------------------------------------
def kernel_over_tracks(pkg, ctx, tracks16, scales, offsets, planes, total, rec):
    """tracks_fbank_device over int16 tracks [m, 1] laid out on the grid decode_files reports -> the packed float32 buffer (as uint32)."""
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
    """feats, info = decode_files(features=rec) of the batch whose int16 mono tracks at up / down of 48 kHz are tracks16: the grid, the
    frame counts and every cell, bit for bit.  -> the number of cells."""
    width, frames_major = width_of(rec), int(rec["layout"][0]) == 1
    offs, planes, total = pkg.fbank_layout(planned, up, down, rec)
    assert np.array_equal(info["feat_offset"], offs) and (offs % 64 == 0).all()
    assert np.array_equal(info["frames"], [frame_count(rec, len(y)) for y in tracks16])
    assert np.array_equal(info["frames"], pkg.fbank_frames(rec, -(-info["track_samples"] * up // down)))
    want = kernel_over_tracks(pkg, ctx, tracks16, scales, offs, planes, total, rec)
    cells = 0
    for sp_off, plane, F, g in zip(offs, planes, info["frames"], feats):
        assert g.dtype == np.float32 and g.shape == ((F, width) if frames_major else (width, F))
        at = cells_of({"out_offset": sp_off, "plane": plane}, F, width, frames_major)
        w = want[at] if frames_major else want[at].T
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), w)
        cells += g.size
    return cells


@pytest.mark.parametrize("name,how,pipeline", [("wenet", dict(rate=16000, mono=True), 1), ("at22k", dict(resample=22050, mono=True), 0)])
def test_files_fbank(pkg, ctx, name, how, pipeline):
    """decode_files(features=record) of the stereo corpus and the files whose frame fails on the device equals tracks_fbank_device
    over the int16 tracks of decode_files with the same rate or ratio, bit for bit; a failed track reports its shorter F and keeps
    its planned plane; scale= reaches the samples; loudness= folds its gain into the scale."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    planned = b.info["track_samples"].copy()
    rec = spec_of(pkg, "wenet", "frames" if pipeline else "bands") if name == "wenet" else pkg.kaldi_fbank(sample_rate=22050, num_mel_bins=40,
                                                                                                           snip_edges=False, feature_layout="bands")
    up, down = {"wenet": (1, 3), "at22k": (147, 320)}[name]
    t16, i16 = ctx.decode_files(None, batch=b, **how)
    scales = np.ones(len(files), dtype=np.float32)  # Kaldi's int16-range convention
    feats, info = ctx.decode_files(None, batch=b, features=rec, scale=scales, **how)
    for field in i16.dtype.names:
        if field not in ("out_samples", "out_offset", "frames"):  # (`frames` is F here, the plan's count of Opus frames there)
            assert np.array_equal(i16[field], info[field]), field
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, up, down) > 10000
    assert any(x is not None for x in bad)
    _, planes, _ = pkg.fbank_layout(planned, up, down, rec)
    for i, seq in enumerate(bad):
        if seq is not None:
            final = b.packet_start(i, seq)
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, seq)
            assert info["track_samples"][i] == final < planned[i]
            assert info["frames"][i] == frame_count(rec, -(-final * up // down)) < frame_count(rec, -(-int(planned[i]) * up // down))
            assert planes[i] == (frame_count(rec, -(-int(planned[i]) * up // down)) + 63) // 64 * 64
    if name == "wenet":  # the record's rate alone names the track, and the default scale is 1 / 32768
        again, ainfo = ctx.decode_files(None, batch=b, features=rec, mono=True, format="f32")
        assert np.array_equal(ainfo, info)
        assert same_as_kernel_alone(pkg, ctx, t16, again, ainfo, planned, np.full(len(files), 2.0 ** -15, dtype=np.float32), rec, up, down) > 10000
        assert not all(np.array_equal(x, y) for x, y in zip(again, feats))
        # loudness=-23.0: the gain of every track on top of scale=, folded into the kernel's scale
        loud, linfo = ctx.decode_files(None, batch=b, features=rec, scale=scales, loudness=-23.0, **how)
        gains = (scales.astype(np.float64) * linfo["gain"]).astype(np.float32)
        plain = np.zeros(len(files), dtype=info.dtype)
        for field in info.dtype.names:
            plain[field] = linfo[field]
        assert np.array_equal(plain, info) and (linfo["gain"] != 1.0).any()
        assert same_as_kernel_alone(pkg, ctx, t16, loud, plain, planned, gains, rec, up, down) > 10000
    b.close()


def test_surround_mfcc(pkg, ctx):
    """A 5.1 layout through mix="mono" with the mfcc8k set at rate=8000: equal to the kernel alone over decode_files(rate=8000,
    mix="mono")."""
    layout = LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    planned = b.info["track_samples"].copy()
    rec = spec_of(pkg, "mfcc8k")
    t16, _ = ms.decode_files(None, batch=b, rate=8000, mix="mono")
    feats, info = ms.decode_files(None, batch=b, features=rec, rate=8000, mix="mono", scale=1.0)
    scales = np.ones(n, dtype=np.float32)
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, rec, 1, 6) > 500
    assert all(f.shape[1] == 13 for f in feats)
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, features=rec, rate=8000, mix="stereo")
    b.close()
    ms.close()


def test_files_refusals_through_the_c_abi(pkg, ctx):
    """opusgpu_files_decode_fbank with a real context, a real batch and real buffers: every refusal is OPUSGPU_BAD_ARG and leaves the
    output buffer and the caller's arrays as they were -- a record whose sample_rate is not the track's among them --; then a call
    in order works."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2)
    n = b.n_files
    good, at22k = spec_of(pkg, "wenet"), pkg.kaldi_fbank(sample_rate=22050)
    total = max(pkg.fbank_layout(b.info["track_samples"], 1, 3, good)[2], pkg.fbank_layout(b.info["track_samples"], 147, 320, at22k)[2])
    fill = np.full(total + 64, GUARD32, dtype=np.uint32)
    d_out = ctx.dev_alloc(fill.nbytes)
    mono_mix, two = pkg.mix_matrix("mono", 2), pkg.mix_matrix("stereo", 2)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)

    def call(rate, up, down, mono, mix, p, scale, out):
        return ctx.lib.opusgpu_files_decode_fbank(ctx.h, b.h, rate, up, down, mono, None if mix is None else mix.ctypes.data, p.ctypes.data,
                                                  None if scale is None else scale.ctypes.data, out, *[a.ctypes.data for a in arrays])

    def params(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    try:
        ctx.h2d(d_out, fill)
        for rate, up, down, mono, mix, p, scale, out in (
                (16000, 0, 0, 1, None, params(n_mels=129), None, d_out), (16000, 0, 0, 1, None, params(layout=3), None, d_out),
                (16000, 0, 0, 1, None, params(reserved=[1, 0]), None, d_out), (16000, 0, 0, 1, None, params(n_fft=500), None, d_out),
                (16000, 0, 0, 1, None, params(frame_shift=0), None, d_out), (16000, 0, 0, 1, None, params(floor=0.0), None, d_out),
                (16000, 0, 0, 1, None, params(high_freq=8001.0), None, d_out), (16000, 0, 0, 1, None, params(n_ceps=13, log=0), None, d_out),
                (16000, 0, 0, 0, None, good, None, d_out), (16000, 0, 0, 1, mono_mix, good, None, d_out), (16000, 0, 0, 0, two, good, None, d_out),
                (16000, 0, 0, 1, None, good, nan, d_out), (16000, 0, 0, 1, None, good, None, d_out.value + 64),
                (24000, 0, 0, 1, None, good, None, d_out), (16000, 0, 0, 1, None, at22k, None, d_out), (0, 147, 320, 1, None, good, None, d_out),
                (16000, 1, 3, 1, None, good, None, d_out), (22050, 0, 0, 1, None, at22k, None, d_out), (0, 3, 1, 1, None, good, None, d_out),
                (0, 0, 0, 1, None, good, None, d_out)):
            assert call(rate, up, down, mono, mix, p, scale, out) == pkg.OPUSGPU_BAD_ARG
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all() and all((a == -7).all() for a in arrays)
        assert call(16000, 0, 0, 1, None, good, None, d_out) == 0  # and the call in order works
        assert np.array_equal(arrays[1], pkg.fbank_frames(good, -(-arrays[2] // 3)))
        assert call(0, 147, 320, 0, mono_mix, at22k, None, d_out) == 0
        assert np.array_equal(arrays[1], pkg.fbank_frames(at22k, -(-arrays[2] * 147 // 320)))
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
rec = pkg.kaldi_fbank(num_mel_bins=80)
ones = 1.0
want, winfo = ctx.decode_files(None, batch=b, features=rec, rate=16000, mono=True, scale=ones)
offs, planes, total = pkg.fbank_layout(b.info["track_samples"], 1, 3, rec)
FILL = 12345.5
out = torch.full((total + 256,), FILL, dtype=torch.float32, device="cuda:0")
feats, info = ctx.decode_files(None, batch=b, features=rec, rate=16000, mono=True, scale=ones, out=out)
assert np.array_equal(info, winfo) and len(feats) == len(files) and sum(w.size for w in want) > 5000
untouched = torch.ones(total + 256, dtype=torch.bool)
for t, w, o in zip(feats, want, offs):
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == w.shape and w.shape[1] == 80
    assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
    assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    untouched[int(o):int(o) + w.size] = False
host = out.cpu()
assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
brec = rec.copy()
brec["layout"] = pkg.MEL_BANDS_MAJOR
bm, _ = ctx.decode_files(None, batch=b, features=brec, mono=True, scale=ones, out=out)
assert all(np.array_equal(t.cpu().numpy().T.copy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32)) for t, w in zip(bm, want))
before = out.clone()
for bad in (out[1:], out.to(torch.float64), out[:total - 1], out[::2], out.cpu()):
    try:
        ctx.decode_files(None, batch=b, features=rec, mono=True, out=bad)
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
assert bool((out == before).all())  # a short `out` raises and leaves no device work behind
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(features=kaldi_fbank(num_mel_bins=80), rate=16000, mono=True, scale=1.0 each, out=tensor): straight into a torch
    tensor of fbank_layout's size, the features views of it equal to the numpy route, every element outside them as it was; a tensor
    that does not fit raises before any device work.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
