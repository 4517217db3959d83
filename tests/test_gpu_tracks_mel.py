"""Log-mel features of the whole-file path on the GPU (include/opusgpu.h TRACK FEATURES: k_tracks_mel, opusgpu_files_decode_mel,
opusgpu_ms_files_decode_mel).  The kernel alone on crafted tracks in buffers of guard words against
tests/test_tracks_mel.py::logmel_ref (float64) within TOL, and its exact properties; whole files bit for bit against the kernel
alone run over the int16 16 kHz mono tracks of the same planned batch (which tests/test_gpu_tracks_resample.py and
tests/test_gpu_tracks_mix.py hold against their integer references).

TOL: 8 x the largest |d log10| of logmel_f32 -- float32 numpy with the library's tables -- against logmel_ref over the kept cells
of crafted_tracks (measured on a CPU: 80 bands 8.30e-05, 128 bands 8.29e-05, both in a narrow low band whose weights are
small, 71 dB under its frame's largest).  yardstick() recomputes it."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import stereo_files
from test_tracks_mel import logmel_f32, logmel_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32 = 0x5A5A5A5A
T = 128  # MEL_T, the kernel's tile in frames
LENGTHS = [0, 1, 159, 160, 161, 199, 200, 201, 319, 320, 559, 560, 160 * T - 1, 160 * T, 160 * T + 1, 160 * T + 161]
YARDSTICK = {80: 8.30e-05, 128: 8.29e-05}
TOL = {n: 8 * v for n, v in YARDSTICK.items()}


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def crafted_tracks():
    """(tracks, scales): every length of LENGTHS twice, uniform random int16 -- once with the default scale, once with a random
    finite one --, an all-zero track and a track of +-40 noise."""
    rng = np.random.default_rng(20)
    tracks, scales = [], []
    for n in LENGTHS:
        for k in range(2):
            tracks.append(rng.integers(-32768, 32768, n, dtype=np.int16))
            scales.append(2.0 ** -15 if k == 0 else float(rng.choice([-1, 1]) * rng.uniform(1, 10) * 10.0 ** rng.integers(-6, 3)))
    tracks.append(np.zeros(160 * 5 + 3, dtype=np.int16))
    scales.append(2.0 ** -15)
    tracks.append(rng.integers(-40, 41, 160 * 9 + 77, dtype=np.int16))
    scales.append(2.0 ** -15)
    scales = np.asarray(scales, dtype=np.float32)
    assert np.isfinite(scales).all() and (scales != 0).all()
    return tracks, scales


@functools.lru_cache(maxsize=None)
def crafted_reference(n_mels):
    """logmel_ref of crafted_tracks: [(log10 [F, n_mels], mel [F, n_mels])], computed once per n_mels."""
    tracks, scales = crafted_tracks()
    return [logmel_ref(y, s, n_mels) for y, s in zip(tracks, scales)]


def kept_cells(mel):
    """The cells the tolerance is held on: float64 mel at least 1e-8 x its frame's largest."""
    return mel >= 1e-8 * mel.max(axis=1, keepdims=True) if mel.size else np.zeros(mel.shape, dtype=bool)


def yardstick(pkg, n_mels):
    tracks, scales = crafted_tracks()
    wc, ws = pkg.mel_basis()
    B = pkg.mel_filterbank(n_mels)
    worst = 0.0
    for y, s, (ref, mel) in zip(tracks, scales, crafted_reference(n_mels)):
        if len(ref):
            worst = max(worst, float(np.abs(logmel_f32(y, s, n_mels, wc, ws, B) - ref)[kept_cells(mel)].max(initial=0)))
    return worst


def lay_out(pkg, rng, tracks, scales, n_mels, frames_major):
    """The input buffer -- garbage everywhere, every track at a multiple of 8 samples with garbage behind its length -- the spans,
    and the size of the output buffer: tracks at multiples of 64 floats with room between them that must stay guard."""
    spans = np.zeros(len(tracks), dtype=pkg.MEL_SPAN_DTYPE)
    at_in = at_out = 0
    for i, y in enumerate(tracks):
        F = len(y) // 160
        plane = (F + 63) // 64 * 64 + 64 * int(rng.integers(0, 2))
        spans[i] = (at_in, len(y), at_out, plane, scales[i], 0)
        at_in = (at_in + len(y) + int(rng.integers(0, 40)) + 7) // 8 * 8
        at_out += n_mels * plane + 64 * int(rng.integers(0, 2))
    buf = rng.integers(-32768, 32768, at_in + 64, dtype=np.int16)
    for sp, y in zip(spans, tracks):
        buf[sp["in_offset"]:sp["in_offset"] + len(y)] = y
    return buf, spans, at_out + 64


def cells_of(sp, F, n_mels, frames_major):
    """Indices [F, n_mels] of a feature track's cells in the output buffer."""
    f, j = np.arange(F)[:, None], np.arange(n_mels)[None, :]
    return sp["out_offset"] + (f * n_mels + j if frames_major else j * sp["plane"] + f)


def run_kernel(pkg, ctx, buf, spans, total, n_mels, layout, runs=1):
    fill = np.full(total, GUARD32, dtype=np.uint32)
    d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
    got = []
    try:
        ctx.h2d(d_in, buf)
        ctx.h2d(d_out, fill)
        ctx.tracks_mel_device(spans[:0], d_in, n_mels, layout, d_out)  # no track: nothing
        none = np.zeros_like(fill)
        ctx.d2h(none, d_out)
        assert (none == GUARD32).all()
        for _ in range(runs):
            ctx.tracks_mel_device(spans, d_in, n_mels, layout, d_out)
            g = np.zeros_like(fill)
            ctx.d2h(g, d_out)
            got.append(g)
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    return got


# ---- the kernel alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,layout", [(80, "bands"), (80, "frames"), (128, "bands"), (128, "frames")])
def test_kernel_alone(pkg, ctx, n_mels, layout):
    """k_tracks_mel on crafted_tracks in one launch: every kept cell within TOL of logmel_ref, at most 1 % of the cells not kept,
    every element outside the tracks' cells an untouched guard word, the all-zero track one value, a second run the same bits."""
    tracks, scales = crafted_tracks()
    refs = crafted_reference(n_mels)
    frames_major = layout == "frames"
    rng = np.random.default_rng(n_mels + frames_major)
    buf, spans, total = lay_out(pkg, rng, tracks, scales, n_mels, frames_major)
    first, second = run_kernel(pkg, ctx, buf, spans, total, n_mels, layout, runs=2)
    assert np.array_equal(first, second)  # the same bits
    written = np.zeros(total, dtype=bool)
    cells = dropped = 0
    worst = 0.0
    for i, (sp, y, (ref, mel)) in enumerate(zip(spans, tracks, refs)):
        F = len(y) // 160
        assert ref.shape == (F, n_mels)
        if not F:
            continue  # n < 160: no cell, nothing written (the guards below)
        at = cells_of(sp, F, n_mels, frames_major)
        assert not written[at].any()
        written[at] = True
        got = first[at].view(np.float32)
        assert np.isfinite(got).all(), i
        keep = kept_cells(mel)
        cells, dropped = cells + keep.size, dropped + int((~keep).sum())
        err = np.abs(got.astype(np.float64) - ref)[keep]
        worst = max(worst, float(err.max(initial=0)))
        assert (err <= TOL[n_mels]).all(), (i, len(y), float(sp["scale"]), float(err.max()), TOL[n_mels], np.argwhere(np.abs(got - ref) * keep > TOL[n_mels])[:4])
        if not y.any():  # the all-zero track
            assert len(np.unique(first[at])) == 1 and abs(float(got[0, 0]) + 10.0) <= 1e-6
    print(f"n_mels {n_mels} {layout}: {cells} cells, {dropped} not kept, worst |d log10| {worst:.3g} (allowed {TOL[n_mels]:.3g}, "
          f"float32 numpy {yardstick(pkg, n_mels):.3g})")
    assert cells > 80000 and dropped <= 0.01 * cells
    assert (first[~written] == GUARD32).all(), np.nonzero(first[~written] != GUARD32)[0][:8]  # padding is never written


def test_no_frame_writes_nothing(pkg, ctx):
    """Tracks with n < 160 alone: 0 frames, not a word of the output changes."""
    rng = np.random.default_rng(3)
    tracks = [rng.integers(-32768, 32768, n, dtype=np.int16) for n in (0, 1, 8, 159)]
    buf, spans, total = lay_out(pkg, rng, tracks, np.ones(4, dtype=np.float32), 80, False)
    spans["plane"] = 64
    (got,) = run_kernel(pkg, ctx, buf, spans, total + 64 * 80 * 4, 80, "bands")
    assert (got == GUARD32).all()


def test_kernel_refusals(pkg, ctx):
    """With a real context and real buffers: what the call refuses changes nothing in the output buffer."""
    spans = np.zeros(1, dtype=pkg.MEL_SPAN_DTYPE)
    spans[0] = (0, 400, 0, 64, 1.0, 0)
    buf = np.zeros(512, dtype=np.int16)
    fill = np.full(64 * 128 + 256, GUARD32, dtype=np.uint32)
    d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(d_in, buf)
        ctx.h2d(d_out, fill)
        for n_mels, layout in ((64, 0), (80, 2), (128, -1), (0, 0)):
            rec = pkg.mel_params(80, "bands")
            rec["n_mels"], rec["layout"] = n_mels, layout
            with pytest.raises(pkg.OpusGpuError):
                ctx.tracks_mel_device(spans, d_in, rec, None, d_out)
        rec = pkg.mel_params(80, "bands")
        rec["reserved"][0, 3] = 1
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_mel_device(spans, d_in, rec, None, d_out)
        for field, value in (("in_offset", 4), ("out_offset", 32), ("plane", 0), ("plane", 96), ("scale", np.inf), ("in_samples", -1)):
            s = spans.copy()
            s[field] = value
            with pytest.raises(pkg.OpusGpuError):
                ctx.tracks_mel_device(s, d_in, 80, "bands", d_out)
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_mel_device(spans, d_in.value + 2, 80, "bands", d_out)  # d_in not 16-byte aligned
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_mel_device(spans, d_in, 80, "bands", d_out.value + 64)  # d_out not 128-byte aligned
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all()
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)


# ---- whole files --------------------------------------------------------------------------------------------
def kernel_over_tracks(pkg, ctx, tracks16, scales, offsets, planes, total, n_mels, layout):
    """tracks_mel_device over int16 tracks [m, 1] laid out on the grid decode_files reports -> the packed float32 buffer (as uint32)."""
    spans = np.zeros(len(tracks16), dtype=pkg.MEL_SPAN_DTYPE)
    at = 0
    for i, y in enumerate(tracks16):
        spans[i] = (at, len(y), offsets[i], planes[i], scales[i], 0)
        at = (at + len(y) + 63) // 64 * 64
    buf = np.full(at + 64, -12345, dtype=np.int16)
    for sp, y in zip(spans, tracks16):
        buf[sp["in_offset"]:sp["in_offset"] + len(y)] = y[:, 0]
    return run_kernel(pkg, ctx, buf, spans, max(total, 1), n_mels, layout)[0]


def same_as_kernel_alone(pkg, ctx, tracks16, feats, info, planned, scales, n_mels, layout):
    """feats, info = decode_files(features="logmel") of the batch whose int16 16 kHz mono tracks are tracks16: the grid, the frame
    counts and every cell, bit for bit.  -> the number of cells."""
    offs, planes, total = pkg.mel_layout(planned, n_mels, layout)
    assert np.array_equal(info["feat_offset"], offs) and (offs % 64 == 0).all()
    assert np.array_equal(info["frames"], [len(y) // 160 for y in tracks16])
    assert np.array_equal(info["frames"], -(-info["track_samples"] // 3) // 160)
    want = kernel_over_tracks(pkg, ctx, tracks16, scales, offs, planes, total, n_mels, layout)
    cells = 0
    for sp_off, plane, F, g in zip(offs, planes, info["frames"], feats):
        assert g.dtype == np.float32 and g.shape == ((F, n_mels) if layout == "frames" else (n_mels, F))
        at = cells_of({"out_offset": sp_off, "plane": plane}, F, n_mels, layout == "frames")
        w = want[at] if layout == "frames" else want[at].T
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint32), w)
        cells += g.size
    return cells


@pytest.mark.parametrize("pipeline", [0, 1])
def test_files_logmel(pkg, ctx, pipeline):
    """decode_files(features="logmel", mono=True) of the stereo corpus and the files whose frame fails on the device equals
    tracks_mel_device over the int16 tracks of decode_files(rate=16000, mono=True), bit for bit; a failed track reports its shorter
    F and keeps its planned plane; mix="mono" is mono=True."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    planned = b.info["track_samples"].copy()
    t16, i16 = ctx.decode_files(None, batch=b, rate=16000, mono=True)
    scales = np.full(len(files), 2.0 ** -15, dtype=np.float32)
    n_mels, layout = (80, "bands") if pipeline == 0 else (128, "frames")
    feats, info = ctx.decode_files(None, batch=b, features="logmel", mono=True, n_mels=n_mels, feature_layout=layout)
    for field in i16.dtype.names:
        if field not in ("out_samples", "out_offset", "frames"):  # (`frames` is F here, the plan's count of Opus frames there)
            assert np.array_equal(i16[field], info[field]), field
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, n_mels, layout) > 10000
    assert any(x is not None for x in bad)
    _, planes, _ = pkg.mel_layout(planned, n_mels, layout)
    for i, seq in enumerate(bad):
        if seq is not None:
            final = b.packet_start(i, seq)
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, seq)
            assert info["track_samples"][i] == final < planned[i] and info["frames"][i] == -(-final // 3) // 160
            assert planes[i] == (-(-planned[i] // 3) // 160 + 63) // 64 * 64
    mixed, minfo = ctx.decode_files(None, batch=b, features="logmel", mix="mono", rate=16000, format="f32", n_mels=n_mels, feature_layout=layout)
    assert np.array_equal(minfo, info) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(mixed, feats))
    gains = np.linspace(0.5, 2.0, len(files)).astype(np.float32) / 32768
    scaled, _ = ctx.decode_files(None, batch=b, features="logmel", mono=True, scale=gains, n_mels=n_mels, feature_layout=layout)
    assert same_as_kernel_alone(pkg, ctx, t16, scaled, info, planned, gains, n_mels, layout) > 10000
    b.close()


def test_surround_logmel(pkg, ctx):
    """A 5.1 layout, mix="mono", frames-major: equal to the kernel alone over decode_files(rate=16000, mix="mono")."""
    layout = LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    planned = b.info["track_samples"].copy()
    t16, _ = ms.decode_files(None, batch=b, rate=16000, mix="mono")
    feats, info = ms.decode_files(None, batch=b, features="logmel", mix="mono", feature_layout="frames")
    scales = np.full(n, 2.0 ** -15, dtype=np.float32)
    assert same_as_kernel_alone(pkg, ctx, t16, feats, info, planned, scales, 80, "frames") > 5000
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, features="logmel", mix="stereo")
    b.close()
    ms.close()


def test_files_refusals_through_the_c_abi(pkg, ctx):
    """opusgpu_files_decode_mel with a real context, a real batch and real buffers: every refusal is OPUSGPU_BAD_ARG and leaves the
    output buffer and the caller's arrays as they were."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2)
    n = b.n_files
    total = pkg.mel_layout(b.info["track_samples"], 128, "bands")[2]
    fill = np.full(total + 64, GUARD32, dtype=np.uint32)
    d_out = ctx.dev_alloc(fill.nbytes)
    good, mono_mix, two = pkg.mel_params(80, "bands"), pkg.mix_matrix("mono", 2), pkg.mix_matrix("stereo", 2)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)

    def call(mono, mix, p, scale, out):
        return ctx.lib.opusgpu_files_decode_mel(ctx.h, b.h, mono, None if mix is None else mix.ctypes.data, p.ctypes.data,
                                                None if scale is None else scale.ctypes.data, out, *[a.ctypes.data for a in arrays])

    def params(**kw):
        rec = good.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    try:
        ctx.h2d(d_out, fill)
        for mono, mix, p, scale, out in ((1, None, params(n_mels=64), None, d_out), (1, None, params(layout=3), None, d_out),
                                         (1, None, params(reserved=[1, 0, 0, 0, 0, 0]), None, d_out), (0, None, good, None, d_out),
                                         (1, mono_mix, good, None, d_out), (0, two, good, None, d_out), (1, None, good, nan, d_out),
                                         (1, None, good, None, d_out.value + 64)):
            assert call(mono, mix, p, scale, out) == pkg.OPUSGPU_BAD_ARG
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all() and all((a == -7).all() for a in arrays)
        assert call(1, None, good, None, d_out) == 0 and (arrays[1] == -(-arrays[2] // 3) // 160).all()  # and the call in order works
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
want, winfo = ctx.decode_files(None, batch=b, features="logmel", mono=True)
offs, planes, total = pkg.mel_layout(b.info["track_samples"], 80, "bands")
FILL = 12345.5
out = torch.full((total + 256,), FILL, dtype=torch.float32, device="cuda:0")
feats, info = ctx.decode_files(None, batch=b, features="logmel", mono=True, out=out)
assert np.array_equal(info, winfo) and len(feats) == len(files) and sum(w.size for w in want) > 5000
untouched = torch.ones(total + 256, dtype=torch.bool)
for t, w, o, p in zip(feats, want, offs, planes):
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == w.shape and w.shape[0] == 80
    assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
    assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
    for j in range(80):
        untouched[int(o) + j * int(p):int(o) + j * int(p) + w.shape[1]] = False
host = out.cpu()
assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
fm, _ = ctx.decode_files(None, batch=b, features="logmel", mono=True, feature_layout="frames", out=out)
assert all(np.array_equal(t.cpu().numpy().T.copy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32)) for t, w in zip(fm, want))
before = out.clone()
for bad in (out[1:], out.to(torch.float64), out[:total - 1], out[::2], out.cpu()):
    try:
        ctx.decode_files(None, batch=b, features="logmel", mono=True, feature_layout="frames", out=bad)
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
assert bool((out == before).all())  # a short `out` raises and leaves no device work behind
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(features="logmel", out=tensor): straight into a torch tensor of mel_layout's size, the features views of it
    equal to the numpy route, every element outside them as it was; a tensor that does not fit raises before any device work.  In
    a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
