"""Track ratios of the whole-file path on the GPU (include/opusgpu.h TRACK RATIOS: k_tracks_resample_ratio, opusgpu_files_decode_ratio,
opusgpu_ms_files_decode_ratio).  A resampled track is a pure integer function of the S16 track, so every check here is bit for bit
against tests/test_tracks_resample_ratio.py::resample_ratio_ref with the taps opusgpu_resample_ratio_taps hands out: the kernel
alone on crafted tracks in a buffer of guard words, whole files against resample_ratio_ref of the S16 tracks of the same planned
batch (which tests/test_gpu_files.py and tests/test_gpu_ms_files.py hold against the reader and the oracle)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import GUARD16, GUARD32, as_format, raw, stereo_files
from test_tracks_resample_ratio import resample_ratio_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["s16", "f32", "f32_planar"]
TILES = (256, 512, 1024)  # the kernel's tile lengths in outputs, by output channels (8 .. 3, 2, 1)


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ---- the kernel alone -------------------------------------------------------------------------------------
def crafted_tracks(rng, C, up, down, taps, tiles=TILES, count=200):
    """About `count` tracks [in_samples, C]: every length at which the kernel takes another path -- none, one sample, around one
    output, around the filter's half length 12 down / up, around one and two tiles of every tile length, counted in input samples
    -- then random lengths below 3,000; random full-scale samples, and tracks of +-32767 in every channel that follow the signs of
    one output's taps, so that the largest int32 sum and both clamps occur."""
    half = 12 * down // up
    lengths = [0, 1, 2, 3, down // up + 2, half - 1, half, half + 1, 2 * half + 1]
    for T in tiles:
        one = -(-T * down // up)  # the first length with more than T outputs is around here
        lengths += [one - 2, one - 1, one, one + 1, one + 2, 2 * one - 1, 2 * one + 2]
    lengths += [int(v) for v in rng.integers(1, 3000, max(count - len(lengths) - 4, 4))]
    tracks = [rng.integers(-32768, 32768, (max(n, 0), C), dtype=np.int16) for n in lengths]
    h = np.asarray(taps).astype(np.int64)
    c = 12 * down
    for m, flip in ((40, 1), (97, -1), (3, 1), (0, -1)):  # the last two: the window reaches in front of the track's first sample
        x = rng.integers(-32768, 32768, (140 * down // up + 50, C), dtype=np.int16)
        t = m * down + c
        p, b = t % up, t // up
        k = np.arange(p, len(h), up)          # the output's taps, against x[b], x[b - 1], ...
        n = b - np.arange(len(k))
        keep = (n >= 0) & (n < len(x))
        x[n[keep]] = (32767 * flip * np.where(h[k[keep]] < 0, -1, 1))[:, None]
        tracks.append(x)
    return tracks


def lay_out(pkg, rng, tracks, C, up, down, planar):
    """The input buffer -- garbage everywhere, every track at a multiple of 8 samples with garbage behind its final length -- the
    spans, and the size of the output buffer: tracks at multiples of 64 with room between them that must stay guard."""
    spans = np.zeros(len(tracks), dtype=pkg.RESAMPLE_SPAN_DTYPE)
    at_in = at_out = 0
    for i, x in enumerate(tracks):
        out_len = -(-len(x) * up // down)
        plane = (out_len + 63) // 64 * 64 + 64 * int(rng.integers(0, 3))
        spans[i] = (at_in, len(x), at_out, plane, 0, 0)
        at_in = (at_in + len(x) + int(rng.integers(0, 40)) + 7) // 8 * 8
        at_out += plane if planar else (out_len + 63) // 64 * 64 + 64 * int(rng.integers(0, 2))
    n = len(tracks)
    scale = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    scale[0] = 2.0 ** -15
    assert np.isfinite(scale).all() and (scale != 0).all()
    spans["scale"] = scale
    buf = rng.integers(-32768, 32768, (at_in + 64, C), dtype=np.int16)
    for sp, x in zip(spans, tracks):
        buf[sp["in_offset"]:sp["in_offset"] + len(x)] = x
    return buf, spans, at_out + 64


def expected(refs, spans, total, CO, format):
    want = np.full(total * CO, GUARD16 if format == "s16" else GUARD32, dtype=np.uint16 if format == "s16" else np.uint32)
    for sp, y in zip(spans, refs):
        v = as_format(y, sp["scale"], format)
        if format == "f32_planar":
            for c in range(CO):
                base = CO * sp["out_offset"] + c * sp["out_plane"]
                want[base:base + len(y)] = raw(v[c])
        else:
            want[CO * sp["out_offset"]:CO * (sp["out_offset"] + len(y))] = raw(v).ravel()
    return want


def run_kernel_case(pkg, ctx, rng, tracks, C, up, down, mono, mix, formats):
    taps = pkg.resample_ratio_taps(up, down)
    M = None if mix is None else pkg.downmix_matrix(C, {"mono": 1, "stereo": 2}[mix])
    CO = 1 if mono else C if M is None else len(M)
    refs = [resample_ratio_ref(x, up, down, taps, mono, M) for x in tracks]  # once, for every format
    assert sum(y.size for y in refs) > 20000
    assert min(int(y.min(initial=0)) for y in refs) == -32768 and max(int(y.max(initial=0)) for y in refs) == 32767  # both clamps occur
    for format in formats:
        buf, spans, total = lay_out(pkg, rng, tracks, C, up, down, format == "f32_planar")
        want = expected(refs, spans, total, CO, format)
        fill = np.full_like(want, GUARD16 if format == "s16" else GUARD32)
        d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
        try:
            ctx.h2d(d_in, buf)
            ctx.h2d(d_out, fill)
            ctx.tracks_resample_ratio_device(spans[:0], d_in, C, up, down, mono, mix, pkg.TRACK_FORMATS[format], d_out)  # no track: nothing
            got = np.zeros_like(want)
            ctx.d2h(got, d_out)
            assert (got == fill).all()
            ctx.tracks_resample_ratio_device(spans, d_in, C, up, down, mono, mix, pkg.TRACK_FORMATS[format], d_out)
            ctx.d2h(got, d_out)
        finally:
            ctx.dev_free(d_in)
            ctx.dev_free(d_out)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (format, len(bad), bad[:8], [hex(v) for v in got[bad[:4]]], [hex(v) for v in want[bad[:4]]],
                               [(i, int(sp["in_samples"])) for i, sp in enumerate(spans) if CO * sp["out_offset"] <= bad[0]][-1:])


KERNEL_CASES = [(up, down, C, mono, mix) for up, down in ((147, 160), (2, 3), (147, 320), (5, 8))
                for C, mono, mix in ((1, False, None), (2, False, None), (2, True, None), (6, False, None), (6, False, "stereo"))]


@pytest.mark.parametrize("up,down,channels,mono,mix", KERNEL_CASES)
def test_kernel_alone(pkg, ctx, up, down, channels, mono, mix):
    """k_tracks_resample_ratio on crafted_tracks in one launch per format: every element of the output buffer equals
    resample_ratio_ref's or is an untouched guard word, whatever lies behind a track's final length in the input."""
    rng = np.random.default_rng(100000 * channels + 100 * down + up + mono)
    tracks = crafted_tracks(rng, channels, up, down, pkg.resample_ratio_taps(up, down))
    run_kernel_case(pkg, ctx, rng, tracks, channels, up, down, mono, mix, FORMATS)


def test_kernel_alone_at_its_widest(pkg, ctx):
    """Eight channels at 1 / 8: a corner where a 256-output tile would take more than 64 KB of LDS and the launch halves it to 128
    outputs -- lengths around one and two of those tiles."""
    rng = np.random.default_rng(18)
    tracks = crafted_tracks(rng, 8, 1, 8, pkg.resample_ratio_taps(1, 8), tiles=(128, 256), count=40)
    run_kernel_case(pkg, ctx, rng, tracks, 8, 1, 8, False, None, ["f32"])


def test_kernel_refusals(pkg, ctx):
    """With a real context and real buffers: what the call refuses changes nothing in the output buffer."""
    spans = np.zeros(1, dtype=pkg.RESAMPLE_SPAN_DTYPE)
    spans[0] = (0, 100, 0, 128, 1.0, 0)
    buf = np.zeros((128, 2), dtype=np.int16)
    fill = np.full(1024, GUARD32, dtype=np.uint32)
    d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(d_in, buf)
        ctx.h2d(d_out, fill)
        for channels, up, down, mono, mix, fmt in ((2, 3, 2, 0, None, 0), (2, 1, 9, 0, None, 1), (3, 2, 3, 1, None, 1), (2, 2, 3, 0, None, 3),
                                                   (9, 2, 3, 0, None, 0), (2, 2, 3, 1, [[8192, 8192]], 0)):
            with pytest.raises((pkg.OpusGpuError, ValueError)):
                ctx.tracks_resample_ratio_device(spans, d_in, channels, up, down, mono, mix, fmt, d_out)
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_resample_ratio_device(spans, d_in.value + 2, 2, 2, 3, 0, None, 0, d_out)  # d_in not 16-byte aligned
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_resample_ratio_device(spans, d_in, 2, 2, 3, 0, None, 0, d_out.value + 64)  # d_out not 128-byte aligned
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all()
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)


# ---- whole files --------------------------------------------------------------------------------------------
def same_as_resampled_s16(pkg, s16, res, up, down, mono, M, format, scales, planned):
    """res = decode_files(resample=, ...) of the batch whose S16 tracks are s16: lengths, codes, the grid and every sample."""
    (t0, i0), (t1, i1) = s16, res
    for field in i0.dtype.names:  # lengths at 48 kHz, final_status, bad_packet and the plan's fields
        assert np.array_equal(i0[field], i1[field]), field
    assert np.array_equal(i1["out_samples"], -(-i0["track_samples"] * up // down))
    offs, total = pkg.resample_ratio_layout(planned, up, down)
    assert np.array_equal(i1["out_offset"], offs) and (offs % 64 == 0).all()
    taps = pkg.resample_ratio_taps(up, down)
    kept = 0
    for i, (a, b) in enumerate(zip(t0, t1)):
        want = as_format(resample_ratio_ref(a, up, down, taps, mono, M), scales[i], format)
        assert b.dtype == want.dtype and b.shape == want.shape, (i, b.shape, want.shape)
        assert np.array_equal(raw(b), raw(want)), i
        kept += want.size
    return kept


@pytest.mark.parametrize("pipeline", [0, 1])
def test_stereo_files(pkg, ctx, pipeline):
    """decode_files(resample=44100, format="f32_planar", scale="head_gain") and (resample=(2, 3), mono=True) of the corpus and the
    files whose frame fails on the device, in order and pipelined: each bit-equal to the reference applied to the same batch's
    int16 tracks; decoded twice on one object with the same bits."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    scales = [pkg.head_gain_scale(g) for g in b.info["output_gain"]]
    s16 = ctx.decode_files(None, batch=b)
    res = ctx.decode_files(None, batch=b, resample=44100, format="f32_planar", scale="head_gain")
    assert same_as_resampled_s16(pkg, s16, res, 147, 160, False, None, "f32_planar", scales, b.info["track_samples"]) > 100000
    again = ctx.decode_files(None, batch=b, resample=(294, 320), format="f32_planar", scale="head_gain")
    assert np.array_equal(again[1], res[1]) and all(np.array_equal(raw(x), raw(y)) for x, y in zip(again[0], res[0]))
    res = ctx.decode_files(None, batch=b, resample=(2, 3), mono=True)
    assert same_as_resampled_s16(pkg, s16, res, 2, 3, True, None, "s16", [None] * len(files), b.info["track_samples"]) > 50000
    info = res[1]
    assert any(x is not None for x in bad)
    for i, seq in enumerate(bad):
        if seq is not None:  # a failed track ends at its packet and its tail is filtered against zeros
            final = b.packet_start(i, seq)
            assert info["track_samples"][i] == final < b.info["track_samples"][i] and info["out_samples"][i] == -(-final * 2 // 3) == len(res[0][i])
    b.close()


def test_surround_32k_stereo(pkg):
    layout = LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    s16 = ms.decode_files(None, batch=b)
    res = ms.decode_files(None, batch=b, resample=32000, mix="stereo")
    assert all(t.shape[1] == 2 for t in res[0])
    M = pkg.downmix_matrix(6, 2)
    assert same_as_resampled_s16(pkg, s16, res, 2, 3, False, M, "s16", [None] * n, b.info["track_samples"]) > 30000
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, rate=32000)
    b.close()
    ms.close()


def test_resample_none_takes_todays_paths(pkg, ctx):
    """decode_files(..., resample=None) returns what decode_files(...) returns, on the S16 path and on the rate= path."""
    files, _ = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    for kw in ({}, dict(rate=16000, mono=True, format="f32")):
        a, c = ctx.decode_files(None, batch=b, **kw), ctx.decode_files(None, batch=b, resample=None, **kw)
        assert a[1].dtype == c[1].dtype and np.array_equal(a[1], c[1]) and all(np.array_equal(raw(x), raw(y)) for x, y in zip(a[0], c[0]))
        assert sum(t.size for t in a[0]) > 30000
    assert "out_samples" not in ctx.decode_files(None, batch=b, resample=None)[1].dtype.names
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
want, winfo = ctx.decode_files(None, batch=b, resample=44100, mono=True, format="f32")
offs, total = pkg.resample_ratio_layout(b.info["track_samples"], 147, 160)
assert total < int(b.track_samples) * 2  # a tensor of the resampled size is enough
FILL = 12345.5
out = torch.full((total + 256,), FILL, dtype=torch.float32, device="cuda:0")
tracks, info = ctx.decode_files(None, batch=b, resample=44100, mono=True, format="f32", out=out)
assert np.array_equal(info, winfo) and len(tracks) == len(files) and sum(len(w) for w in want) > 15000
untouched = torch.ones(total + 256, dtype=torch.bool)
for t, w, o in zip(tracks, want, offs):
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == w.shape and w.shape[1] == 1
    assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
    assert np.array_equal(t.cpu().numpy().view(np.uint32), w.view(np.uint32))
    untouched[int(o):int(o) + len(w)] = False
host = out.cpu()
assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
for bad in (out[1:], out.to(torch.float64), out[:total - 1], out[::2], out.cpu()):
    try:
        ctx.decode_files(None, batch=b, resample=44100, mono=True, format="f32", out=bad)
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(resample=, mono=, out=tensor): straight into a torch tensor of the RESAMPLED size, the tracks views of it equal
    to the numpy route, every element outside the tracks as it was.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
