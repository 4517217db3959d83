"""Track rates of the whole-file path on the GPU (include/opusgpu.h TRACK RATES: k_tracks_resample, opusgpu_files_decode_resampled,
opusgpu_ms_files_decode_resampled).  A resampled track is a pure integer function of the S16 track, so every check here is bit for
bit against tests/test_tracks_resample.py::resample_ref -- int64 dot products with the taps opusgpu_resample_taps hands out: the
kernel alone on crafted tracks in a buffer of guard words, whole files against resample_ref of the S16 tracks of the same planned
batch (which tests/test_gpu_files.py and tests/test_gpu_ms_files.py hold against the reader and the oracle)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
import ogg_util
from ms_util import LAYOUTS
from test_tracks_resample import resample_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = {24000: 2, 16000: 3, 12000: 4, 8000: 6, 48000: 1}
FORMATS = ["s16", "f32", "f32_planar"]
GUARD16, GUARD32 = 0x5A5A, 0x5A5A5A5A


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def taps_of(pkg, rate):
    return None if rate == 48000 else pkg.resample_taps(rate)


def as_format(y, scale, format):
    """A resampled int16 track [m, channels] as `format` stores it: (float)y * scale, planar transposed."""
    if format == "s16":
        return y
    f = y.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(f.T) if format == "f32_planar" else f


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.int16 else a.view(np.uint32)


# ---- the kernel alone -------------------------------------------------------------------------------------
def crafted_tracks(rng, C, D, taps):
    """About 200 tracks [in_samples, C]: every length at which the kernel takes another path -- none, one sample, around one output,
    around the filter's half length, around one tile of every tile length the kernel uses (256, 512, 1,024 outputs) and behind two
    tiles -- then random lengths; random full-scale samples, and tracks of +-32767 that follow the signs of the taps around one
    output, so that the largest int32 sum and both clamps occur."""
    lengths = [0, 1, D - 1, D, D + 1, 12 * D - 1, 12 * D, 12 * D + 1]
    for T in (256, 512, 1024):
        lengths += [T * D - 1, T * D, T * D + 1, 2 * T * D + 3]
    lengths += [int(v) for v in rng.integers(1, 3000, 200 - len(lengths) - 4)]
    tracks = [rng.integers(-32768, 32768, (n, C), dtype=np.int16) for n in lengths]
    if taps is not None:
        sign = np.where(np.asarray(taps) < 0, -1, 1).astype(np.int16)
        for m, flip in ((15, 1), (40, -1), (12, 1), (0, -1)):  # the last two: the window reaches the track's first sample / lies in front of it
            x = rng.integers(-32768, 32768, (60 * D, C), dtype=np.int16)
            lo = m * D - 12 * D
            k = np.arange(len(sign))
            keep = lo + k >= 0
            x[lo + k[keep]] = (32767 * flip * sign[keep])[:, None]
            tracks.append(x)
    return tracks


def lay_out(pkg, rng, tracks, C, CO, D, planar):
    """The input buffer -- garbage everywhere, every track at a multiple of 8 samples with garbage behind its final length -- the
    spans, and the size of the output buffer: tracks at multiples of 64 with room between them that must stay guard."""
    spans = np.zeros(len(tracks), dtype=pkg.RESAMPLE_SPAN_DTYPE)
    at_in = at_out = 0
    for i, x in enumerate(tracks):
        out_len = -(-len(x) // D)
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


def expected(tracks, spans, total, CO, rate, taps, mono, format):
    want = np.full(total * CO, GUARD16 if format == "s16" else GUARD32, dtype=np.uint16 if format == "s16" else np.uint32)
    written = 0
    lo = hi = 0
    for sp, x in zip(spans, tracks):
        y = resample_ref(x, rate, taps, mono)
        lo, hi = min(lo, int(y.min(initial=0))), max(hi, int(y.max(initial=0)))
        v = as_format(y, sp["scale"], format)
        if format == "f32_planar":
            for c in range(CO):
                base = CO * sp["out_offset"] + c * sp["out_plane"]
                want[base:base + len(y)] = raw(v[c])
        else:
            want[CO * sp["out_offset"]:CO * (sp["out_offset"] + len(y))] = raw(v).ravel()
        written += y.size
    assert written > 20000
    return want, (lo, hi)


KERNEL_CASES = [(C, mono, rate) for C, mono in ((1, False), (1, True), (2, False), (2, True), (6, False)) for rate in RATES
                if rate != 48000 or mono]


@pytest.mark.parametrize("channels,mono,rate", KERNEL_CASES)
def test_kernel_alone(pkg, ctx, channels, mono, rate):
    """k_tracks_resample on crafted_tracks in one launch per format: every element of the output buffer equals resample_ref's or
    is an untouched guard word, whatever lies behind a track's final length in the input."""
    C, D = channels, RATES[rate]
    CO = 1 if mono else C
    rng = np.random.default_rng(1000 * C + rate // 100 + mono)
    taps = taps_of(pkg, rate)
    tracks = crafted_tracks(rng, C, D, taps)
    for format in FORMATS:
        buf, spans, total = lay_out(pkg, rng, tracks, C, CO, D, format == "f32_planar")
        want, clamps = expected(tracks, spans, total, CO, rate, taps, mono, format)
        if D > 1:
            assert clamps == (-32768, 32767)  # both clamps occur
        fill = np.full_like(want, GUARD16 if format == "s16" else GUARD32)
        d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
        try:
            ctx.h2d(d_in, buf)
            ctx.h2d(d_out, fill)
            ctx.tracks_resample_device(spans[:0], d_in, C, rate, mono, pkg.TRACK_FORMATS[format], d_out)  # no track: nothing
            got = np.zeros_like(want)
            ctx.d2h(got, d_out)
            assert (got == fill).all()
            ctx.tracks_resample_device(spans, d_in, C, rate, mono, pkg.TRACK_FORMATS[format], d_out)
            ctx.d2h(got, d_out)
        finally:
            ctx.dev_free(d_in)
            ctx.dev_free(d_out)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (format, len(bad), bad[:8], [hex(v) for v in got[bad[:4]]], [hex(v) for v in want[bad[:4]]],
                               [(i, int(sp["in_samples"])) for i, sp in enumerate(spans) if CO * sp["out_offset"] <= bad[0]][-1:])


def test_kernel_refusals(pkg, ctx):
    """With a real context and real buffers: what the call refuses changes nothing in the output buffer."""
    spans = np.zeros(1, dtype=pkg.RESAMPLE_SPAN_DTYPE)
    spans[0] = (0, 100, 0, 64, 1.0, 0)
    buf = np.zeros((128, 2), dtype=np.int16)
    fill = np.full(1024, GUARD32, dtype=np.uint32)
    d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(d_in, buf)
        ctx.h2d(d_out, fill)
        for channels, rate, mono, fmt in ((2, 44100, 0, 0), (2, 48000, 0, 1), (3, 16000, 1, 1), (2, 16000, 0, 3), (9, 16000, 0, 0)):
            with pytest.raises(pkg.OpusGpuError):
                ctx.tracks_resample_device(spans, d_in, channels, rate, mono, fmt, d_out)
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_resample_device(spans, d_in.value + 2, 2, 16000, 0, 0, d_out)  # d_in not 16-byte aligned
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_resample_device(spans, d_in, 2, 16000, 0, 0, d_out.value + 64)  # d_out not 128-byte aligned
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all()
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)


# ---- whole files --------------------------------------------------------------------------------------------
def same_as_resampled_s16(pkg, s16, res, rate, mono, format, scales, planned):
    """res = decode_files(rate=, mono=, format=) of the batch whose S16 tracks are s16: lengths, codes, the grid and every sample."""
    (t0, i0), (t1, i1) = s16, res
    D = RATES[rate]
    for field in i0.dtype.names:  # lengths at 48 kHz, final_status, bad_packet and the plan's fields
        assert np.array_equal(i0[field], i1[field]), field
    assert np.array_equal(i1["out_samples"], -(-i0["track_samples"] // D))
    offs, total = pkg.resample_layout(planned, rate)
    assert np.array_equal(i1["out_offset"], offs) and (offs % 64 == 0).all()
    taps = taps_of(pkg, rate)
    kept = 0
    for i, (a, b) in enumerate(zip(t0, t1)):
        want = as_format(resample_ref(a, rate, taps, mono), scales[i], format)
        assert b.dtype == want.dtype and b.shape == want.shape, (i, b.shape, want.shape)
        assert np.array_equal(raw(b), raw(want)), i
        kept += want.size
    return kept


def stereo_files(channels):
    files = [c[1] for c in fu.corpus20(channels, channel_switches=False)] + [f[1] for f in fu.failing_files(channels)]
    bad = [None] * (len(files) - 5) + [f[2] for f in fu.failing_files(channels)]
    return files, bad


@pytest.mark.parametrize("channels,pipeline", [(2, 0), (2, 1), (1, 0)])
def test_files_16k_mono(pkg, ctx, channels, pipeline):
    """decode_files(rate=16000, mono=True) of the corpus, its mono twin and the files whose frame fails on the device: a failed
    track is ceil(final / 3) samples and its tail is filtered against zeros, whatever earlier frames of the failing packet left
    behind its final length.  Once with the pipeline on; decoded twice on one object."""
    files, bad = stereo_files(channels)
    ctx.streams_alloc(len(files), channels)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch(files, channels=channels, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    s16 = ctx.decode_files(None, batch=b)
    res = ctx.decode_files(None, batch=b, rate=16000, mono=True)
    kept = same_as_resampled_s16(pkg, s16, res, 16000, True, "s16", [None] * len(files), b.info["track_samples"])
    assert kept > 30000
    info = res[1]
    assert any(x is not None for x in bad)
    for i, seq in enumerate(bad):
        if seq is not None:
            final = b.packet_start(i, seq)
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, seq)
            assert info["track_samples"][i] == final < b.info["track_samples"][i] and info["out_samples"][i] == -(-final // 3) == len(res[0][i])
    again = ctx.decode_files(None, batch=b, rate=16000, mono=True)
    assert np.array_equal(again[1], res[1]) and all(np.array_equal(x, y) for x, y in zip(again[0], res[0]))
    b.close()


def test_files_24k_planar_head_gain(pkg, ctx):
    rng = np.random.default_rng(8)
    gains = [256, -1541]
    gain_files = [fu.opus_file([[fu.packet(rng, 0xFC, 120) for _ in range(3)] for _ in range(2)], 2, 312, serial=60 + i, end_trim=57,
                               head=ogg_util.opus_head(channels=2, pre_skip=312, gain=g))[0] for i, g in enumerate(gains)]
    files = stereo_files(2)[0] + gain_files
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    assert list(b.info["output_gain"][-2:]) == gains
    scales = [pkg.head_gain_scale(g) for g in b.info["output_gain"]]
    s16 = ctx.decode_files(None, batch=b)
    res = ctx.decode_files(None, batch=b, rate=24000, format="f32_planar", scale="head_gain")
    assert same_as_resampled_s16(pkg, s16, res, 24000, False, "f32_planar", scales, b.info["track_samples"]) > 100000
    res = ctx.decode_files(None, batch=b, rate=48000, mono=True, format="f32")  # the downmix alone
    assert same_as_resampled_s16(pkg, s16, res, 48000, True, "f32", [2.0 ** -15] * len(files), b.info["track_samples"]) > 100000
    b.close()


@pytest.mark.parametrize("format", ["s16", "f32"])
def test_surround_16k(pkg, format):
    layout = LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    s16 = ms.decode_files(None, batch=b)
    res = ms.decode_files(None, batch=b, rate=16000, format=format)
    assert all(t.shape[1] == 6 for t in res[0])
    assert same_as_resampled_s16(pkg, s16, res, 16000, False, format, [2.0 ** -15] * n, b.info["track_samples"]) > 50000
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, rate=44100)
    b.close()
    ms.close()


def test_default_arguments_take_todays_path(pkg, ctx):
    """decode_files(...) without rate or mono returns what opusgpu_files_decode writes for the same batch, and the info it always
    returned: no field more."""
    files, _ = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    tracks, info = ctx.decode_files(None, batch=b)
    assert "out_samples" not in info.dtype.names and len(info.dtype.names) == len(pkg.FILE_INFO_DTYPE.names) + 2
    total = int(b.track_samples) * 2
    packed = np.zeros(total, dtype=np.int16)
    lengths = np.zeros(len(files), dtype=np.int64)
    status = np.zeros((len(files), 2), dtype=np.int32)
    d = ctx.dev_alloc(packed.nbytes)
    try:
        ctx.set_mode(False)
        ctx._chk(ctx.lib.opusgpu_files_decode(ctx.h, b.h, d, lengths.ctypes.data, status.ctypes.data), "opusgpu_files_decode")
        ctx.d2h(packed, d)
    finally:
        ctx.dev_free(d)
    assert np.array_equal(info["track_samples"], lengths) and np.array_equal(info["final_status"], status[:, 0])
    assert sum(len(t) for t in tracks) > 100000
    for t, o, ln in zip(tracks, b.info["track_offset"], lengths):
        assert t.dtype == np.int16 and np.array_equal(t, packed[2 * o:2 * (o + ln)].reshape(ln, 2))
    same = ctx.decode_files(None, batch=b, rate=48000, mono=False)
    assert np.array_equal(same[1], info) and all(np.array_equal(x, y) for x, y in zip(same[0], tracks))
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
want, winfo = ctx.decode_files(None, batch=b, rate=16000, mono=True, format="f32")
offs, total = pkg.resample_layout(b.info["track_samples"], 16000)
assert total * 3 < int(b.track_samples) * 2  # a tensor of the resampled size is enough
FILL = 12345.5
out = torch.full((total + 256,), FILL, dtype=torch.float32, device="cuda:0")
tracks, info = ctx.decode_files(None, batch=b, rate=16000, mono=True, format="f32", out=out)
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
        ctx.decode_files(None, batch=b, rate=16000, mono=True, format="f32", out=bad)
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(rate=, mono=, out=tensor): straight into a torch tensor of the RESAMPLED size, the tracks views of it equal to
    the numpy route, every element outside the tracks as it was.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
