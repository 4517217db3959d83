"""The channel mix of the whole-file path on the GPU (include/opusgpu.h CHANNEL MIX: k_tracks_resample_mix,
opusgpu_tracks_resample_mixed_device, opusgpu_files_decode_mixed, opusgpu_ms_files_decode_mixed).  A mixed track is a pure integer
function of the S16 track, so every check is bit for bit against resample_ref(mix_ref(x, M), ...) of tests/test_tracks_mix.py and
tests/test_tracks_resample.py: the kernel alone on crafted tracks in a buffer of guard words, whole files against the S16 tracks
of the same planned batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import GUARD16, GUARD32, as_format, crafted_tracks, lay_out, raw, stereo_files, taps_of
from test_tracks_mix import mix_ref
from test_tracks_resample import resample_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = {24000: 2, 16000: 3, 12000: 4, 8000: 6, 48000: 1}
FORMATS = ["s16", "f32", "f32_planar"]


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def random_matrix(rng, CO, C):
    """Full-range int16 entries, rescaled so that every row's abs-sum is <= 65535 (and close to it where it was above)."""
    M = rng.integers(-32768, 32768, (CO, C)).astype(np.int64)
    for row in M:
        s = np.abs(row).sum()
        if s > 65535:
            row[:] = np.trunc(row * (65535.0 / s))
    assert (np.abs(M).sum(axis=1) <= 65535).all() and np.abs(M).max() > 8000
    return M.astype(np.int16)


def matrix_of(pkg, rng, C, CO):
    if (C, CO) == (2, 1):
        return np.array([[8192, 8192]], dtype=np.int16)
    if (C, CO) == (2, 2):
        return np.array([[0, -16384], [16384, 0]], dtype=np.int16)  # a swap with one negated channel
    if C == 6:
        return pkg.downmix_matrix(6, CO)
    if (C, CO) == (8, 8):
        M = np.zeros((8, 8), dtype=np.int16)
        M[np.arange(8), rng.permutation(8)] = 16384 * rng.choice([-1, 1], 8)
        return M
    return random_matrix(rng, CO, C)


def full_row(rng, C):
    """A random row of abs-sum exactly 65535 (one channel: 32767, the most an int16 holds), signs random."""
    if C == 1:
        return np.array([32767 * rng.choice([-1, 1])], dtype=np.int16)
    w = rng.random(C) + 0.05
    mag = np.minimum(np.floor(65535 * w / w.sum()).astype(np.int64), 32767)
    while mag.sum() < 65535:  # hand the rest to entries that have room
        i = int(np.argmax(np.where(mag < 32767, rng.random(C), -1)))
        mag[i] += min(65535 - mag.sum(), 32767 - mag[i])
    assert mag.sum() == 65535
    return (mag * rng.choice([-1, 1], C)).astype(np.int16)


def clamp_tracks(rng, row, D):
    """Two tracks of +-full scale that follow the signs of `row` and of its negative: the mix clamps at both ends."""
    x = np.where(row < 0, -32768, 32767).astype(np.int16)
    up = np.tile(x, (40 * D + 5, 1))
    up[::7] = rng.integers(-32768, 32768, (len(up[::7]), len(row)), dtype=np.int16)
    return [up, (-1 - up.astype(np.int32)).astype(np.int16)]  # ~x: the other end


KERNEL_CASES = [(C, CO, rate) for C, CO in ((2, 1), (2, 2), (1, 2), (3, 2), (5, 1), (6, 1), (6, 2), (7, 2), (8, 2), (8, 8))
                for rate in ((24000, 16000, 12000, 8000, 48000) if (C, CO) == (6, 2) else (16000, 48000))]


@pytest.mark.parametrize("C,CO,rate", KERNEL_CASES)
def test_kernel_alone(pkg, ctx, C, CO, rate):
    """k_tracks_resample_mix on crafted_tracks in one launch per format: every element of the output buffer equals
    resample_ref(mix_ref(...)) or is an untouched guard word, whatever lies behind a track's final length in the input.  The
    last row of a random matrix has abs-sum 65535, and two tracks of +-full scale follow its signs."""
    D = RATES[rate]
    rng = np.random.default_rng(100000 * C + 1000 * CO + rate // 100)
    taps = taps_of(pkg, rate)
    M = matrix_of(pkg, rng, C, CO)
    hard = (C, CO) in ((1, 2), (3, 2), (5, 1), (7, 2), (8, 2))  # the random matrices: their last row is one of abs-sum 65535
    if hard:
        M[-1] = full_row(rng, C)
        assert np.abs(M[-1].astype(np.int64)).sum() == (65535 if C > 1 else 32767)
    tracks = crafted_tracks(rng, C, D, taps) + clamp_tracks(rng, M[-1], D)
    mixed = [mix_ref(x, M) for x in tracks]
    if hard:
        both = np.concatenate([m[:, -1] for m in mixed[-2:]])
        full = np.concatenate([(x.astype(np.int64) @ M[-1].astype(np.int64) + 8192) >> 14 for x in tracks[-2:]])
        assert full.max() > 32767 and full.min() < -32768 and both.max() == 32767 and both.min() == -32768  # both clamps of the mix
    for format in FORMATS:
        buf, spans, total = lay_out(pkg, rng, tracks, C, CO, D, format == "f32_planar")
        want = np.full(total * CO, GUARD16 if format == "s16" else GUARD32, dtype=np.uint16 if format == "s16" else np.uint32)
        written = 0
        for sp, x in zip(spans, mixed):
            y = resample_ref(x, rate, taps, mono=False) if D > 1 else x
            v = as_format(y, sp["scale"], format)
            if format == "f32_planar":
                for c in range(CO):
                    base = CO * sp["out_offset"] + c * sp["out_plane"]
                    want[base:base + len(y)] = raw(v[c])
            else:
                want[CO * sp["out_offset"]:CO * (sp["out_offset"] + len(y))] = raw(v).ravel()
            written += y.size
        assert written > 20000
        fill = np.full_like(want, GUARD16 if format == "s16" else GUARD32)
        d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
        try:
            ctx.h2d(d_in, buf)
            ctx.h2d(d_out, fill)
            ctx.tracks_resample_mixed_device(spans[:0], d_in, C, rate, M, pkg.TRACK_FORMATS[format], d_out)  # no track: nothing
            got = np.zeros_like(want)
            ctx.d2h(got, d_out)
            assert (got == fill).all()
            ctx.tracks_resample_mixed_device(spans, d_in, C, rate, M, pkg.TRACK_FORMATS[format], d_out)
            ctx.d2h(got, d_out)
            if (C, CO) == (2, 1):  # the special staging writes the same buffer, bit for bit
                ctx.h2d(d_out, fill)
                ctx.tracks_resample_device(spans, d_in, 2, rate, 1, pkg.TRACK_FORMATS[format], d_out)
                mono = np.zeros_like(want)
                ctx.d2h(mono, d_out)
                assert np.array_equal(mono, got), format
        finally:
            ctx.dev_free(d_in)
            ctx.dev_free(d_out)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (format, len(bad), bad[:8], [hex(v) for v in got[bad[:4]]], [hex(v) for v in want[bad[:4]]],
                               [(i, int(sp["in_samples"])) for i, sp in enumerate(spans) if CO * sp["out_offset"] <= bad[0]][-1:])


def test_kernel_refusals(pkg, ctx):
    """With a real context and real buffers: what the call refuses changes nothing in the output buffer."""
    spans = np.zeros(1, dtype=pkg.RESAMPLE_SPAN_DTYPE)
    spans[0] = (0, 100, 0, 128, 1.0, 0)
    buf = np.zeros((128, 2), dtype=np.int16)
    fill = np.full(2048, GUARD32, dtype=np.uint32)
    ok = np.array([[8192, 8192]], dtype=np.int16)
    over = np.zeros(1, dtype=pkg.MIX_MATRIX_DTYPE)
    over["out_channels"], over["in_channels"] = 1, 2
    over["m"][0, 0, :2] = [-32768, -32768]
    nine = over.copy()
    nine["m"][0, 0, :2] = [8192, 8192]
    nine["out_channels"] = 9
    d_in, d_out = ctx.dev_alloc(buf.nbytes), ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(d_in, buf)
        ctx.h2d(d_out, fill)
        for channels, rate, mix, fmt in ((2, 44100, ok, 0), (2, 16000, ok, 3), (2, 16000, over, 0), (2, 48000, nine, 1), (3, 16000, nine, 0)):
            with pytest.raises(pkg.OpusGpuError):
                ctx.tracks_resample_mixed_device(spans, d_in, channels, rate, mix, fmt, d_out)
        with pytest.raises(ValueError):
            ctx.tracks_resample_mixed_device(spans, d_in, 3, 16000, ok, 0, d_out)  # two columns for three channels
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_resample_mixed_device(spans, d_in.value + 2, 2, 16000, ok, 0, d_out)  # d_in not 16-byte aligned
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_resample_mixed_device(spans, d_in, 2, 48000, ok, 0, d_out.value + 64)  # d_out not 128-byte aligned
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all()
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)


# ---- whole files --------------------------------------------------------------------------------------------
def same_as_mixed_s16(pkg, s16, res, rate, M, format, scales, planned):
    """res = decode_files(rate=, mix=, format=) of the batch whose S16 tracks are s16: lengths, codes, the grid and every sample
    (test_gpu_tracks_resample.py::same_as_resampled_s16 with the mix in front)."""
    (t0, i0), (t1, i1) = s16, res
    D = RATES[rate]
    for field in i0.dtype.names:
        assert np.array_equal(i0[field], i1[field]), field
    assert i1.dtype.names == i0.dtype.names + ("out_samples", "out_offset")
    assert np.array_equal(i1["out_samples"], -(-i0["track_samples"] // D))
    offs, total = pkg.resample_layout(planned, rate)
    assert np.array_equal(i1["out_offset"], offs) and (offs % 64 == 0).all()
    taps = taps_of(pkg, rate)
    kept = 0
    for i, (a, b) in enumerate(zip(t0, t1)):
        x = mix_ref(a, M)
        want = as_format(resample_ref(x, rate, taps, mono=False) if D > 1 else x, scales[i], format)
        assert b.dtype == want.dtype and b.shape == want.shape, (i, b.shape, want.shape)
        assert np.array_equal(raw(b), raw(want)), i
        kept += want.size
    return kept


@pytest.mark.parametrize("name,seed", [("5.1", 51), ("7.1", 71)])
def test_surround_16k_mono_and_stereo(pkg, name, seed):
    """The 5.1 corpus of test_gpu_tracks_resample.py::test_surround_16k and a 7.1 one through the default tables; decoded twice on
    one object."""
    layout = LAYOUTS[name]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(seed), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    assert (b.info["status"] == 0).all()
    s16 = ms.decode_files(None, batch=b)
    assert len(s16[1].dtype.names) == len(pkg.FILE_INFO_DTYPE.names) + 2  # mix=None: today's info, no field more
    unit = [2.0 ** -15] * n
    mono = ms.decode_files(None, batch=b, rate=16000, mix="mono")
    assert all(t.shape[1] == 1 and t.dtype == np.int16 for t in mono[0])
    kept = same_as_mixed_s16(pkg, s16, mono, 16000, pkg.downmix_matrix(b.channels, 1), "s16", unit, b.info["track_samples"])
    stereo = ms.decode_files(None, batch=b, rate=16000, mix="stereo", format="f32_planar")
    assert all(t.shape[0] == 2 and t.dtype == np.float32 for t in stereo[0])
    kept += same_as_mixed_s16(pkg, s16, stereo, 16000, pkg.downmix_matrix(b.channels, 2), "f32_planar", unit, b.info["track_samples"])
    assert kept > 30000
    again = ms.decode_files(None, batch=b, rate=16000, mix="mono")
    assert np.array_equal(again[1], mono[1]) and all(np.array_equal(x, y) for x, y in zip(again[0], mono[0]))
    with pytest.raises(ValueError):
        ms.decode_files(None, batch=b, rate=16000, mix=np.eye(2))
    b.close()
    ms.close()


def test_stereo_files_mix_mono_is_mono(pkg, ctx):
    """decode_files(rate=16000, mix="mono") of the stereo corpus and the files whose frame fails on the device equals
    decode_files(rate=16000, mono=True) array for array; failed tracks end at ceil(final / 3).  Left only at 24 kHz; mix=None is
    today's call."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    s16 = ctx.decode_files(None, batch=b)
    assert "out_samples" not in s16[1].dtype.names and len(s16[1].dtype.names) == len(pkg.FILE_INFO_DTYPE.names) + 2
    none = ctx.decode_files(None, batch=b, mix=None)
    assert none[1].dtype == s16[1].dtype and np.array_equal(none[1], s16[1]) and all(np.array_equal(x, y) for x, y in zip(none[0], s16[0]))
    want = ctx.decode_files(None, batch=b, rate=16000, mono=True)
    res = ctx.decode_files(None, batch=b, rate=16000, mix="mono")
    assert res[1].dtype == want[1].dtype and np.array_equal(res[1], want[1])
    assert all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(res[0], want[0]))
    assert sum(t.size for t in res[0]) > 30000
    assert any(x is not None for x in bad)
    for i, seq in enumerate(bad):
        if seq is not None:
            final = b.packet_start(i, seq)
            assert (res[1]["final_status"][i], res[1]["bad_packet"][i]) == (-18, seq)
            assert res[1]["track_samples"][i] == final < b.info["track_samples"][i] and res[1]["out_samples"][i] == -(-final // 3) == len(res[0][i])
    again = ctx.decode_files(None, batch=b, rate=16000, mix="mono")
    assert np.array_equal(again[1], res[1]) and all(np.array_equal(x, y) for x, y in zip(again[0], res[0]))
    left = ctx.decode_files(None, batch=b, rate=24000, mix=[[1.0, 0.0]], format="f32")
    M = np.array([[16384, 0]], dtype=np.int16)
    assert same_as_mixed_s16(pkg, s16, left, 24000, M, "f32", [2.0 ** -15] * len(files), b.info["track_samples"]) > 30000
    swap = ctx.decode_files(None, batch=b, mix=np.array([[0, 16384], [16384, 0]]))  # 48000: the mix alone
    assert same_as_mixed_s16(pkg, s16, swap, 48000, np.array([[0, 16384], [16384, 0]], dtype=np.int16), "s16", [None] * len(files),
                             b.info["track_samples"]) > 100000
    with pytest.raises(ValueError):
        ctx.decode_files(None, batch=b, rate=16000, mix="mono", mono=True)
    b.close()


OUT_SCRIPT = r"""
import importlib.util, os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "tests"))
spec = importlib.util.spec_from_file_location("esp32_opus_player_amd", os.path.join(root, "esp32-opus-player_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pkg)
import ms_files_util as mf
from ms_util import LAYOUTS
import torch
layout = LAYOUTS["5.1"]
n = 6
corpus = mf.corpus(pkg, np.random.default_rng(23), layout, n, 5)
ms = pkg.MultistreamContext(0, n, *layout)
b = pkg.MsFileBatch([c[0] for c in corpus], layout)
want, winfo = ms.decode_files(None, batch=b, rate=16000, mix="stereo", format="f32")
offs, total = pkg.resample_layout(b.info["track_samples"], 16000)
assert total * 2 * 3 < int(b.track_samples) * 6  # a tensor of the MIXED size is enough: two channels at a third of the rate
FILL = 12345.5
out = torch.full((2 * total + 256,), FILL, dtype=torch.float32, device="cuda:0")
tracks, info = ms.decode_files(None, batch=b, rate=16000, mix="stereo", format="f32", out=out)
assert np.array_equal(info, winfo) and len(tracks) == n and sum(w.size for w in want) > 15000
untouched = torch.ones(2 * total + 256, dtype=torch.bool)
for t, w, o in zip(tracks, want, offs):
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == w.shape and w.shape[1] == 2
    assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
    assert np.array_equal(t.cpu().numpy().view(np.uint32), w.view(np.uint32))
    untouched[2 * int(o):2 * (int(o) + len(w))] = False
host = out.cpu()
assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
for bad in (out[1:], out.to(torch.float64), out[:2 * total - 1], out[::2], out.cpu()):
    try:
        ms.decode_files(None, batch=b, rate=16000, mix="stereo", format="f32", out=bad)
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
b.close()
ms.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(rate=, mix=, out=tensor): straight into a torch tensor of the MIXED size, the tracks views of it equal to the
    numpy route, every element outside the tracks as it was.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor_mix.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
