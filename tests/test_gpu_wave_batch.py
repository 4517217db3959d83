"""Wave batches on the GPU (include/opusgpu.h WAVE BATCHES: k_wave_stats, k_wave_fold, k_wave_batch,
opusgpu_tracks_wave_batch_device, and the whole-file resampling calls under opusgpu_set_wave_batch).  The stage alone on crafted
int16 tracks whose padding holds other samples, into a buffer of canary words: every element of the tensor and the mask bit for bit
against wave_batch_ref of tests/test_wave_batch.py, the records' integers exactly and their sub and mul within BOUND of the
definition, nothing written outside.  Through the files: the dense result against the reference applied to the int16 call's own
result."""
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import stereo_files
from test_wave_batch import NONE, PEAK, ZMUV, good_request, stats_held, wave_batch_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A
GUARD = 256  # bytes of canary at either end: the tensor stays 128-byte aligned
NORM_KW = {NONE: None, ZMUV: "zmuv", PEAK: ("peak", 0.75)}


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def lay_tracks(pkg, rng, tracks, C, scales):
    """Interleaved int16 tracks on different multiples of 8 samples, other samples between them -> (int16 buffer, WAVE_SPAN_DTYPE
    spans)."""
    spans = np.zeros(len(tracks), dtype=pkg.WAVE_SPAN_DTYPE)
    at = 8 * int(rng.integers(0, 3))
    for t, y in enumerate(tracks):
        spans[t] = (at, len(y), scales[t], 0)
        at = (at + len(y) + 7) // 8 * 8 + 8 * int(rng.integers(0, 4))
    buf = rng.integers(-32768, 32768, (at + 8) * C, dtype=np.int64).astype(np.int16)
    for sp, y in zip(spans, tracks):
        o = int(sp["in_offset"]) * C
        buf[o:o + y.size] = y.reshape(-1)
    return buf, spans


def run_stage(pkg, ctx, d_s16, spans, C, format, wb):
    """The stage into canary bytes -> (the tensor's words, flat; the mask [n, S] or None; the records).  Every byte outside the
    tensor and the mask is still canary."""
    n, S = len(spans), wb.stride
    floats, mask_at = pkg.wave_batch_layout(n, C, S, wb.mask)
    fill = np.full(4 * floats + 2 * GUARD, CANARY, dtype=np.uint8)
    d_out = ctx.dev_alloc(fill.nbytes)
    try:
        ctx.h2d(d_out, fill)
        stats = ctx.tracks_wave_batch_device(spans, C, format, wb, d_s16, d_out.value + GUARD)
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
    finally:
        ctx.dev_free(d_out)
    body = got[GUARD:len(got) - GUARD]
    tensor = body[:4 * n * S * C]
    written = np.zeros(len(got), dtype=bool)
    written[GUARD:GUARD + tensor.size] = True
    mask = None
    if wb.mask:
        assert mask_at % 128 == 0 and 0 <= mask_at - tensor.size < 128
        mask = body[mask_at:mask_at + n * S].reshape(n, S)
        written[GUARD + mask_at:GUARD + mask_at + n * S] = True
    assert (got[~written] == CANARY).all()  # in front of and behind both the tensor and the mask
    return tensor.view(np.uint32), mask, stats


def request_of(pkg, lengths, C, S, norm, eps=1e-7, target=0.75, pad=0.0, mask=True):
    kw = {NONE: None, ZMUV: ("zmuv", eps), PEAK: ("peak", target)}[norm]
    return pkg.wave_batch_request(lengths, C, S, kw, pad, mask)


def stage_held(pkg, ctx, rng, tracks, C, S, scales, norm, format, eps=1e-7, target=0.75, pad=-0.25):
    """One call of the stage over `tracks` against the reference -> (words, records)."""
    buf, spans = lay_tracks(pkg, rng, tracks, C, scales)
    wb = request_of(pkg, [len(y) for y in tracks], C, S, norm, eps, target, pad)
    d_s16 = ctx.dev_alloc(buf.nbytes)
    try:
        ctx.h2d(d_s16, buf)
        words, mask, stats = run_stage(pkg, ctx, d_s16, spans, C, format, wb)
    finally:
        ctx.dev_free(d_s16)
    stats_held(stats, tracks, scales, norm, eps, target)
    want, want_mask = wave_batch_ref(tracks, C, format == "f32_planar", S, norm, pad, scales, stats)
    assert np.array_equal(words, want.reshape(-1).view(np.uint32)), (C, S, norm, format)
    assert np.array_equal(mask, want_mask)
    return words, stats


@pytest.mark.parametrize("format", ["f32", "f32_planar"])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_stage_alone(pkg, ctx, C, format):
    """S in {1, 5, 1003}, the lengths {0, 1, 7, 8, 9, S} that fit, as many tracks as make n * S * C no multiple of 4 -- so tracks begin
    at every place of a 16-byte piece and the tensor ends inside one --, sources on different multiples of 8, three norms: the
    tensor, the mask and the records against the reference, canaries untouched, a second call the same bits, and a track alone the
    record and the cells it has among the others."""
    rng = np.random.default_rng(100 * C + len(format))
    for S in (1, 5, 1003):
        base = [L for L in (0, 1, 7, 8, 9) if L < S] + [S]
        lengths = list(base)
        while len(lengths) * S * C % 4 == 0 or len(lengths) < 3:
            lengths.append(base[len(lengths) % len(base)])
        assert len(lengths) * S * C % 4
        tracks = [rng.integers(-32768, 32768, (L, C), dtype=np.int64).astype(np.int16) for L in lengths]
        scales = [np.float32(v) for v in rng.uniform(0.5, 2.0, len(tracks)) * 2.0 ** -15]
        for norm in (NONE, ZMUV, PEAK):
            words, stats = stage_held(pkg, ctx, rng, tracks, C, S, scales, norm, format)
            again, stats2 = stage_held(pkg, ctx, rng, tracks, C, S, scales, norm, format)  # (other source offsets)
            assert np.array_equal(words, again) and np.array_equal(stats, stats2)
            t = len(tracks) - 1
            alone, stat1 = stage_held(pkg, ctx, rng, tracks[t:], C, S, scales[t:], norm, format)
            assert np.array_equal(alone, words.reshape(len(tracks), -1)[t]) and np.array_equal(stat1[0], stats[t])


def test_directed_tracks(pkg, ctx):
    """What the sums must survive: all -32768 over more than three chunks of k_wave_stats plus one sample (a pair squares to 2^31),
    all 32767, alternating extremes, a constant (exactly 0.0f in every real cell under ZMUV), and 30000 everywhere but one 30001 at
    scale 1 and eps 1e-12, where V = N - 1 and a double variance is off by orders of magnitude.  One and two channels."""
    rng = np.random.default_rng(9)
    chunk = 16384
    alt = np.tile(np.array([-32768, 32767], dtype=np.int16), 2049)[:4097]
    near = np.full(5000, 30000, dtype=np.int16)
    near[1667] = 30001
    flat = [np.full(3 * chunk + 1, -32768, dtype=np.int16), np.full(20000, 32767, dtype=np.int16), alt, np.full(1000, 1234, dtype=np.int16),
            near, np.zeros(64, dtype=np.int16)]
    for C in (1, 2):
        tracks = [y[:len(y) // C * C].reshape(-1, C) for y in flat]
        S = max(len(y) for y in tracks) + 3
        scales = [np.float32(1.0)] * len(tracks)
        for norm in (ZMUV, PEAK):
            for format in ("f32", "f32_planar")[:C]:
                words, stats = stage_held(pkg, ctx, rng, tracks, C, S, scales, norm, format, eps=1e-12, target=1.0, pad=0.0)
                cells = words.reshape(len(tracks), -1)
                assert int(stats[0]["sumsq"]) == tracks[0].size << 30 and int(stats[0]["peak"]) == 32768
                if norm == ZMUV:
                    assert (cells[3] == 0).all() and (cells[5] == 0).all()  # the constant tracks: +0.0 in every cell, real or pad
                    N = tracks[4].size
                    assert N * int(stats[4]["sumsq"]) - int(stats[4]["sum"]) ** 2 == N - 1
                else:
                    assert np.abs(cells[0].view(np.float32)).max() == 1.0 and float(stats[5]["mul"]) == 1.0


def test_stage_refusals(pkg, ctx):
    """What the stand-alone call refuses, with NULL buffers: nothing reaches the device."""
    lib = ctx.lib
    spans = np.zeros(2, dtype=pkg.WAVE_SPAN_DTYPE)
    spans["in_offset"], spans["samples"], spans["scale"] = [0, 16], [10, 5], 1.0
    rec = good_request(pkg, stride_samples=10)

    def call(s, ch=1, fmt=pkg.TRACKS_F32, r=rec, h=ctx.h):
        return lib.opusgpu_tracks_wave_batch_device(h, len(s), s.ctypes.data, ch, fmt, r.ctypes.data, None, None, None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    BAD = pkg.OPUSGPU_BAD_ARG
    assert call(spans, h=None) == BAD and call(spans) == BAD and b"NULL" in lib.opusgpu_last_error(ctx.h)  # in order but for the buffers
    for s in (but(in_offset=4), but(in_offset=-8), but(samples=-1), but(samples=11), but(scale=np.nan), but(scale=np.inf), but(reserved=1)):
        assert call(s) == BAD
    assert b"below the samples" in (call(but(samples=11)) and lib.opusgpu_last_error(ctx.h))
    for kw in (dict(ch=0), dict(ch=9), dict(fmt=pkg.TRACKS_S16), dict(fmt=3), dict(r=good_request(pkg, stride_samples=10, norm=7)),
               dict(r=good_request(pkg, stride_samples=10, eps=0.0)), dict(r=good_request(pkg, stride_samples=0x7fffffff), ch=2)):
        assert call(spans, **kw) == BAD, kw
    assert call(spans[:0]) == 0  # nothing to do is no error


# ---- through the files --------------------------------------------------------------------------------------
def dense_equals(pkg, dense, dinfo, s16, sinfo, C, planar, wb, scales, norm, eps=1e-7, target=0.75, pad=0.0):
    """A dense result against the reference applied to the int16 call's own result; info as that call's but for out_offset and the
    new fields."""
    n, S = len(s16), wb.stride
    for field in sinfo.dtype.names:
        if field != "out_offset":
            assert np.array_equal(sinfo[field], dinfo[field]), field
    if "out_offset" in dinfo.dtype.names:
        assert np.array_equal(dinfo["out_offset"], np.arange(n) * S)
    assert dense.dtype == np.float32 and dense.shape == ((n, C, S) if planar else (n, S, C) if C > 1 else (n, S))
    tracks = [np.asarray(y).reshape(-1, C) for y in s16]
    stats = dinfo["wave_stats"]
    stats_held(stats, tracks, scales, norm, eps, target)
    want, want_mask = wave_batch_ref(tracks, C, planar, S, norm, pad, scales, stats)
    assert np.array_equal(np.ascontiguousarray(dense).reshape(-1).view(np.uint32), want.reshape(-1).view(np.uint32))
    if wb.mask:
        assert np.array_equal(dinfo["mask"], want_mask)
    else:
        assert "mask" not in dinfo.dtype.names
    return sum(y.size for y in tracks)


def test_files_16k_mono(pkg, ctx):
    """decode_files(rate=16000, mono=True, format="f32", wave_*) of the stereo corpus and the files whose frame fails on the device,
    each norm: the reference of the int16 call's result, bit for bit; a failed file pads from its final length; two runs give the
    same bits; NONE equals the packed float call cell for cell, also under a loudness target; the packed call is what it was
    behind it (the request is cleared); a track decoded alone has the record it has in the batch."""
    files, bad = stereo_files(2)
    n = len(files)
    ctx.streams_alloc(n, 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    kw = dict(batch=b, rate=16000, mono=True)
    s16, sinfo = ctx.decode_files(None, **kw)
    packed, pinfo = ctx.decode_files(None, format="f32", **kw)
    S = int((-(-b.info["track_samples"] // 3)).max()) + 3
    scales = [np.float32(2.0 ** -15)] * n
    for norm in (NONE, ZMUV, PEAK):
        more = dict(format="f32", wave_stride=S, wave_normalize=NORM_KW[norm], wave_mask=True)
        wb = pkg.files_request(b, rate=16000, mono=True, **more).wave_batch
        dense, dinfo = ctx.decode_files(None, **kw, **more)
        assert dense_equals(pkg, dense, dinfo, s16, sinfo, 1, False, wb, scales, norm) > 30000
        again, ainfo = ctx.decode_files(None, **kw, **more)
        assert np.array_equal(again.view(np.uint32), dense.view(np.uint32)) and np.array_equal(ainfo, dinfo)
        if norm == NONE:
            for t, y in enumerate(packed):
                assert np.array_equal(dense[t, :len(y)].view(np.uint32), y[:, 0].view(np.uint32)) and (dense[t, len(y):] == 0).all()
    assert any(x is not None for x in bad)
    for i, seq in enumerate(bad):
        if seq is not None:
            L = int(dinfo["out_samples"][i])
            assert L == -(-b.packet_start(i, seq) // 3) < -(-b.info["track_samples"][i] // 3) and dinfo["final_status"][i] == -18
            assert (dense[i, L:] == 0).all() and int(dinfo["mask"][i].sum()) == L
    after, afinfo = ctx.decode_files(None, format="f32", **kw)  # the request is gone
    assert np.array_equal(afinfo, pinfo) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(after, packed))
    # NONE under a loudness target: the packed float call's cells; ZMUV: the gain is in the scale
    loud, linfo = ctx.decode_files(None, format="f32", loudness=-23.0, **kw)
    dense, dinfo = ctx.decode_files(None, format="f32", loudness=-23.0, wave_stride=S, **kw)
    assert (dinfo["gain"] != 1.0).any() and np.array_equal(dinfo["gain"], linfo["gain"])
    for t, y in enumerate(loud):
        assert np.array_equal(dense[t, :len(y)].view(np.uint32), y[:, 0].view(np.uint32)) and (dense[t, len(y):] == 0).all()
    gained = [np.float32(np.float64(np.float32(2.0 ** -15)) * g) for g in linfo["gain"]]
    dense, dinfo = ctx.decode_files(None, format="f32", loudness=-23.0, wave_normalize="zmuv", **kw)
    wb = pkg.files_request(b, rate=16000, mono=True, format="f32", loudness=-23.0, wave_normalize="zmuv").wave_batch
    assert wb.stride == S - 3
    dense_equals(pkg, dense, dinfo, s16, sinfo, 1, False, wb, gained, ZMUV)
    b.close()
    # a track decoded alone: the record it has in the batch
    t = 3
    b1 = pkg.FileBatch(files[t:t + 1], channels=2, flags=pkg.PAGES_GROUP_BY_MODE)
    one, oinfo = ctx.decode_files(None, batch=b1, rate=16000, mono=True, format="f32", wave_normalize=NORM_KW[PEAK], wave_mask=True)
    b1.close()
    more = dict(format="f32", wave_stride=S, wave_normalize=NORM_KW[PEAK], wave_mask=True)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    dense, dinfo = ctx.decode_files(None, batch=b, rate=16000, mono=True, **more)
    b.close()
    L = int(oinfo["out_samples"][0])
    assert np.array_equal(oinfo["wave_stats"][0], dinfo["wave_stats"][t]) and np.array_equal(one[0, :L].view(np.uint32), dense[t, :L].view(np.uint32))


def test_files_44k_planar_and_48k_and_cuts(pkg, ctx):
    """resample=44100 as planar stereo; 48 kHz with neither mix nor mono (the identity mix) against the plain int16 tracks; a packed
    batch of cuts at 24 kHz."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)]
    n = len(files)
    ctx.streams_alloc(n, 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    scales = [np.float32(2.0 ** -15)] * n
    s16, sinfo = ctx.decode_files(None, batch=b, resample=44100)
    more = dict(format="f32_planar", wave_normalize="zmuv", wave_mask=True)
    wb = pkg.files_request(b, resample=44100, **more).wave_batch
    dense, dinfo = ctx.decode_files(None, batch=b, resample=44100, **more)
    assert dense_equals(pkg, dense, dinfo, s16, sinfo, 2, True, wb, scales, ZMUV) > 100000
    # 48 kHz: the tracks themselves
    s16, sinfo = ctx.decode_files(None, batch=b)
    S = int(b.info["track_samples"].max()) + 1
    more = dict(format="f32", wave_stride=S, wave_normalize=("peak", 0.75), wave_pad=-1.0)
    wb = pkg.files_request(b, **more).wave_batch
    dense, dinfo = ctx.decode_files(None, batch=b, **more)
    assert np.array_equal(dinfo["out_samples"], sinfo["track_samples"])
    assert dense_equals(pkg, dense, dinfo, s16, sinfo, 2, False, wb, scales, PEAK, pad=-1.0) > 100000
    b.close()
    cuts = [(0, 0, None), (1, 100, 3000), (2, 960, 6000), (3, 0, 1)]
    ctx.streams_alloc(len(cuts), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
    s16, sinfo = ctx.decode_files(None, batch=b, rate=24000)
    more = dict(format="f32", wave_normalize="zmuv", wave_mask=True)
    wb = pkg.files_request(b, rate=24000, **more).wave_batch
    dense, dinfo = ctx.decode_files(None, batch=b, rate=24000, **more)
    assert dense_equals(pkg, dense, dinfo, s16, sinfo, 2, False, wb, scales[:len(cuts)], ZMUV) > 2000
    assert np.array_equal(dinfo["cut_start"], b.cut_info["start"]) and int(dinfo["out_samples"][3]) == 1
    b.close()


def test_surround_stereo_mix(pkg):
    """A 5.1 MultistreamContext through mix="stereo" at 16 kHz under ZMUV, and all six channels at 48 kHz as planes under PEAK."""
    layout = LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    scales = [np.float32(2.0 ** -15)] * n
    s16, sinfo = ms.decode_files(None, batch=b, rate=16000, mix="stereo")
    more = dict(format="f32", wave_normalize="zmuv", wave_mask=True)
    wb = pkg.files_request(b, True, 0, rate=16000, mix="stereo", **more).wave_batch
    dense, dinfo = ms.decode_files(None, batch=b, rate=16000, mix="stereo", **more)
    assert dense_equals(pkg, dense, dinfo, s16, sinfo, 2, False, wb, scales, ZMUV) > 20000
    s16, sinfo = ms.decode_files(None, batch=b)
    more = dict(format="f32_planar", wave_normalize=("peak", 0.75))
    wb = pkg.files_request(b, True, 0, **more).wave_batch
    dense, dinfo = ms.decode_files(None, batch=b, **more)
    assert dense_equals(pkg, dense, dinfo, s16, sinfo, 6, True, wb, scales, PEAK) > 100000
    again, ainfo = ms.decode_files(None, batch=b)  # the request is gone
    assert np.array_equal(ainfo, sinfo) and all(np.array_equal(x, y) for x, y in zip(again, s16))
    b.close()
    ms.close()


def test_refusals_through_the_c_abi(pkg, ctx):
    """opusgpu_files_decode_resampled under a request whose stride is too small, and with int16 tracks: OPUSGPU_BAD_ARG, the buffer
    and the arrays as they were; a stride that fits works and reports t * S; with the request off the call is the packed one."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2)
    n = b.n_files
    lib = ctx.lib
    L = int((-(-b.info["track_samples"] // 3)).max())
    offs, total = pkg.resample_layout(b.info["track_samples"], 16000)
    fill = np.full(4 * max(total, n * L) + 256, CANARY, dtype=np.uint8)
    d_out = ctx.dev_alloc(fill.nbytes)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]
    tail = [a.ctypes.data for a in arrays]
    try:
        ctx.h2d(d_out, fill)
        assert lib.opusgpu_set_wave_batch(ctx.h, good_request(pkg, stride_samples=L - 1, mask=0).ctypes.data) == 0
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_F32, None, d_out, *tail) == pkg.OPUSGPU_BAD_ARG
        assert b"stride_samples is below" in lib.opusgpu_last_error(ctx.h)
        assert lib.opusgpu_set_wave_batch(ctx.h, good_request(pkg, stride_samples=L, mask=0).ctypes.data) == 0
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_S16, None, d_out, *tail) == pkg.OPUSGPU_BAD_ARG
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == CANARY).all() and all((a == -7).all() for a in arrays)
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_F32, None, d_out, *tail) == 0
        assert np.array_equal(arrays[0], np.arange(n) * L)
        ctx.d2h(got, d_out)
        assert (got[4 * n * L:] == CANARY).all()
        assert lib.opusgpu_set_wave_batch(ctx.h, None) == 0
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_F32, None, d_out, *tail) == 0
        assert np.array_equal(arrays[0], offs)
    finally:
        lib.opusgpu_set_wave_batch(ctx.h, None)
        ctx.dev_free(d_out)
        b.close()


def test_other_calls_ignore_the_request(pkg, ctx):
    """Under a request that no call of this batch could keep (S = 1), opusgpu_files_decode, opusgpu_files_decode_as and a feature call
    return what they return without it: they never read it."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2)
    calls = (dict(), dict(format="f32_planar"), dict(features="logmel", mono=True))
    want = [ctx.decode_files(None, batch=b, **kw) for kw in calls]
    assert ctx.lib.opusgpu_set_wave_batch(ctx.h, good_request(pkg, stride_samples=1).ctypes.data) == 0
    try:
        for kw, (tracks, info) in zip(calls, want):
            got, ginfo = ctx.decode_files(None, batch=b, **kw)
            assert np.array_equal(ginfo, info) and all(np.array_equal(x, y) for x, y in zip(got, tracks)), kw
        with pytest.raises(pkg.OpusGpuError):
            ctx.decode_files(None, batch=b, rate=16000, format="f32")  # (the request is on: this one reads it)
    finally:
        ctx.lib.opusgpu_set_wave_batch(ctx.h, None)
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
n = len(files)
ctx = pkg.Context(0)
ctx.streams_alloc(n, 2)
b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE)
S = int((-(-b.info["track_samples"] // 3)).max()) + 7
kw = dict(batch=b, rate=16000, format="f32", wave_stride=S, wave_normalize="zmuv", wave_mask=True)
want, winfo = ctx.decode_files(None, **kw)
assert want.shape == (n, S, 2)
floats, mask_at = pkg.wave_batch_layout(n, 2, S, True)
FILL = 12345.5
out = torch.full((floats + 256,), FILL, dtype=torch.float32, device="cuda:0")
got, info = ctx.decode_files(None, out=out, **kw)
assert np.array_equal(info, winfo) and info["mask"].sum() == info["out_samples"].sum()
assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, S, 2)
assert got.untyped_storage().data_ptr() == out.untyped_storage().data_ptr() and got.data_ptr() == out.data_ptr()  # a view of `out`
assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
mask = out.view(torch.uint8)[mask_at:mask_at + n * S].cpu().numpy().reshape(n, S)
assert np.array_equal(mask, winfo["mask"])
assert bool((out[floats:] == FILL).all())
before = out.clone()
for bad in (out[1:], out[:floats - 1], out.to(torch.float64), out.cpu()):
    try:
        ctx.decode_files(None, out=bad, **kw)
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
assert bool((out == before).all())
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(rate=16000, format="f32", wave_stride=S, wave_normalize="zmuv", wave_mask=True, out=tensor): the result is a view
    of the tensor of shape [n, S, 2], equal to the numpy route, the mask behind it, the elements behind that as they were; a tensor
    that does not fit raises before any device work.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
