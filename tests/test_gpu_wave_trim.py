"""Wave trim on the GPU (include/opusgpu.h WAVE TRIM: k_wave_trim_energy, k_wave_trim_fold, opusgpu_tracks_wave_trim_device, and the
whole-file resampling calls under opusgpu_set_wave_trim).  The stage alone on crafted int16 tracks whose padding holds other
samples: every field of every record and every flag byte equal to wave_trim_ref of tests/test_wave_trim.py -- the definition is
integers throughout --, nothing written outside.  Through the files: the dense result against wave_trim_ref and then wave_batch_ref
applied to the int16 result of the same call without the wave keywords."""
import os
import re

import numpy as np
import pytest

import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import stereo_files
from test_gpu_wave_batch import lay_tracks
from test_wave_batch import ZMUV, stats_held, wave_batch_ref
from test_wave_trim import ABS, frame_energies, records_held, wave_trim_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A
GUARD = 64
SOURCE = open(os.path.join(ROOT, "esp32-opus-player_amd", "csrc", "og_wave_trim.hpp")).read()
TILE = int(re.search(r"constexpr int WTRIM_TILE = (\d+);", SOURCE).group(1))  # elements a tile's frames advance over, at most


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def abs_spec(pkg, threshold, fl, hop, margin=0, flags=True):
    """A trim_spec() record in ABS mode with the threshold given as the integer it is."""
    rec = pkg.trim_spec(0.0, fl, hop, ref=0.0, margin=margin, flags=flags)
    rec["threshold"] = threshold
    return rec


def run_trim(pkg, ctx, d_s16, spans, C, req):
    """The stand-alone call into canary bytes -> (records, list of flag arrays or None); every byte around them is still canary."""
    n = len(spans)
    frames = pkg.wave_trim_frames(spans["samples"], int(req["hop"][0]))
    want_flags = int(req["flags"][0]) == 1
    rec_bytes = n * pkg.WAVE_TRIM_STAT_DTYPE.itemsize
    recs = np.full(rec_bytes + 2 * GUARD, CANARY, dtype=np.uint8)
    flags = np.full(int(frames.sum()) + 2 * GUARD, CANARY, dtype=np.uint8)
    rc = ctx.lib.opusgpu_tracks_wave_trim_device(ctx.h, n, spans.ctypes.data, C, req.ctypes.data, d_s16, recs[GUARD:].ctypes.data,
                                                 flags[GUARD:].ctypes.data, None)
    assert rc == 0, ctx.lib.opusgpu_last_error(ctx.h)
    assert (recs[:GUARD] == CANARY).all() and (recs[GUARD + rec_bytes:] == CANARY).all()
    assert (flags[:GUARD] == CANARY).all() and (flags[len(flags) - GUARD:] == CANARY).all()
    body = flags[GUARD:len(flags) - GUARD]
    if not want_flags:
        assert (body == CANARY).all()
    stats = recs[GUARD:GUARD + rec_bytes].copy().view(pkg.WAVE_TRIM_STAT_DTYPE)
    return stats, (np.split(body.copy(), np.cumsum(frames)[:-1]) if want_flags else None)


def trim_held(pkg, ctx, rng, tracks, C, req):
    """One call of the stage over `tracks`, laid out among loud samples, against the reference -> (records, flags)."""
    buf, spans = lay_tracks(pkg, rng, tracks, C, [np.float32(1.0)] * len(tracks))
    d_s16 = ctx.dev_alloc(buf.nbytes)
    try:
        ctx.h2d(d_s16, buf)
        stats, flags = run_trim(pkg, ctx, d_s16, spans, C, req)
    finally:
        ctx.dev_free(d_s16)
    want, want_flags = wave_trim_ref(tracks, C, req)
    records_held(stats, want)
    if flags is not None:
        assert len(flags) == len(want_flags) and all(np.array_equal(g, w) for g, w in zip(flags, want_flags))
    return stats, flags


def patchy(rng, L, C):
    """L samples of quiet and loud stretches of 24 samples."""
    amp = np.repeat(rng.choice([0, 2, 30, 1500, 32767], size=L // 24 + 1), 24)[:L]
    return (rng.uniform(-1, 1, (L, C)) * amp[:, None]).round().astype(np.int16)


@pytest.mark.parametrize("fl,hop", [(16, 8), (48, 16), (400, 160), (2048, 512)])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_stage_alone(pkg, ctx, C, fl, hop):
    """G = hop (16 / 8), G < hop (48 / 16: G 8; 400 / 160: G 40, five octets a granule) and fl / G = 2 (16 / 8); the lengths 0, 1,
    hop - 1, hop, hop + 1, fl / 2, fl and one of more than two tiles plus 1; REL with flags, ABS without: records and flags equal
    the reference, canaries untouched, a second call (other source offsets) the same bits, and a track alone the record it has among
    the others."""
    rng = np.random.default_rng(1000 * C + fl)
    lengths = [0, 1, hop - 1, hop, hop + 1, fl // 2, fl, 2 * (TILE // C) + hop + 1]
    tracks = [patchy(rng, L, C) for L in lengths]
    for req in (pkg.trim_spec(25.0, fl, hop, flags=True), pkg.trim_spec(30.0, fl, hop, ref=-20.0, margin=8), pkg.trim_spec(25.0, fl, hop)):
        stats, flags = trim_held(pkg, ctx, rng, tracks, C, req)
        again, flags2 = trim_held(pkg, ctx, rng, tracks, C, req)
        assert stats.tobytes() == again.tobytes() and (flags is None or all(np.array_equal(a, b) for a, b in zip(flags, flags2)))
        t = len(tracks) - 1
        alone, flags1 = trim_held(pkg, ctx, rng, tracks[t:], C, req)
        assert alone[0].tobytes() == stats[t].tobytes() and (flags is None or np.array_equal(flags1[0], flags[t]))
    assert 0 < int(stats[t]["count"]) and int(stats[t]["frames"]) == 1 + lengths[t] // hop


def test_one_sample_at_every_place(pkg, ctx):
    """A single non-zero sample at every position p of the first three hops, one track each, threshold 0: exactly the frames whose
    span holds p are active."""
    fl, hop, L = 48, 16, 5 * 16 + 3
    rng = np.random.default_rng(3)
    tracks = []
    for p in range(3 * hop):
        y = np.zeros((L, 1), dtype=np.int16)
        y[p] = -7
        tracks.append(y)
    stats, flags = trim_held(pkg, ctx, rng, tracks, 1, abs_spec(pkg, 0, fl, hop))
    for p, got in enumerate(flags):
        want = [1 if f * hop - fl // 2 <= p < f * hop + fl // 2 else 0 for f in range(1 + L // hop)]
        assert got.tolist() == want and int(stats[p]["emax"]) == 49, p


def test_the_widest_sums(pkg, ctx):
    """-32768 in every sample at fl = 8192: a full frame's energy is 2^43.  REL at 60 dB keeps the track, REL with ratio 1 and ABS at
    Emax nothing, ABS at Emax - 1 the full frames; two channels as well."""
    fl, hop = 8192, 2048
    rng = np.random.default_rng(4)
    full = fl << 30
    for C in (1, 2):
        L = 3 * fl + 5
        tracks = [np.full((L, C), -32768, dtype=np.int16)]
        stats, _ = trim_held(pkg, ctx, rng, tracks, C, pkg.trim_spec(60.0, fl, hop, flags=True))
        assert (int(stats[0]["emax"]), int(stats[0]["start"]), int(stats[0]["count"])) == (full, 0, L)
        stats, _ = trim_held(pkg, ctx, rng, tracks, C, pkg.trim_spec(0.0, fl, hop, flags=True))
        assert (int(stats[0]["thr"]), int(stats[0]["count"]), int(stats[0]["active"]), int(stats[0]["first"])) == (full, 0, 0, -1)
        stats, _ = trim_held(pkg, ctx, rng, tracks, C, abs_spec(pkg, full, fl, hop))
        assert int(stats[0]["count"]) == 0
        stats, flags = trim_held(pkg, ctx, rng, tracks, C, abs_spec(pkg, full - 1, fl, hop))
        inside = [1 if f * hop - fl // 2 >= 0 and f * hop + fl // 2 <= L else 0 for f in range(1 + L // hop)]
        assert flags[0].tolist() == inside and sum(inside) == int(stats[0]["active"]) > 0


def test_thresholds_are_strict_and_silence_trims_to_nothing(pkg, ctx):
    """ABS at the exact M of a frame: that frame is silent; at M - 1: active.  REL with ratio 1: Emax > thr never holds.  An all-zero
    track in REL mode: nothing (librosa keeps it whole -- the header's one divergence)."""
    fl, hop, C = 400, 160, 2
    rng = np.random.default_rng(5)
    y = patchy(rng, 3000, C)
    M = frame_energies(y, C, fl, hop)
    f = int(np.argsort(M)[len(M) // 2])
    assert M[f] > 0
    _, flags = trim_held(pkg, ctx, rng, [y], C, abs_spec(pkg, M[f], fl, hop))
    assert flags[0][f] == 0
    _, flags = trim_held(pkg, ctx, rng, [y], C, abs_spec(pkg, M[f] - 1, fl, hop))
    assert flags[0][f] == 1
    stats, flags = trim_held(pkg, ctx, rng, [y, np.zeros((777, C), dtype=np.int16)], C, pkg.trim_spec(0.0, fl, hop, flags=True))
    assert [int(v) for v in stats["count"]] == [0, 0] and int(stats[0]["thr"]) == int(stats[0]["emax"]) == max(M) and not flags[0].any()
    stats, _ = trim_held(pkg, ctx, rng, [np.zeros((777, C), dtype=np.int16)], C, pkg.trim_spec(60.0, fl, hop))
    assert (int(stats[0]["count"]), int(stats[0]["emax"]), int(stats[0]["full"]), int(stats[0]["frames"])) == (0, 0, 777, 5)


def test_a_burst_in_noise(pkg, ctx):
    """Low-level noise around a burst, margins 0 and 24 and one larger than the lead-in, which clamps to 0 and L; and two channels
    with the burst in the second only (the maximum over the channels)."""
    fl, hop = 64, 16
    rng = np.random.default_rng(6)
    L, a, b = 1000, 320, 640
    noise = rng.integers(-3, 4, (L, 2)).astype(np.int16)
    mono = noise[:, :1].copy()
    mono[a:b, 0] = rng.integers(-20000, 20001, b - a)
    stereo = noise.copy()
    stereo[a:b, 1] = mono[a:b, 0]
    spans = {}
    for margin in (0, 24, 400):
        stats, _ = trim_held(pkg, ctx, rng, [mono], 1, pkg.trim_spec(40.0, fl, hop, margin=margin))
        spans[margin] = (int(stats[0]["start"]), int(stats[0]["start"] + stats[0]["count"]))
        two, _ = trim_held(pkg, ctx, rng, [stereo, mono.repeat(2, axis=1)], 2, pkg.trim_spec(40.0, fl, hop, margin=margin))
        assert two[0].tobytes() == stats[0].tobytes() and two[1].tobytes() == stats[0].tobytes()
    s0, e0 = spans[0]
    assert a - fl // 2 <= s0 <= a and b <= e0 <= b + fl // 2 + hop
    assert spans[24] == (s0 - 24, e0 + 24) and spans[400] == (0, L)


# ---- through the files --------------------------------------------------------------------------------------
def trimmed_equals(pkg, dense, dinfo, s16, sinfo, C, planar, S, spec, scales, mask=True):
    """A trimmed dense result against wave_trim_ref and then wave_batch_ref applied to the int16 call's own result -> the reference's
    records."""
    n = len(s16)
    tracks = [np.asarray(y).reshape(-1, C) for y in s16]
    want, want_flags = wave_trim_ref(tracks, C, spec)
    records_held(dinfo["wave_trim"], want)
    assert [int(v) for v in dinfo["out_samples"]] == [w["count"] for w in want]
    assert [int(v) for v in dinfo["trim_start"]] == [w["start"] for w in want] and np.array_equal(dinfo["trim_samples"], dinfo["out_samples"])
    assert [w["full"] for w in want] == [int(v) for v in sinfo["out_samples"]]
    for field in sinfo.dtype.names:
        if field not in ("out_offset", "out_samples"):
            assert np.array_equal(sinfo[field], dinfo[field]), field
    assert np.array_equal(dinfo["out_offset"], np.arange(n) * S)
    kept = [y[w["start"]:w["start"] + w["count"]] for y, w in zip(tracks, want)]
    stats = dinfo["wave_stats"]
    stats_held(stats, kept, scales, ZMUV, 1e-7, 1.0)  # (its counts are those of the trimmed tracks)
    ref, ref_mask = wave_batch_ref(kept, C, planar, S, ZMUV, 0.0, scales, stats)
    assert dense.dtype == np.float32 and dense.shape == ref.reshape(dense.shape).shape
    assert np.array_equal(np.ascontiguousarray(dense).reshape(-1).view(np.uint32), ref.reshape(-1).view(np.uint32))
    if mask:
        assert np.array_equal(dinfo["mask"], ref_mask)
    if int(spec["flags"][0]):
        assert all(np.array_equal(g, w) for g, w in zip(dinfo["activity"], want_flags))
        for t, w in enumerate(want):  # the trim span is the hull of the intervals, widened by the margin
            iv = pkg.activity_intervals(dinfo["activity"][t], int(spec["hop"][0]), w["full"])
            assert (len(iv) == 0) == (w["count"] == 0)
    else:
        assert "activity" not in dinfo.dtype.names
    return want


def quantile_spec(pkg, s16, C, q, fl, hop, margin=0, flags=True):
    """ABS at the q-quantile of the reference's own frame energies over all tracks of an int16 result."""
    M = sorted(m for y in s16 for m in frame_energies(np.asarray(y).reshape(-1, C), C, fl, hop))
    return abs_spec(pkg, M[int(q * (len(M) - 1))], fl, hop, margin, flags)


def kinds(want):
    """(tracks cut in front, tracks cut behind, tracks untouched) of the reference's records."""
    front = sum(1 for w in want if w["count"] and w["start"] > 0)
    behind = sum(1 for w in want if w["count"] and w["start"] + w["count"] < w["full"])
    whole = sum(1 for w in want if w["full"] and w["start"] == 0 and w["count"] == w["full"])
    return front, behind, whole


def test_files_16k_mono(pkg, ctx):
    """decode_files(rate=16000, mono=True, format="f32", wave_normalize="zmuv", wave_mask=True, wave_trim=...) of the stereo corpus
    and the files whose frame fails on the device: REL and an ABS threshold at a quantile of the reference's own frame energies.  The
    corpus must show a track cut in front, one cut behind and one untouched.  wave_trim=None in between is the call without the
    keyword; a loudness target moves no trim index, its gain is in the scale."""
    files, bad = stereo_files(2)
    n = len(files)
    ctx.streams_alloc(n, 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    kw = dict(batch=b, rate=16000, mono=True)
    s16, sinfo = ctx.decode_files(None, **kw)
    more = dict(format="f32", wave_normalize="zmuv", wave_mask=True)
    S = pkg.files_request(b, rate=16000, mono=True, **more).wave_batch.stride
    scales = [np.float32(2.0 ** -15)] * n
    plain, pinfo = ctx.decode_files(None, **kw, **more)
    seen = np.zeros(3, dtype=np.int64)
    for spec in (quantile_spec(pkg, s16, 1, 0.35, 400, 160), quantile_spec(pkg, s16, 1, 0.6, 2048, 512, margin=64, flags=False),
                 pkg.trim_spec(20.0, 400, 160)):
        dense, dinfo = ctx.decode_files(None, **kw, **more, wave_trim=spec)
        want = trimmed_equals(pkg, dense, dinfo, s16, sinfo, 1, False, S, spec, scales)
        print("front / behind / whole", kinds(want), [(w["start"], w["count"], w["full"]) for w in want])
        seen += kinds(want)
        between, binfo = ctx.decode_files(None, **kw, **more, wave_trim=None)  # the request is gone
        assert np.array_equal(between.view(np.uint32), plain.view(np.uint32)) and np.array_equal(binfo, pinfo)
    assert (seen > 0).all(), seen
    # a failed file is trimmed inside its final length
    assert any(x is not None for x in bad)
    for i, seq in enumerate(bad):
        if seq is not None:
            assert int(dinfo["wave_trim"]["full"][i]) == -(-b.packet_start(i, seq) // 3) and dinfo["final_status"][i] == -18
    # a loudness target: the same trim records, the gain in the scale
    spec = quantile_spec(pkg, s16, 1, 0.35, 400, 160)
    quiet, qinfo = ctx.decode_files(None, **kw, **more, wave_trim=spec)
    loud, linfo = ctx.decode_files(None, **kw, **more, wave_trim=spec, loudness=-23.0)
    assert (linfo["gain"] != 1.0).any() and np.array_equal(linfo["wave_trim"], qinfo["wave_trim"])
    gained = [np.float32(np.float64(np.float32(2.0 ** -15)) * g) for g in linfo["gain"]]
    tracks = [np.asarray(y).reshape(-1, 1)[int(r["start"]):int(r["start"] + r["count"])] for y, r in zip(s16, linfo["wave_trim"])]
    stats_held(linfo["wave_stats"], tracks, gained, ZMUV, 1e-7, 1.0)
    ref, ref_mask = wave_batch_ref(tracks, 1, False, S, ZMUV, 0.0, gained, linfo["wave_stats"])
    assert np.array_equal(loud.reshape(-1).view(np.uint32), ref.reshape(-1).view(np.uint32)) and np.array_equal(linfo["mask"], ref_mask)
    b.close()


def test_files_cuts(pkg, ctx):
    """A packed batch of cuts at 24 kHz, both channels, trimmed."""
    import files_util as fu
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)]
    cuts = [(0, 0, None), (1, 100, 3000), (2, 960, 6000), (3, 0, 1)]
    ctx.streams_alloc(len(cuts), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
    s16, sinfo = ctx.decode_files(None, batch=b, rate=24000)
    more = dict(format="f32", wave_normalize="zmuv", wave_mask=True)
    S = pkg.files_request(b, rate=24000, **more).wave_batch.stride
    spec = quantile_spec(pkg, s16, 2, 0.4, 48, 16, margin=8)
    dense, dinfo = ctx.decode_files(None, batch=b, rate=24000, wave_trim=spec, **more)
    want = trimmed_equals(pkg, dense, dinfo, s16, sinfo, 2, False, S, spec, [np.float32(2.0 ** -15)] * len(cuts))
    assert np.array_equal(dinfo["cut_start"], b.cut_info["start"]) and want[3]["full"] == 1 and sum(w["count"] for w in want) > 1000
    b.close()


def test_surround_stereo_mix(pkg):
    """A 5.1 MultistreamContext through mix="stereo" at 16 kHz as planes under ZMUV, trimmed; the call without the keywords is what
    it was behind it."""
    layout = LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    scales = [np.float32(2.0 ** -15)] * n
    kw = dict(batch=b, rate=16000, mix="stereo")
    s16, sinfo = ms.decode_files(None, **kw)
    more = dict(format="f32_planar", wave_normalize="zmuv", wave_mask=True)
    S = pkg.files_request(b, True, 0, rate=16000, mix="stereo", **more).wave_batch.stride
    plain, pinfo = ms.decode_files(None, **kw, **more)
    seen = np.zeros(3, dtype=np.int64)
    for spec in (quantile_spec(pkg, s16, 2, 0.35, 400, 160), quantile_spec(pkg, s16, 2, 0.6, 2048, 512, margin=64), pkg.trim_spec(20.0, 400, 160)):
        dense, dinfo = ms.decode_files(None, **kw, **more, wave_trim=spec)
        want = trimmed_equals(pkg, dense, dinfo, s16, sinfo, 2, True, S, spec, scales)
        print("front / behind / whole", kinds(want), [(w["start"], w["count"], w["full"]) for w in want])
        seen += kinds(want)
        between, binfo = ms.decode_files(None, **kw, **more, wave_trim=None)
        assert np.array_equal(between.view(np.uint32), plain.view(np.uint32)) and np.array_equal(binfo, pinfo)
    assert (seen > 0).all(), seen
    again, ainfo = ms.decode_files(None, **kw)  # the requests are gone
    assert np.array_equal(ainfo, sinfo) and all(np.array_equal(x, y) for x, y in zip(again, s16))
    b.close()
    ms.close()


def test_refusals_through_the_c_abi(pkg, ctx):
    """opusgpu_files_decode_resampled with a trim request whose wave batch was cleared: OPUSGPU_BAD_ARG with the reason, the buffer
    and the arrays as they were; with both on, out_lengths are the trimmed counts and the records are kept; with both off the call
    is the packed one."""
    import files_util as fu
    from test_wave_batch import good_request
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
        assert lib.opusgpu_set_wave_batch(ctx.h, good_request(pkg, stride_samples=L, mask=0).ctypes.data) == 0
        assert lib.opusgpu_set_wave_trim(ctx.h, pkg.trim_spec(20.0, 400, 160, flags=True).ctypes.data) == 0
        assert lib.opusgpu_set_wave_batch(ctx.h, None) == 0
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_F32, None, d_out, *tail) == pkg.OPUSGPU_BAD_ARG
        assert b"without a wave-batch request" in lib.opusgpu_last_error(ctx.h)
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == CANARY).all() and all((a == -7).all() for a in arrays)
        assert lib.opusgpu_set_wave_batch(ctx.h, good_request(pkg, stride_samples=L, mask=0).ctypes.data) == 0
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_F32, None, d_out, *tail) == 0
        recs = np.zeros(n + 1, dtype=pkg.WAVE_TRIM_STAT_DTYPE)
        assert lib.opusgpu_last_wave_trim(ctx.h, n + 1, recs.ctypes.data) == n and lib.opusgpu_last_wave_trim(ctx.h, 0, None) == n
        assert np.array_equal(arrays[0], np.arange(n) * L) and np.array_equal(arrays[1], recs["count"][:n])
        assert np.array_equal(recs["full"][:n], -(-arrays[2] // 3)) and (recs[n:].view(np.uint8) == 0).all()
        have = int(recs["frames"][:n].sum())
        flags = np.full(have + 8, CANARY, dtype=np.uint8)
        assert lib.opusgpu_last_wave_trim_flags(ctx.h, have, flags.ctypes.data) == have
        assert (flags[have:] == CANARY).all() and int(flags[:have].sum()) == int(recs["active"][:n].sum())
        ctx.d2h(got, d_out)
        assert (got[4 * n * L:] == CANARY).all()
        assert lib.opusgpu_set_wave_trim(ctx.h, None) == 0 and lib.opusgpu_set_wave_batch(ctx.h, None) == 0
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_F32, None, d_out, *tail) == 0
        assert np.array_equal(arrays[0], offs) and np.array_equal(arrays[1], -(-arrays[2] // 3))
    finally:
        lib.opusgpu_set_wave_trim(ctx.h, None)
        lib.opusgpu_set_wave_batch(ctx.h, None)
        ctx.dev_free(d_out)
        b.close()
