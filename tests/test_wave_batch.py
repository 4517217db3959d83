"""Wave batches of the whole-file path (include/opusgpu.h, WAVE BATCHES), what needs no GPU: the exported symbols and the records,
every refusal of opusgpu_set_wave_batch, the layout call, the whole-file refusals that come before device work, what files_request
makes of wave_stride= / wave_normalize= / wave_pad= / wave_mask=, the kernels' resources, and the reference that
tests/test_gpu_wave_batch.py holds the kernels to.

wave_stat_def is the header's definition with Python integers for V and exact rationals up to the one square root; wave_batch_ref
the output as a function of the int16 tracks and a record's sub and mul, which the kernels must equal bit for bit.

THE BOUND on sub and mul (BOUND = 2^-48, relative) is the header's: at most eight double roundings of 2^-53 in the implementation,
as many in the evaluation of the definition, doubled.  wave_stat_def itself rounds three times (the variance, the root, the
reciprocal)."""
import ctypes as C
import fractions
import math
import os
import re

import numpy as np
import pytest

from test_files_request import TABLE, keywords
from test_feat_batch import same_request
from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_set_wave_batch", "opusgpu_ms_set_wave_batch", "opusgpu_last_wave_stats", "opusgpu_ms_last_wave_stats",
       "opusgpu_wave_batch_layout", "opusgpu_tracks_wave_batch_device"]
BOUND = 2.0 ** -48
NONE, ZMUV, PEAK = 0, 1, 2


# ---- the reference ------------------------------------------------------------------------------------------
def wave_stat_def(y, scale, norm, eps=1e-7, target=1.0):
    """The definition for one track: y its int16 samples of all channels, any shape -> a dict of count, sum, sumsq, peak (Python
    integers) and sub, mul (floats).  NONE measures nothing."""
    y = [int(v) for v in np.asarray(y).reshape(-1)]
    N, k = len(y), fractions.Fraction(float(np.float32(scale)))
    if norm == NONE:
        return dict(count=N, sum=0, sumsq=0, peak=0, sub=0.0, mul=1.0)
    s, q, peak = sum(y), sum(v * v for v in y), max((abs(v) for v in y), default=0)
    if norm == ZMUV:
        V = N * q - s * s
        sub = float(k * s / N) if N else 0.0
        var = k * k * V / (N * N) if N else fractions.Fraction(0)
        mul = 1.0 / math.sqrt(float(var + fractions.Fraction(float(eps))))
    else:
        d = peak * k
        sub, mul = 0.0, (float(fractions.Fraction(float(target)) / d) if d else 1.0)
    return dict(count=N, sum=s, sumsq=q, peak=peak, sub=sub, mul=mul)


def wave_batch_ref(tracks, C, planar, S, norm, pad, scales, stats):
    """WAVE BATCHES as a function of the int16 tracks (tracks[t] int16 [L[t], C]) and the records' sub and mul (stats: anything
    indexable by t and then by "sub" / "mul") -> (float32 [n, S, C] or [n, C, S], uint8 mask [n, S])."""
    n = len(tracks)
    out = np.full((n, S, C), np.float32(pad), dtype=np.float32)
    mask = np.zeros((n, S), dtype=np.uint8)
    for t, y in enumerate(tracks):
        y = np.asarray(y, dtype=np.int16).reshape(-1, C)
        L = len(y)
        k = np.float32(scales[t])
        if norm == NONE:
            out[t, :L] = y.astype(np.float32) * k
        else:  # y * k is exact in double; the subtraction, the multiplication and the conversion round once each
            out[t, :L] = ((y.astype(np.float64) * np.float64(k) - np.float64(stats[t]["sub"])) * np.float64(stats[t]["mul"])).astype(np.float32)
        mask[t, :L] = 1
    return (np.ascontiguousarray(out.transpose(0, 2, 1)) if planar else out), mask


def stats_held(got, tracks, scales, norm, eps, target):
    """The records of a call against the definition: the integers exactly, sub and mul within BOUND."""
    for t, y in enumerate(tracks):
        want = wave_stat_def(y, scales[t], norm, eps, target)
        for f in ("count", "sum", "sumsq", "peak"):
            assert int(got[t][f]) == want[f], (t, f, int(got[t][f]), want[f])
        for f in ("sub", "mul"):
            g, w = float(got[t][f]), want[f]
            assert g == w or abs(g - w) <= BOUND * abs(w), (t, f, g, w)
        assert int(got[t]["reserved"]) == 0


def test_the_reference_on_a_constant_track():
    """A constant track: V = 0, sub = k c exactly, every real cell exactly +0.0 -- for scales whose product with N c is not a
    double."""
    for c, L, scale in ((1234, 1000, 2.0 ** -15), (-7, 3, 0.1), (32767, 4999, 1.0 / 3), (-32768, 17, 1.2345e-5)):
        y = np.full((L, 1), c, dtype=np.int16)
        st = wave_stat_def(y, scale, ZMUV)
        assert st["sub"] == float(np.float32(scale)) * c and st["mul"] == 1.0 / math.sqrt(1e-7)
        out, mask = wave_batch_ref([y], 1, False, L + 2, ZMUV, 0.5, [scale], [st])
        assert (out[0, :L].view(np.uint32) == 0).all() and (out[0, L:] == 0.5).all() and list(mask[0]) == [1] * L + [0, 0]


def test_the_reference_where_a_double_variance_fails():
    """30000 everywhere but one 30001, scale 1, eps 1e-12: V = N - 1 exactly.  sumsq / N - mean^2 in double, the form FEATURE BATCHES
    uses for its float features, misses BOUND by many orders of magnitude here: the record needs the integer form."""
    N = 5000
    y = np.full(N, 30000, dtype=np.int16)
    y[N // 3] = 30001
    st = wave_stat_def(y, 1.0, ZMUV, 1e-12)
    assert N * st["sumsq"] - st["sum"] ** 2 == N - 1
    assert abs(st["mul"] - 1 / math.sqrt((N - 1) / N ** 2 + 1e-12)) <= 4 * 2.0 ** -53 * st["mul"]
    x = y.astype(np.float64)
    mean = x.sum() / N
    naive = 1 / math.sqrt((x * x).sum() / N - mean * mean + 1e-12)
    print("naive relative error", abs(naive - st["mul"]) / st["mul"], "bound", BOUND)
    assert abs(naive - st["mul"]) > 1e6 * BOUND * st["mul"]


# ---- ABI and refusals ---------------------------------------------------------------------------------------
def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    assert all(s in pkg.EXPORTS for s in NEW)
    assert (pkg.WAVE_BATCH_REQ_DTYPE.itemsize, pkg.WAVE_SPAN_DTYPE.itemsize, pkg.WAVE_STAT_DTYPE.itemsize) == (64, 24, 48)
    assert [pkg.WAVE_STAT_DTYPE.fields[f][1] for f in ("count", "sum", "sumsq", "sub", "mul", "peak", "reserved")] == [0, 8, 16, 24, 32, 40, 44]
    header = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    assert "WAVE BATCHES." in header and all(re.search(r"\b%s\(" % s, header) for s in NEW)
    assert header.index("FEATURE BATCHES.") < header.index("WAVE BATCHES.")
    for name, v in pkg.WAVE_NORMS.items():
        if name is not None:
            assert re.search(r"#define OPUSGPU_WAVE_NORM_%s %d\b" % (name.upper(), v), header)


def good_request(pkg, **kw):
    rec = pkg.wave_batch_request([10], 1, 16000, "zmuv", wave_mask=True).rec.copy()
    for k, v in kw.items():
        rec[k] = v
    return rec


def test_set_time_refusals(pkg, handles):
    lib = pkg.load_lib()
    assert lib.opusgpu_set_wave_batch(None, None) == pkg.OPUSGPU_BAD_ARG and lib.opusgpu_ms_set_wave_batch(None, None) == pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_last_wave_stats(None, 0, None) == pkg.OPUSGPU_BAD_ARG and lib.opusgpu_ms_last_wave_stats(None, 0, None) == pkg.OPUSGPU_BAD_ARG
    for fn, h in zip((lib.opusgpu_set_wave_batch, lib.opusgpu_ms_set_wave_batch), handles):
        for kw in (dict(norm=3), dict(norm=-1), dict(pad_value=np.nan), dict(pad_value=np.inf), dict(eps=np.nan), dict(eps=np.inf),
                   dict(target=np.nan), dict(target=-np.inf), dict(eps=0.0), dict(eps=-1e-7), dict(norm=PEAK, target=0.0),
                   dict(norm=PEAK, target=-1.0), dict(stride_samples=0), dict(stride_samples=-3), dict(mask=2),
                   dict(reserved=[0, 0, 0, 0, 0, 1]), dict(reserved=[1, 0, 0, 0, 0, 0])):
            assert fn(h, good_request(pkg, **kw).ctypes.data) == pkg.OPUSGPU_BAD_ARG, kw
        # what a norm does not read only has to be finite
        for kw in (dict(), dict(norm=PEAK, eps=0.0), dict(norm=ZMUV, target=0.0), dict(norm=NONE, eps=-1.0, target=-1.0), dict(mask=0)):
            assert fn(h, good_request(pkg, **kw).ctypes.data) == 0, kw
        assert fn(h, good_request(pkg, enabled=0, norm=99).ctypes.data) == 0  # off: nothing of it is read
        assert fn(h, None) == 0


def test_layout(pkg):
    lib = pkg.load_lib()
    at = C.c_int64(-1)
    assert lib.opusgpu_wave_batch_layout(5, 2, 1003, 0, C.byref(at)) == 5 * 2 * 1003 and at.value == -1
    assert lib.opusgpu_wave_batch_layout(5, 2, 1003, 0, None) == 10030 and lib.opusgpu_wave_batch_layout(0, 1, 1, 0, None) == 0
    # the mask lies behind the tensor on the next 128-byte boundary, and the total covers it
    for n, ch, S in ((5, 2, 1003), (3, 1, 5), (7, 3, 1), (4, 1, 32), (1, 8, 16000), (0, 1, 7)):
        tensor = 4 * n * ch * S
        total = lib.opusgpu_wave_batch_layout(n, ch, S, 1, C.byref(at))
        assert at.value == (tensor + 127) // 128 * 128 and at.value - tensor < 128
        assert total == (at.value + n * S + 3) // 4 and lib.opusgpu_wave_batch_layout(n, ch, S, 1, None) == total
        assert pkg.wave_batch_layout(n, ch, S, True) == (total, at.value) and pkg.wave_batch_layout(n, ch, S) == (n * ch * S, None)
    for bad in ((-1, 1, 5, 0), (1, 0, 5, 0), (1, 9, 5, 0), (1, 1, 0, 0), (1, 1, -4, 0), (1, 1, 5, 2), (1, 1, 5, -1), (1, 2, 1 << 30, 0),
                (1, 8, 1 << 28, 1)):
        assert lib.opusgpu_wave_batch_layout(*bad, None) == pkg.OPUSGPU_BAD_ARG, bad
    assert lib.opusgpu_wave_batch_layout(3, 8, (1 << 28) - 1, 0, None) == 3 * 8 * ((1 << 28) - 1)
    with pytest.raises(ValueError):
        pkg.wave_batch_layout(1, 2, 1 << 30)


def test_whole_file_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """int16 tracks with a request on, a stride below a planned length and S * C above 0x7fffffff: OPUSGPU_BAD_ARG from the three
    resampling calls of both kinds of decoder with d_out NULL, the arrays untouched, the reason in the decoder's message."""
    lib = pkg.load_lib()
    F32, S16 = pkg.TRACKS_F32, pkg.TRACKS_S16
    for b, prefix, h, mono, ch in ((batch, "opusgpu_", handles[0], (0,), 2), (ms_batch, "opusgpu_ms_", handles[1], (), 6)):
        setter, err = getattr(lib, prefix + "set_wave_batch"), getattr(lib, prefix + "last_error")
        planned = b.info["track_samples"]
        arrays = [np.full(b.n_files, -7, dtype=np.int64) for _ in range(3)] + [np.full((b.n_files, 2), -7, dtype=np.int32)]
        tail = [None] + [a.ctypes.data for a in arrays]
        ident = pkg.mix_matrix(16384 * np.eye(ch, dtype=np.int16), ch)

        # (the call, the most samples of a planned track at its rate)
        calls = ((lambda fmt: getattr(lib, prefix + "files_decode_resampled")(h, b.h, 16000, *mono, fmt, None, *tail), -(-planned // 3)),
                 (lambda fmt: getattr(lib, prefix + "files_decode_mixed")(h, b.h, 48000, ident.ctypes.data, fmt, None, *tail), planned),
                 (lambda fmt: getattr(lib, prefix + "files_decode_ratio")(h, b.h, 147, 160, *mono, None, fmt, None, *tail),
                  -(-planned * 147 // 160)))
        try:
            assert setter(h, good_request(pkg, stride_samples=int(planned.max())).ctypes.data) == 0
            for call, _ in calls:
                assert call(S16) == pkg.OPUSGPU_BAD_ARG and b"the format is int16" in err(h)
            for call, lengths in calls:
                assert lengths.max() > 1
                assert setter(h, good_request(pkg, stride_samples=int(lengths.max()) - 1).ctypes.data) == 0
                assert call(F32) == pkg.OPUSGPU_BAD_ARG and b"stride_samples is below" in err(h)
            assert setter(h, good_request(pkg, stride_samples=0x7fffffff // ch + 1).ctypes.data) == 0
            for call, _ in calls:
                assert call(F32) == pkg.OPUSGPU_BAD_ARG and b"0x7fffffff" in err(h)
        finally:
            assert setter(h, None) == 0
        assert all((a == -7).all() for a in arrays)


# ---- files_request ------------------------------------------------------------------------------------------
def test_the_new_keywords(pkg, batch, ms_batch):
    planned = batch.info["track_samples"]
    n = batch.n_files
    L16 = -(-planned // 3)
    packed = pkg.files_request(batch, rate=16000, mono=True, format="f32")
    req = pkg.files_request(batch, rate=16000, mono=True, format="f32", wave_stride=int(L16.max()) + 5, wave_normalize="zmuv", wave_mask=True)
    wb = req.wave_batch
    S = int(L16.max()) + 5
    assert (req.entry, req.args, req.kind, req.channels, req.fmt) == (packed.entry, packed.args, "resampled", 1, pkg.TRACKS_F32)
    assert packed.wave_batch is None and (wb.channels, wb.stride, wb.mask, wb.n, req.total) == (1, S, True, n, n * S)
    assert np.array_equal(req.offsets, np.arange(n) * S) and (req.planes == S).all()
    assert (wb.floats, wb.mask_offset) == pkg.wave_batch_layout(n, 1, S, True)
    rec = wb.rec
    assert rec.dtype == pkg.WAVE_BATCH_REQ_DTYPE and rec.shape == (1,) and int(rec["enabled"][0]) == 1
    assert (int(rec["norm"][0]), float(rec["eps"][0]), float(rec["pad_value"][0]), int(rec["mask"][0])) == (ZMUV, 1e-7, 0.0, 1)
    assert (rec["reserved"] == 0).all() and int(rec["stride_samples"][0]) == S
    # every keyword alone turns the request dense; S defaults to the longest planned track
    for kw, norm in ((dict(wave_normalize=("zmuv", 1e-5)), ZMUV), (dict(wave_normalize=("peak", 0.5)), PEAK), (dict(wave_pad=-1.5), NONE),
                     (dict(wave_mask=True), NONE), (dict(wave_normalize="none"), NONE), (dict(wave_stride=int(L16.max())), NONE)):
        w = pkg.files_request(batch, rate=16000, mono=True, format="f32_planar", **kw).wave_batch
        assert w.stride == L16.max() and int(w.rec["norm"][0]) == norm and w.mask == bool(kw.get("wave_mask")), kw
    assert float(pkg.files_request(batch, rate=16000, format="f32", wave_normalize=("zmuv", 1e-5)).wave_batch.rec["eps"][0]) == 1e-5
    assert float(pkg.files_request(batch, rate=16000, format="f32", wave_normalize=("peak", 0.5)).wave_batch.rec["target"][0]) == 0.5
    assert float(pkg.files_request(batch, rate=16000, format="f32", wave_pad=-1.5).wave_batch.rec["pad_value"][0]) == -1.5
    # a ratio and a mix: the planned lengths are the call's own
    r = pkg.files_request(batch, resample=44100, format="f32_planar", wave_normalize="zmuv")
    assert (r.entry, r.args[:2], r.channels, r.wave_batch.stride) == ("files_decode_ratio", (147, 160), 2, int((-(-planned * 147 // 160)).max()))
    m = pkg.files_request(batch, mix="mono", rate=24000, format="f32", wave_stride=100000)
    assert (m.entry, m.args[0], m.channels, m.wave_batch.stride) == ("files_decode_mixed", 24000, 1, 100000)
    # 48 kHz with neither mix nor mono: the mixed call with the identity matrix
    for kw in (dict(), dict(rate=48000)):
        u = pkg.files_request(batch, format="f32", wave_mask=True, **kw)
        assert (u.entry, u.args[0], u.channels, u.kind) == ("files_decode_mixed", 48000, 2, "resampled")
        assert np.array_equal(u.mix["m"][0][:2, :2], 16384 * np.eye(2)) and u.wave_batch.stride == planned.max()
    assert pkg.files_request(batch, format="f32").entry == "files_decode_as"
    # the multistream batch, with a loudness target
    ms = pkg.files_request(ms_batch, True, 0, mix="stereo", rate=16000, format="f32", wave_normalize="zmuv", loudness=-23.0)
    assert (ms.entry, ms.channels, ms.total) == ("files_decode_mixed", 2, ms_batch.n_files * ms.wave_batch.stride) and ms.loudness is not None
    u6 = pkg.files_request(ms_batch, True, 0, format="f32_planar", wave_stride=20000)
    assert (u6.entry, u6.channels, u6.wave_batch.channels) == ("files_decode_mixed", 6, 6)
    # out= is held against the buffer's size, the mask included
    ok = Tensor(wb.floats)
    kw = dict(rate=16000, mono=True, format="f32", wave_stride=S, wave_normalize="zmuv", wave_mask=True)
    assert pkg.files_request(batch, out=ok, **kw).out is ok
    with pytest.raises(ValueError):
        pkg.files_request(batch, out=Tensor(wb.floats - 1), **kw)
    assert wb.floats > n * S


def test_value_errors(pkg, batch):
    L16 = int((-(-batch.info["track_samples"] // 3)).max())
    base = dict(rate=16000, mono=True, format="f32")
    for kw in (dict(base, features="logmel", wave_stride=L16), dict(base, features="logmel", wave_mask=True),
               dict(rate=16000, mono=True, wave_stride=L16), dict(rate=16000, mono=True, format="s16", wave_normalize="zmuv"),
               dict(rate=16000, format="s16", wave_mask=True), dict(wave_pad=0.0), dict(base, format="f64", wave_mask=True),
               dict(base, wave_stride=L16 - 1), dict(base, wave_stride=0), dict(base, wave_stride=16000.0), dict(base, wave_stride=True),
               dict(base, wave_stride=1 << 31), dict(base, wave_normalize="cmvn"), dict(base, wave_normalize="peak"),
               dict(base, wave_normalize=("peak", 0.0)), dict(base, wave_normalize=("zmuv", -1e-7)), dict(base, wave_normalize=("zmuv", np.nan)),
               dict(base, wave_normalize=("none", 1.0)), dict(base, wave_normalize=("zmuv", 1e-7, 2)), dict(base, wave_normalize=1),
               dict(base, wave_pad=np.nan), dict(base, wave_pad="zero"), dict(base, wave_mask=1), dict(base, wave_mask="yes")):
        with pytest.raises(ValueError):
            pkg.files_request(batch, **kw)
    assert pkg.files_request(batch, wave_stride=L16, **base).wave_batch.stride == L16
    # the batch's own stride= with the keywords stays refused, with the message it had
    sb = pkg.FileBatch(batch_files(), channels=2, cuts=[(0, 0, 4800), (1, 960, 2880)], stride=4800)
    try:
        with pytest.raises(ValueError) as e:
            pkg.files_request(sb, format="f32", wave_normalize="zmuv")
        assert str(e.value) == pkg.STRIDE_REFUSED
        assert pkg.files_request(sb, format="f32").stride == 4800
    finally:
        sb.close()


def batch_files():
    import files_util as fu
    return [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_requests_without_the_keywords_are_what_they_were(pkg, batch, ms_batch, row):
    kw, *want = TABLE[row]
    for b, multistream, expected in ((batch, False, want[0]), (ms_batch, True, want[1])):
        if expected is None:
            continue
        plain = pkg.files_request(b, multistream, 0, **keywords(pkg, kw))
        named = pkg.files_request(b, multistream, 0, wave_stride=None, wave_normalize=None, wave_pad=None, wave_mask=False, **keywords(pkg, kw))
        same_request(pkg, plain, named)
        assert plain.wave_batch is None and (plain.entry, plain.channels, plain.kind) == (expected[0], expected[2], expected[3])


# ---- kernels ------------------------------------------------------------------------------------------------
def test_kernel_resources():
    """k_wave_stats, k_wave_fold and k_wave_batch once each: no scratch and no LDS at all (the reduction of k_wave_stats is a butterfly
    over the wave and one integer atomic a wave), and registers for 8 waves per SIMD.  No k_tracks_* or k_feat_* name matches them."""
    meta = _kernel_metadata()
    for name in ("k_wave_stats", "k_wave_fold", "k_wave_batch"):
        seen = [v for mangled, v in meta.items() if re.search(r"\d+" + name + r"(P|E|v|$)", mangled)]
        print(name, seen)
        assert len(seen) == 1, (name, sorted(meta)[:6])
        vgpr, scratch, lds = seen[0]
        assert scratch == 0 and lds == 0
        assert vgpr <= 64  # 8 waves per SIMD
    assert not [m for m in meta if re.search(r"k_(tracks|feat)_\w*", m) and "k_wave" in m]
