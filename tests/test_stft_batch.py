"""STFT batches of the whole-file path (include/opusgpu.h, STFT BATCHES), what needs no GPU: the exported symbols and the records,
every refusal of opusgpu_set_stft_batch, the layout call, the whole-file refusals that come before device work, what files_request
makes of stft_stride= / stft_normalize= / stft_pad=, the kernels' resources, and the numpy restatement of the definition that
tests/test_gpu_stft_batch.py holds the GPU to.

stft_batch_ref is the float64 restatement of the header's definition; stft_batch_f32 the plain float32 forms of NONE, WHISPER, REFMAX
and AFFINE, which the kernels must equal bit for bit.  CASES are the synthetic grids the GPU test uploads.

THE BOUND is FEATURE BATCHES' (tests/test_feat_batch.py: bound_of, derived there): 2^-23 |y| + 2^-30 max_f |x[f][k]| / d.  It was
derived for |x| <= 20, per-bin variance >= 0.25 wherever F > 3 and F <= 5000; the cells here are drawn the same way (uniform in
[-16, 16] plus an offset per bin in [-4, 4]) and no track has more than 2049 frames, so it holds as it stands, whatever `bins` is: a
bin's sums do not depend on the other bins."""
import os
import re

import numpy as np
import pytest

from test_feat_batch import bound_of, same_request  # noqa: F401 (bound_of: for the GPU test)
from test_files_request import TABLE, keywords
from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)
from test_tracks_stft import stft_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_set_stft_batch", "opusgpu_ms_set_stft_batch", "opusgpu_stft_batch_layout", "opusgpu_tracks_stft_batch_device"]
REAL_NORMS = ["none", "whisper", "refmax", "cmn", "cmvn", "affine"]
PAIR_NORMS = ["none", "affine"]
VAR_FLOOR = 1e-4
CONSTANT = np.float32(3.7)
# (bins, c) -> the frames of the five tracks of one call: both sides of the 1,024-frame segment boundary, a multi-segment track, the
# 16-byte piece and 64-frame edges, a track without a frame; the last track of a set is the constant one.  1025 bins: F <= 70.
CASES = {(33, 1): [1025, 0, 63, 2049, 1024], (129, 1): [1023, 0, 1, 1025, 65], (257, 1): [1024, 1, 2049, 0, 65],
         (257, 2): [65, 1025, 0, 63, 1023], (1025, 1): [70, 0, 1, 65, 63]}


def strides_of(frames):
    """The largest F, an odd stride (with odd bins track 1 then starts at an element that is no multiple of 4: shared first and last
    pieces) and a multiple of 64."""
    m = max(frames)
    return [m, m + 1 + m % 2, (m + 63) // 64 * 64 + 64]


def grid_cells(bins, c, frames):
    """The real cells of every track, float32 [F, bins] (c = 1) or [F, bins, 2]: uniform in [-16, 16] plus an offset per bin in
    [-4, 4]; the last track holds one value."""
    rng = np.random.default_rng(2000 + bins + c)
    off = rng.uniform(-4, 4, (bins, c))
    cells = [(rng.uniform(-16, 16, (F, bins, c)) + off).astype(np.float32) for F in frames]
    cells[-1][:] = CONSTANT
    return cells if c == 2 else [x[:, :, 0] for x in cells]


def affine_of(bins):
    rng = np.random.default_rng(77 + bins)
    return rng.uniform(-4, 4, bins).astype(np.float32), rng.uniform(0.05, 2, bins).astype(np.float32)


def request_of(pkg, bins, c, frames, S, norm, pad_mode, pad_value=-10.0):
    """The StftBatch of one run of the GPU test."""
    normalize = {"none": None, "whisper": "whisper", "refmax": "refmax", "cmn": "cmn", "cmvn": pkg.stft_norm("cmvn", var_floor=VAR_FLOOR),
                 "affine": ("affine",) + affine_of(bins)}[norm]
    return pkg.stft_batch_request(frames, bins, c, S, normalize, (pad_value, pad_mode))


def _collate(cells, bins, c, frames_major, sb, dtype):
    """The definition with every operation in `dtype`: float64 is the reference, float32 the bit-exact form of the norms without sums."""
    rec, S = sb.rec, sb.stride
    norm, normalized = int(rec["norm"][0]), int(rec["pad_mode"][0]) == 1
    pad, rng_, add, mul = (dtype(rec[k][0]) for k in ("pad_value", "range", "add", "mul"))
    out = np.zeros((len(cells), S, bins, c), dtype=dtype)
    for t, x32 in enumerate(cells):
        F = len(x32)
        x32 = x32.reshape(F, bins, c)

        def y(v):
            v = np.asarray(v, dtype=dtype)
            v = np.full((bins, c), v) if v.ndim == 0 else v  # (no arithmetic: NONE keeps a cell's bits, -0.0 among them)
            if norm in (1, 5):
                m = dtype(x32.max()) if F else dtype(-np.inf)
                lo = dtype(m - rng_)
                if norm == 1:
                    return ((np.maximum(v, lo) + add).astype(dtype) * mul).astype(dtype)
                return ((np.maximum(v, lo) - m).astype(dtype) * mul).astype(dtype)
            if norm in (2, 3):
                assert dtype is np.float64 and c == 1
                xs = x32.astype(np.float64)
                mean = xs.mean(axis=0) if F else np.zeros((bins, c))
                var = xs.var(axis=0) if F else np.zeros((bins, c))
                d = np.sqrt(np.maximum(var, float(rec["var_floor"][0]))) if norm == 3 else 1.0
                return (v - mean) / d
            if norm == 4:
                return ((v - sb.sub.astype(dtype)[:, None]).astype(dtype) * sb.mul.astype(dtype)[:, None]).astype(dtype)
            return v
        out[t, :F] = y(x32)
        out[t, F:] = pad if not normalized or (norm == 5 and F == 0) else y(pad)
    out = out if frames_major else out.transpose(0, 2, 1, 3)
    return np.ascontiguousarray(out if c == 2 else out[..., 0])


def stft_batch_ref(cells, bins, c, frames_major, sb):
    """STFT BATCHES in float64: cells[t] float32 [F[t], bins] (or [F[t], bins, 2] for pairs) -> float64 [n, S, bins(, 2)] (frames-
    major) or [n, bins, S(, 2)]."""
    return _collate(cells, bins, c, frames_major, sb, np.float64)


def stft_batch_f32(cells, bins, c, frames_major, sb):
    """NONE, WHISPER, REFMAX and AFFINE as the header writes them, every operation a rounded float32 one -> float32, stft_batch_ref's
    shape."""
    assert int(sb.rec["norm"][0]) in (0, 1, 4, 5)
    return _collate(cells, bins, c, frames_major, sb, np.float32)


# ---- ABI and refusals ---------------------------------------------------------------------------------------
def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    assert all(s in pkg.EXPORTS for s in NEW)
    assert pkg.STFT_BATCH_REQ_DTYPE.itemsize == 64 and pkg.STFT_BATCH_SPAN_DTYPE.itemsize == 24
    assert pkg.STFT_BATCH_REQ_DTYPE == pkg.FEAT_BATCH_REQ_DTYPE  # the fields of opusgpu_feat_batch_req
    header = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    assert "STFT BATCHES." in header and all(re.search(r"\b%s\(" % s, header) for s in NEW)
    assert re.search(r"#define OPUSGPU_STFT_NORM_REFMAX %d\b" % pkg.STFT_NORM_REFMAX, header) and pkg.STFT_NORM_REFMAX == 5
    assert "opusgpu_stft_batch_req { /* 64 bytes" in header and "opusgpu_stft_batch_span { /* 24 bytes" in header
    assert {k: v for k, v in pkg.STFT_NORMS.items() if k != "refmax"} == pkg.FEAT_NORMS


def good_request(pkg, **kw):
    rec = pkg.stft_batch_request([10], 257, 1, 320, "refmax").rec.copy()
    for k, v in kw.items():
        rec[k] = v
    return rec


def test_set_time_refusals(pkg, handles):
    lib = pkg.load_lib()
    assert lib.opusgpu_set_stft_batch(None, None, None, None, 0) == pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_ms_set_stft_batch(None, None, None, None, 0) == pkg.OPUSGPU_BAD_ARG
    sub, mul = affine_of(1025)
    bad_sub = sub.copy()
    bad_sub[1024] = np.inf
    big = np.ones(1026, dtype=np.float32)
    for fn, h in zip((lib.opusgpu_set_stft_batch, lib.opusgpu_ms_set_stft_batch), handles):
        def call(rec, s=None, m=None, bins=0):
            return fn(h, rec.ctypes.data, None if s is None else s.ctypes.data, None if m is None else m.ctypes.data, bins)
        for kw in (dict(norm=6), dict(norm=-1), dict(pad_mode=2), dict(pad_value=np.nan), dict(pad_value=np.inf), dict(range=np.nan),
                   dict(add=-np.inf), dict(mul=np.nan), dict(var_floor=np.nan), dict(var_floor=np.inf), dict(var_floor=0.0),
                   dict(var_floor=-1.0), dict(stride_frames=0), dict(stride_frames=-3), dict(reserved=[0, 0, 0, 0, 1]),
                   dict(reserved=[1, 0, 0, 0, 0])):
            assert call(good_request(pkg, **kw)) == pkg.OPUSGPU_BAD_ARG, kw
        affine = good_request(pkg, norm=pkg.FEAT_NORM_AFFINE)
        for s, m, bins in ((None, mul, 1025), (sub, None, 1025), (sub, mul, 0), (big, big, 1026), (bad_sub, mul, 1025), (sub, bad_sub, 1025)):
            assert call(affine, s, m, bins) == pkg.OPUSGPU_BAD_ARG
        assert call(good_request(pkg)) == 0 and call(affine, sub, mul, 1025) == 0 and call(affine, sub, mul, 129) == 0
        for norm in range(6):  # every norm of the section is taken at set time: what pairs refuse is known at the call
            assert call(good_request(pkg, norm=norm), sub, mul, 257) == 0
        assert call(good_request(pkg, enabled=0, norm=99)) == 0  # off: nothing of it is read
        assert fn(h, None, None, None, 0) == 0


def test_layout(pkg):
    lib = pkg.load_lib()
    n, bins, S = 5, 513, 3000
    for c in (1, 2):
        offs = np.full(n, -1, dtype=np.int64)
        assert lib.opusgpu_stft_batch_layout(n, bins, c, S, offs.ctypes.data) == n * S * bins * c
        assert np.array_equal(offs, np.arange(n) * S * bins * c)
    assert lib.opusgpu_stft_batch_layout(n, bins, 1, S, None) == n * S * bins and lib.opusgpu_stft_batch_layout(0, 1, 1, 1, None) == 0
    for bad in ((-1, bins, 1, S), (n, 0, 1, S), (n, 1026, 1, S), (n, bins, 0, S), (n, bins, 3, S), (n, bins, 1, 0), (n, bins, 1, -1)):
        assert lib.opusgpu_stft_batch_layout(*bad, None) == pkg.OPUSGPU_BAD_ARG, bad
    # S * bins * c at the limit and one above it
    top = 0x7fffffff
    assert lib.opusgpu_stft_batch_layout(1, 1, 1, top, None) == top
    assert lib.opusgpu_stft_batch_layout(1, 1, 1, top + 1, None) == pkg.OPUSGPU_BAD_ARG
    S1025 = top // 1025
    assert lib.opusgpu_stft_batch_layout(3, 1025, 1, S1025, None) == 3 * 1025 * S1025
    assert lib.opusgpu_stft_batch_layout(3, 1025, 1, S1025 + 1, None) == pkg.OPUSGPU_BAD_ARG
    S2 = top // (257 * 2)
    assert lib.opusgpu_stft_batch_layout(2, 257, 2, S2, None) == 2 * 514 * S2
    assert lib.opusgpu_stft_batch_layout(2, 257, 2, S2 + 1, None) == pkg.OPUSGPU_BAD_ARG
    assert pkg.stft_batch_layout(n, bins, 2, S)[1] == n * S * bins * 2
    with pytest.raises(ValueError):
        pkg.stft_batch_layout(n, 1026, 1, S)


def test_whole_file_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """A stride below a planned F, S * bins * c above the limit, AFFINE vectors of another length and a norm that pairs do not take:
    OPUSGPU_BAD_ARG from the STFT call of both kinds of decoder with d_out NULL, the arrays untouched, the reason in the decoder's
    message.  The other feature calls ignore the request."""
    lib = pkg.load_lib()
    enh, mag = stft_of(pkg, "enh"), stft_of(pkg, "enh", power=1)
    mix6 = pkg.mix_matrix("mono", 6)
    sub, mul = affine_of(129)
    for b, prefix, h, args in ((batch, "opusgpu_", handles[0], (16000, 0, 0, 1, None)), (ms_batch, "opusgpu_ms_", handles[1], (16000, 0, 0, mix6.ctypes.data))):
        setter, err, call = getattr(lib, prefix + "set_stft_batch"), getattr(lib, prefix + "last_error"), getattr(lib, prefix + "files_decode_stft")
        planned_f = pkg.stft_frames(enh, -(-b.info["track_samples"] // 3))
        assert planned_f.max() > 1
        arrays = [np.full(b.n_files, -7, dtype=np.int64) for _ in range(3)] + [np.full((b.n_files, 2), -7, dtype=np.int32)]
        tail = [a.ctypes.data for a in arrays]
        try:
            short = good_request(pkg, norm=0, stride_frames=int(planned_f.max()) - 1)
            assert setter(h, short.ctypes.data, None, None, 0) == 0
            assert call(h, b.h, *args, enh.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            assert b"stride_frames is below" in err(h)
            assert call(h, b.h, *args, mag.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            huge = good_request(pkg, norm=0, stride_frames=0x7fffffff // 514 + 1)
            assert setter(h, huge.ctypes.data, None, None, 0) == 0
            assert call(h, b.h, *args, enh.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            assert b"0x7fffffff" in err(h)
            affine = good_request(pkg, norm=pkg.FEAT_NORM_AFFINE, stride_frames=int(planned_f.max()))
            assert setter(h, affine.ctypes.data, sub.ctypes.data, mul.ctypes.data, 129) == 0
            assert call(h, b.h, *args, mag.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            assert b"AFFINE" in err(h)
            for norm in (1, 2, 3, 5):
                pairs = good_request(pkg, norm=norm, stride_frames=int(planned_f.max()))
                assert setter(h, pairs.ctypes.data, None, None, 0) == 0
                assert call(h, b.h, *args, enh.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG, norm
                assert b"pairs" in err(h)
            # the feature-batch request still refuses an STFT call, whatever this section's request says
            fb = pkg.feature_batch_request([10], 80, feature_stride=3000)
            assert getattr(lib, prefix + "set_feature_batch")(h, fb.rec.ctypes.data, None, None, 80) == 0
            try:
                assert call(h, b.h, *args, enh.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
                assert b"not batched" in err(h)
            finally:
                assert getattr(lib, prefix + "set_feature_batch")(h, None, None, None, 0) == 0
        finally:
            assert setter(h, None, None, None, 0) == 0
        assert all((a == -7).all() for a in arrays)


# ---- files_request ------------------------------------------------------------------------------------------
def test_the_new_keywords(pkg, batch, ms_batch):
    planned = batch.info["track_samples"]
    n = batch.n_files
    enh, vits, mag = stft_of(pkg, "enh"), stft_of(pkg, "vits", "frames"), stft_of(pkg, "enh", power=1)
    F = pkg.stft_frames(enh, -(-planned // 3))
    packed = pkg.files_request(batch, features=enh, mono=True)
    req = pkg.files_request(batch, features=enh, mono=True, stft_stride=320)
    sb = req.stft_batch
    assert (req.entry, req.args[:4], req.kind, req.channels) == (packed.entry, packed.args[:4], "features", 1) and packed.stft_batch is None
    assert req.feature_batch is None and req.wave_batch is None
    assert (sb.bins, sb.c, sb.stride, req.total) == (257, 2, 320, n * 320 * 514) and np.array_equal(req.offsets, np.arange(n) * 320 * 514)
    assert (req.planes == 320).all() and F.max() <= 320
    rec = sb.rec
    assert rec.dtype == pkg.STFT_BATCH_REQ_DTYPE and rec.shape == (1,) and int(rec["enabled"][0]) == 1
    assert (int(rec["norm"][0]), int(rec["pad_mode"][0]), float(rec["pad_value"][0])) == (pkg.FEAT_NORM_NONE, pkg.FEAT_PAD_VALUE, 0.0)
    assert (rec["reserved"] == 0).all()
    # stft_normalize= alone: S is the largest planned F; refmax reads range 8 and mul 10; whisper pads as FEATURE BATCHES does
    alone = pkg.files_request(batch, features=mag, mono=True, stft_normalize="refmax").stft_batch
    assert (alone.bins, alone.c, alone.stride) == (257, 1, F.max()) and int(alone.rec["norm"][0]) == pkg.STFT_NORM_REFMAX
    assert (float(alone.rec["range"][0]), float(alone.rec["mul"][0]), int(alone.rec["pad_mode"][0]), float(alone.rec["pad_value"][0])) == (8.0, 10.0, 0, 0.0)
    wh = pkg.files_request(batch, features=mag, mono=True, stft_normalize="whisper").stft_batch.rec
    assert (float(wh["range"][0]), float(wh["add"][0]), float(wh["mul"][0]), int(wh["pad_mode"][0]), float(wh["pad_value"][0])) == (8.0, 4.0, 0.25, 1, -10.0)
    own = pkg.stft_norm("refmax", range=6, mul=20)
    orec = pkg.files_request(batch, features=mag, mono=True, stft_normalize=own, stft_pad=(-120, "normalized")).stft_batch.rec
    assert (float(orec["range"][0]), float(orec["mul"][0]), int(orec["pad_mode"][0]), float(orec["pad_value"][0])) == (6.0, 20.0, 1, -120.0)
    assert float(pkg.files_request(batch, features=mag, mono=True, stft_normalize=pkg.stft_norm("cmvn", var_floor=0.5), stft_pad=2).stft_batch.rec["var_floor"][0]) == 0.5
    # affine on pairs, with vectors of `bins` entries
    sub, mul = affine_of(257)
    ab = pkg.files_request(batch, features=enh, mono=True, stft_normalize=("affine", sub, mul)).stft_batch
    assert int(ab.rec["norm"][0]) == pkg.FEAT_NORM_AFFINE and np.array_equal(ab.sub, sub) and np.array_equal(ab.mul, mul) and ab.c == 2
    # a record at a ratio, frames-major; the multistream batch; rate= / resample= / loudness= compose
    vreq = pkg.files_request(batch, features=vits, mono=True, stft_stride=192, stft_normalize="cmn")
    assert (vreq.stft_batch.bins, vreq.stft_batch.c, vreq.total) == (513, 1, n * 192 * 513) and vreq.args[:3] == (0, 147, 320)
    assert pkg.stft_frames(vits, -(-planned * 147 // 320)).max() <= 192
    ms = pkg.files_request(ms_batch, True, 0, features=enh, mix="mono", stft_stride=320)
    assert ms.entry == "files_decode_stft" and ms.total == ms_batch.n_files * 320 * 514
    assert pkg.files_request(batch, features=enh, mono=True, resample=16000, stft_stride=320, loudness=-23.0).loudness is not None
    # out= is held against the dense size, in floats
    ok = Tensor(req.total)
    assert pkg.files_request(batch, features=enh, mono=True, stft_stride=320, out=ok).out is ok
    with pytest.raises(ValueError):
        pkg.files_request(batch, features=enh, mono=True, stft_stride=320, out=Tensor(req.total - 1))
    assert pkg.files_request(batch, features=enh, mono=True, out=Tensor(packed.total)).stft_batch is None


class _Mem:
    """What _run_files_request asks of a Context, with a fake C call that fills the arrays: enough to see the result's shape."""

    def dev_alloc(self, nbytes):
        return 0

    def dev_free(self, p):
        pass

    def d2h(self, arr, p):
        arr[:] = 1.0


def test_the_result_is_one_tensor_complex_over_pairs(pkg, batch):
    """_run_files_request over a library that does nothing: [n, bins, S] float32 for real cells, complex64 of the same shape (a view
    of the pairs) for the complex STFT, [n, S, bins] frames-major; the request is set before the call and cleared behind it."""
    n = batch.n_files
    calls = []

    class Lib:
        def __getattr__(self, name):
            def fn(*a):
                calls.append((name, a[1] is not None if len(a) > 1 else None))
                return 0
            return fn
    for rec, dtype, shape in ((stft_of(pkg, "enh"), np.complex64, (n, 257, 320)), (stft_of(pkg, "enh", "frames"), np.complex64, (n, 320, 257)),
                              (stft_of(pkg, "enh", power=2), np.float32, (n, 257, 320))):
        req = pkg.files_request(batch, features=rec, mono=True, stft_stride=320)
        calls.clear()
        req = req._replace(offsets=np.zeros(n, dtype=np.int64))  # (the fake call leaves the offsets 0)
        dense, info = pkg._run_files_request(req, Lib(), "opusgpu_", None, lambda rc, what: None, batch, _Mem())
        assert dense.dtype == dtype and dense.shape == shape and (dense == (1 + 1j if dtype == np.complex64 else 1)).all()
        assert [c[0] for c in calls] == ["opusgpu_set_stft_batch", "opusgpu_files_decode_stft", "opusgpu_set_stft_batch"]
        assert calls[0][1] is True and calls[2][1] is False


def test_value_errors(pkg, batch):
    enh, mag = stft_of(pkg, "enh"), stft_of(pkg, "enh", power=1)
    F = int(pkg.stft_frames(enh, -(-batch.info["track_samples"] // 3)).max())
    sub, mul = affine_of(257)
    nan = sub.copy()
    nan[3] = np.nan
    real, pairs = dict(features=mag, mono=True), dict(features=enh, mono=True)
    for kw in (dict(stft_stride=320), dict(stft_normalize="cmn"), dict(stft_pad=0.0),                      # no features
               dict(rate=16000, mono=True, stft_normalize="cmn"),                                           # tracks
               dict(features="logmel", mono=True, stft_stride=3000), dict(features="logmel", mono=True, stft_normalize="whisper"),
               dict(features=pkg.mel_spec(16000, 512, 160, 400), mono=True, stft_pad=0.0), dict(features=pkg.kaldi_fbank(), mono=True, stft_stride=3000),
               dict(pairs, stft_normalize="whisper"), dict(pairs, stft_normalize="refmax"), dict(pairs, stft_normalize="cmn"),
               dict(pairs, stft_normalize="cmvn"), dict(pairs, stft_normalize=pkg.stft_norm("refmax", range=6)),
               dict(real, stft_normalize="l2"), dict(real, stft_normalize=3), dict(real, stft_normalize=("affine", sub)),
               dict(real, stft_normalize=("scale", sub, mul)), dict(real, stft_normalize=("affine", sub[:256], mul[:256])),
               dict(real, stft_normalize=("affine", sub, mul[:256])), dict(real, stft_normalize=("affine", nan, mul)),
               dict(real, stft_normalize=("affine", sub, nan)), dict(real, stft_stride=F - 1), dict(pairs, stft_stride=F - 1),
               dict(real, stft_stride=0), dict(real, stft_stride=320.0), dict(real, stft_stride=True), dict(real, stft_stride=1 << 30),
               dict(pairs, stft_stride=0x7fffffff // 514 + 1), dict(real, stft_pad=np.nan), dict(real, stft_pad=(0.0, "reflect")),
               dict(real, stft_pad="zero"),
               dict(pairs, stft_stride=320, feature_stride=320),  # FEATURE BATCHES' keywords stay refused with the record
               dict(pairs, stft_stride=320, wave_stride=320), dict(pairs, stft_stride=320, format="s16")):
        with pytest.raises(ValueError):
            pkg.files_request(batch, **kw)
    assert pkg.files_request(batch, stft_stride=F, **real).stft_batch.stride == F
    assert pkg.files_request(batch, stft_stride=0x7fffffff // 514, **pairs).stft_batch.stride == 0x7fffffff // 514
    for kw in (dict(feature_stride=320), dict(normalize="cmn"), dict(feature_pad=0.0)):
        with pytest.raises(ValueError, match="1 - 128"):
            pkg.files_request(batch, stft_stride=320, **pairs, **kw)
    for kw in (dict(var_floor=0.0), dict(var_floor=np.nan), dict(range=np.inf), dict(sub=sub)):
        with pytest.raises(ValueError):
            pkg.stft_norm("cmvn", **kw)
    for kind in ("affine", "db", 5):
        with pytest.raises(ValueError):
            pkg.stft_norm(kind)
    with pytest.raises(ValueError):
        pkg.stft_norm("affine", sub=np.zeros(1026), mul_vec=np.ones(1026))
    with pytest.raises(ValueError):
        pkg.stft_batch_request([10], 257, 3, 320)
    # the batch's own stride= stays refused, with the message it had
    import files_util as fu
    sbatch = pkg.FileBatch([c[1] for c in fu.corpus20(2, channel_switches=False)[:4]], channels=2, cuts=[(0, 0, 4800), (1, 960, 2880)], stride=4800)
    try:
        with pytest.raises(ValueError) as e:
            pkg.files_request(sbatch, stft_stride=320, **pairs)
        assert str(e.value) == pkg.STRIDE_REFUSED
    finally:
        sbatch.close()


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_requests_without_the_keywords_are_what_they_were(pkg, batch, ms_batch, row):
    kw, *want = TABLE[row]
    for b, multistream, expected in ((batch, False, want[0]), (ms_batch, True, want[1])):
        if expected is None:
            continue
        plain = pkg.files_request(b, multistream, 0, **keywords(pkg, kw))
        named = pkg.files_request(b, multistream, 0, stft_stride=None, stft_normalize=None, stft_pad=None, **keywords(pkg, kw))
        same_request(pkg, plain, named)
        assert plain.stft_batch is None and plain._fields[-1] == "stft_batch"
        assert (plain.entry, plain.channels, plain.kind) == (expected[0], expected[2], expected[3])


def test_the_packed_stft_request_is_what_it_was(pkg, batch):
    for rec in (stft_of(pkg, "enh"), stft_of(pkg, "vits", "frames")):
        plain = pkg.files_request(batch, features=rec, mono=True)
        named = pkg.files_request(batch, features=rec, mono=True, stft_stride=None, stft_normalize=None, stft_pad=None)
        same_request(pkg, plain, named)
        offs, planes, total = pkg.stft_layout(batch.info["track_samples"], *((1, 3) if int(rec["sample_rate"][0]) == 16000 else (147, 320)), rec)
        assert plain.total == total and np.array_equal(plain.offsets, offs) and np.array_equal(plain.planes, planes)


# ---- kernels ------------------------------------------------------------------------------------------------
def test_kernel_resources():
    """k_stft_stats, k_stft_fold, k_stft_batch and k_stft_pad once each, no scratch; static LDS only in k_stft_stats, k_feat_stats'
    8,192 bytes at any width (a workgroup per chunk of 128 bins); at most 64 registers: 8 waves per SIMD.  No k_feat_* or k_tracks_*
    name matches them."""
    meta = _kernel_metadata()
    for name, lds_most in (("k_stft_stats", 8192), ("k_stft_fold", 0), ("k_stft_batch", 0), ("k_stft_pad", 0)):
        seen = [v for mangled, v in meta.items() if re.search(r"\d+" + name + r"(P|E|v|$)", mangled)]
        print(name, seen)
        assert len(seen) == 1, (name, sorted(meta)[:6])
        vgpr, scratch, lds = seen[0]
        assert scratch == 0 and lds <= lds_most and vgpr <= 64
    assert not [m for m in meta if re.search(r"k_(tracks|feat)_\w*", m) and "k_stft_" in m]


# ---- the restatement ----------------------------------------------------------------------------------------
def test_the_restatement_by_hand(pkg):
    """stft_batch_ref and stft_batch_f32 on a grid small enough to work out by hand: REFMAX with a log10 power spectrogram's numbers
    is librosa.power_to_db(ref=np.max, top_db=80) of the power; a track without a frame is pad_value verbatim; pairs under AFFINE."""
    x = np.array([[0.0, -3.0], [-9.5, -1.0], [-2.0, -0.5]], dtype=np.float32)  # [F = 3, bins = 2] log10 power
    sb = pkg.stft_batch_request([3, 0], 2, 1, 4, "refmax", (-7.0, "normalized"))
    got = stft_batch_f32([x, x[:0]], 2, 1, True, sb)
    db = 10.0 * np.maximum(x, x.max() - 8.0) - 10.0 * x.max()  # power_to_db: 10 log10(S) - 10 log10(max), floored at max - 80
    assert got.shape == (2, 4, 2) and np.array_equal(got[0, :3], db.astype(np.float32))
    assert (got[0, 3] == np.float32((max(-7.0, 0.0 - 8.0) - 0.0) * 10.0)).all() and (got[1] == np.float32(-7.0)).all()
    assert np.array_equal(stft_batch_ref([x, x[:0]], 2, 1, True, sb), got.astype(np.float64))  # (exact in both at these numbers)
    assert np.array_equal(stft_batch_f32([x, x[:0]], 2, 1, False, sb), got.transpose(0, 2, 1))
    z = np.arange(12, dtype=np.float32).reshape(3, 2, 2)
    ab = pkg.stft_batch_request([3], 2, 2, 5, ("affine", [1.0, 2.0], [0.5, 2.0]), 9.0)
    pairs = stft_batch_f32([z], 2, 2, False, ab)
    assert pairs.shape == (1, 2, 5, 2) and np.array_equal(pairs[0, 1, :3], (z[:, 1] - 2.0) * 2.0) and (pairs[0, :, 3:] == 9.0).all()
    cm = pkg.stft_batch_request([3], 2, 1, 3, "cmn")
    assert np.allclose(stft_batch_ref([x], 2, 1, True, cm)[0].mean(axis=0), 0, atol=1e-15)
