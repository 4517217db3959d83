"""Feature batches of the whole-file path (include/opusgpu.h, FEATURE BATCHES), what needs no GPU: the exported symbols and the
records, every refusal of opusgpu_set_feature_batch, the layout call, the whole-file refusals that come before device work, what
files_request makes of feature_stride= / normalize= / feature_pad=, the kernels' resources, and the tolerance that
tests/test_gpu_feat_batch.py holds CMN and CMVN to.

feat_batch_ref is the float64 numpy restatement of the header's definition; feat_batch_f32 the plain float32 forms of NONE, WHISPER
and AFFINE, which the kernels must equal bit for bit.  GRIDS are the synthetic grids the GPU test uploads.

THE BOUND (bound_of).  A CMN / CMVN cell may differ from feat_batch_ref by 2^-23 |y| + 2^-30 max_f |x[f][j]| / d, d = 1 (CMN) or
sqrt(max(var_j, var_floor)) (CMVN): the final float32 rounding is 2^-24 relative; a double mean over F <= 2^20 frames errs by at most
F 2^-53 max |x| <= 2^-33 max |x|; a one-pass double variance on these inputs (|x| <= 20, var_j >= 0.25 wherever F > 3, F <= 5000)
errs by about 2^-32 relative, which moves y by that much of |y|.  test_the_bound_separates_double_from_float shows on the GPU
test's own F = 5000 track that float64 restatements in one-pass and two-pass form, summed in sequence, stay within a quarter of it and
that a float32-accumulating CMN leaves it.  Observed ratios error / bound, worst cell: one-pass 6.0e-08 (CMVN; CMN's mean came
out the same double), two-pass 0 to the digits printed, float32 accumulation 404."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_files_request import TABLE, keywords
from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_set_feature_batch", "opusgpu_ms_set_feature_batch", "opusgpu_feat_batch_layout", "opusgpu_tracks_feature_batch_device"]
NORMS = ["none", "whisper", "cmn", "cmvn", "affine"]
VAR_FLOOR = 1e-4
# the frames of the tracks of one call, by feature width: the segment edges (1023, 1024, 1025), a multi-segment track (5000), the
# 16-byte piece and 64-frame edges, a track without a frame; the last track of either set is the constant one
FRAMES_A, FRAMES_B = [5000, 0, 1025, 64, 3, 300], [1024, 5000, 257, 65, 63, 1, 1023, 300]
WIDTHS = {1: FRAMES_B, 3: FRAMES_B, 13: FRAMES_B, 64: FRAMES_A, 65: FRAMES_B, 80: FRAMES_A, 128: FRAMES_A}
CONSTANT = np.float32(3.7)


def strides_of(frames):
    m = max(frames)
    return [m, m + 1, 5003, 5004, 5056]


def grid_cells(W, frames):
    """The real cells of every track, float32 [F, W]: uniform in [-16, 16] plus an offset per bin in [-4, 4]; the last track holds one
    value."""
    rng = np.random.default_rng(1000 + W)
    off = rng.uniform(-4, 4, W)
    cells = [(rng.uniform(-16, 16, (F, W)) + off).astype(np.float32) for F in frames]
    cells[-1][:] = CONSTANT
    return cells


def affine_of(W):
    rng = np.random.default_rng(77 + W)
    return rng.uniform(-4, 4, W).astype(np.float32), rng.uniform(0.05, 2, W).astype(np.float32)


def request_of(pkg, W, frames, S, norm, pad_mode, pad_value=-10.0):
    """The FeatureBatch of one run of the GPU test."""
    normalize = {"none": None, "whisper": "whisper", "cmn": "cmn", "cmvn": pkg.feature_norm("cmvn", var_floor=VAR_FLOOR),
                 "affine": ("affine",) + affine_of(W)}[norm]
    return pkg.feature_batch_request(frames, W, S, normalize, (pad_value, pad_mode))


def stats_of(x, rec):
    """Per bin, in float64 from the header's definition: (mean_j, d_j) of a track's real cells x [F, W]."""
    F, W = x.shape
    x = x.astype(np.float64)
    mean = x.mean(axis=0) if F else np.zeros(W)
    var = x.var(axis=0) if F else np.zeros(W)
    d = np.sqrt(np.maximum(var, float(rec["var_floor"][0]))) if int(rec["norm"][0]) == 3 else np.ones(W)
    return mean, d


def feat_batch_ref(cells, W, frames_major, fb):
    """FEATURE BATCHES in float64: cells[t] float32 [F[t], W] -> float64 [n, S, W] (frames-major) or [n, W, S]."""
    rec, S = fb.rec, fb.stride
    norm, normalized = int(rec["norm"][0]), int(rec["pad_mode"][0]) == 1
    pad, rng_, add, mul = (np.float64(rec[k][0]) for k in ("pad_value", "range", "add", "mul"))
    out = np.zeros((len(cells), S, W))
    for t, x in enumerate(cells):
        F = len(x)

        def y(v):
            v = np.asarray(v, dtype=np.float64)
            if norm == 1:
                m = x.max() if F else -np.inf
                return (np.maximum(v, m - rng_) + add) * mul
            if norm in (2, 3):
                mean, d = stats_of(x, rec)
                return (v - mean) / d
            if norm == 4:
                return (v - fb.sub.astype(np.float64)) * fb.mul.astype(np.float64)
            return v + np.zeros(W)
        out[t, :F] = y(x)
        out[t, F:] = y(pad) if normalized else pad
    return out if frames_major else out.transpose(0, 2, 1)


def feat_batch_f32(cells, W, frames_major, fb):
    """NONE, WHISPER and AFFINE as the header writes them, every operation a rounded float32 one -> float32, feat_batch_ref's shape."""
    rec, S = fb.rec, fb.stride
    norm, normalized = int(rec["norm"][0]), int(rec["pad_mode"][0]) == 1
    pad, rng_, add, mul = (np.float32(rec[k][0]) for k in ("pad_value", "range", "add", "mul"))
    assert norm in (0, 1, 4)
    out = np.zeros((len(cells), S, W), dtype=np.float32)
    for t, x in enumerate(cells):
        F = len(x)

        def y(v):
            v = np.asarray(v, dtype=np.float32)
            if norm == 1:
                m = x.max() if F else np.float32(-np.inf)
                return ((np.maximum(v, np.float32(m - rng_)) + add).astype(np.float32) * mul).astype(np.float32)
            if norm == 4:
                return ((v - fb.sub).astype(np.float32) * fb.mul).astype(np.float32)
            return v + np.zeros(W, dtype=np.float32)
        out[t, :F] = y(x)
        out[t, F:] = y(pad) if normalized else pad
    return out if frames_major else out.transpose(0, 2, 1)


def bound_of(cells, W, frames_major, fb, ref):
    """THE BOUND above for every cell of `ref` (feat_batch_ref's result), pad cells included."""
    rec = fb.rec
    top = np.zeros((len(cells), 1, W))
    for t, x in enumerate(cells):
        if len(x):
            top[t, 0] = np.abs(x.astype(np.float64)).max(axis=0) / stats_of(x, rec)[1]
    y = ref if frames_major else ref.transpose(0, 2, 1)
    b = 2.0 ** -23 * np.abs(y) + 2.0 ** -30 * top
    return b if frames_major else b.transpose(0, 2, 1)


# ---- ABI and refusals ---------------------------------------------------------------------------------------
def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    assert all(s in pkg.EXPORTS for s in NEW)
    assert pkg.FEAT_BATCH_REQ_DTYPE.itemsize == 64 and pkg.FEAT_SPAN_DTYPE.itemsize == 24
    header = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    assert "FEATURE BATCHES." in header and all(re.search(r"\b%s\(" % s, header) for s in NEW)
    assert re.search(r"#define OPUSGPU_FEAT_SEG %d\b" % pkg.FEAT_SEG, header)
    for name, v in pkg.FEAT_NORMS.items():
        if name not in (None, "none"):
            assert re.search(r"#define OPUSGPU_FEAT_NORM_%s %d\b" % (name.upper(), v), header)


def good_request(pkg, **kw):
    rec = pkg.feature_batch_request([10], 80, 3000, "whisper").rec.copy()
    for k, v in kw.items():
        rec[k] = v
    return rec


def test_set_time_refusals(pkg, handles):
    lib = pkg.load_lib()
    assert lib.opusgpu_set_feature_batch(None, None, None, None, 0) == pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_ms_set_feature_batch(None, None, None, None, 0) == pkg.OPUSGPU_BAD_ARG
    sub, mul = affine_of(80)
    bad_sub = sub.copy()
    bad_sub[79] = np.inf
    for fn, h in zip((lib.opusgpu_set_feature_batch, lib.opusgpu_ms_set_feature_batch), handles):
        def call(rec, s=None, m=None, width=0):
            return fn(h, rec.ctypes.data, None if s is None else s.ctypes.data, None if m is None else m.ctypes.data, width)
        for kw in (dict(norm=5), dict(norm=-1), dict(pad_mode=2), dict(pad_value=np.nan), dict(pad_value=np.inf), dict(range=np.nan),
                   dict(add=-np.inf), dict(mul=np.nan), dict(var_floor=np.nan), dict(var_floor=np.inf), dict(var_floor=0.0),
                   dict(var_floor=-1.0), dict(stride_frames=0), dict(stride_frames=-3), dict(reserved=[0, 0, 0, 0, 1]),
                   dict(reserved=[1, 0, 0, 0, 0])):
            assert call(good_request(pkg, **kw)) == pkg.OPUSGPU_BAD_ARG, kw
        affine = good_request(pkg, norm=pkg.FEAT_NORM_AFFINE)
        for s, m, width in ((None, mul, 80), (sub, None, 80), (sub, mul, 0), (sub, mul, 129), (bad_sub, mul, 80), (sub, bad_sub, 80)):
            assert call(affine, s, m, width) == pkg.OPUSGPU_BAD_ARG
        assert call(good_request(pkg)) == 0 and call(affine, sub, mul, 80) == 0
        assert call(good_request(pkg, enabled=0, norm=99)) == 0  # off: nothing of it is read
        assert fn(h, None, None, None, 0) == 0


def test_layout(pkg):
    lib = pkg.load_lib()
    n, W, S = 5, 80, 3000
    offs = np.full(n, -1, dtype=np.int64)
    assert lib.opusgpu_feat_batch_layout(n, W, S, offs.ctypes.data) == n * S * W
    assert np.array_equal(offs, np.arange(n) * S * W)
    assert lib.opusgpu_feat_batch_layout(n, W, S, None) == n * S * W and lib.opusgpu_feat_batch_layout(0, 1, 1, None) == 0
    for bad in ((-1, W, S), (n, 0, S), (n, 129, S), (n, W, 0), (n, 128, (1 << 24))):
        assert lib.opusgpu_feat_batch_layout(*bad, None) == pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_feat_batch_layout(3, 128, (1 << 24) - 1, None) == 3 * 128 * ((1 << 24) - 1)
    assert pkg.feat_batch_layout(n, W, S)[1] == n * S * W


def test_whole_file_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """A stride below a planned F and AFFINE vectors of another width: OPUSGPU_BAD_ARG from the feature calls of both kinds of
    decoder with d_out NULL, the arrays untouched, the reason in the decoder's message; without the request the same call gets
    past these checks."""
    lib = pkg.load_lib()
    params = pkg.mel_params(80, "bands")
    kaldi = pkg.kaldi_fbank(num_mel_bins=23)
    mix6 = pkg.mix_matrix("mono", 6)
    sub, mul = affine_of(80)
    for b, prefix, h, mel_args, fbank_args in ((batch, "opusgpu_", handles[0], (1, None), (16000, 0, 0, 1, None)),
                                               (ms_batch, "opusgpu_ms_", handles[1], (mix6.ctypes.data,), (16000, 0, 0, mix6.ctypes.data))):
        setter, err = getattr(lib, prefix + "set_feature_batch"), getattr(lib, prefix + "last_error")
        planned_f = -(-b.info["track_samples"] // 3) // 160
        assert planned_f.max() > 1
        arrays = [np.full(b.n_files, -7, dtype=np.int64) for _ in range(3)] + [np.full((b.n_files, 2), -7, dtype=np.int32)]
        tail = [a.ctypes.data for a in arrays]
        short = good_request(pkg, stride_frames=int(planned_f.max()) - 1)
        assert setter(h, short.ctypes.data, None, None, 0) == 0
        try:
            assert getattr(lib, prefix + "files_decode_mel")(h, b.h, *mel_args, params.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            assert b"stride_frames is below" in err(h)
            kaldi_f = int(pkg.fbank_frames(kaldi, -(-b.info["track_samples"] // 3)).max())
            assert 1 < kaldi_f < planned_f.max()  # (snip_edges: fewer frames than the log-mel's)
            short = good_request(pkg, stride_frames=kaldi_f - 1)
            assert setter(h, short.ctypes.data, None, None, 0) == 0
            assert getattr(lib, prefix + "files_decode_fbank")(h, b.h, *fbank_args, kaldi.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            affine = good_request(pkg, norm=pkg.FEAT_NORM_AFFINE, stride_frames=int(planned_f.max()))
            assert setter(h, affine.ctypes.data, sub.ctypes.data, mul.ctypes.data, 80) == 0
            assert getattr(lib, prefix + "files_decode_fbank")(h, b.h, *fbank_args, kaldi.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            assert b"AFFINE" in err(h)
            huge = good_request(pkg, stride_frames=1 << 30)
            assert setter(h, huge.ctypes.data, None, None, 0) == 0
            assert getattr(lib, prefix + "files_decode_mel")(h, b.h, *mel_args, params.ctypes.data, None, None, *tail) == pkg.OPUSGPU_BAD_ARG
            assert b"0x7fffffff" in err(h)
        finally:
            assert setter(h, None, None, None, 0) == 0
        assert all((a == -7).all() for a in arrays)


# ---- files_request ------------------------------------------------------------------------------------------
def same_request(pkg, a, b):
    assert type(a) is type(b) and a._fields == b._fields
    for f in a._fields:
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y), f
        else:
            assert x is y or x == y, f


def test_the_new_keywords(pkg, batch, ms_batch):
    planned = batch.info["track_samples"]
    F = -(-planned // 3) // 160
    n = batch.n_files
    packed = pkg.files_request(batch, features="logmel", mono=True)
    req = pkg.files_request(batch, features="logmel", mono=True, feature_stride=3000, normalize="whisper")
    fb = req.feature_batch
    assert (req.entry, req.args[0], req.kind, req.channels) == (packed.entry, packed.args[0], "features", 1) and packed.feature_batch is None
    assert (fb.width, fb.stride, req.total) == (80, 3000, n * 3000 * 80) and np.array_equal(req.offsets, np.arange(n) * 240000)
    assert (req.planes == 3000).all()
    rec = fb.rec
    assert rec.dtype == pkg.FEAT_BATCH_REQ_DTYPE and rec.shape == (1,) and int(rec["enabled"][0]) == 1
    assert (int(rec["norm"][0]), int(rec["pad_mode"][0]), float(rec["pad_value"][0])) == (pkg.FEAT_NORM_WHISPER, pkg.FEAT_PAD_NORMALIZED, -10.0)
    assert (float(rec["range"][0]), float(rec["add"][0]), float(rec["mul"][0])) == (8.0, 4.0, 0.25) and (rec["reserved"] == 0).all()
    # normalize= alone: S is the largest planned F; everything but whisper pads with 0 verbatim
    alone = pkg.files_request(batch, features="logmel", mono=True, normalize="cmn", feature_layout="frames").feature_batch
    assert alone.stride == F.max() and (int(alone.rec["pad_mode"][0]), float(alone.rec["pad_value"][0])) == (pkg.FEAT_PAD_VALUE, 0.0)
    assert int(alone.rec["norm"][0]) == pkg.FEAT_NORM_CMN and float(alone.rec["var_floor"][0]) == 1e-20
    only = pkg.files_request(batch, features="logmel", mono=True, feature_stride=int(F.max())).feature_batch
    assert int(only.rec["norm"][0]) == pkg.FEAT_NORM_NONE
    # Kaldi records: the width is n_ceps for MFCC; the planned frames are the record's
    mfcc = pkg.kaldi_mfcc(num_mel_bins=23, num_ceps=13)
    sub, mul = affine_of(13)
    kf = pkg.fbank_frames(mfcc, -(-planned // 3))
    kreq = pkg.files_request(batch, features=mfcc, mono=True, normalize=("affine", sub, mul), feature_pad=(1.5, "normalized"))
    kb = kreq.feature_batch
    assert (kb.width, kb.stride, kreq.total) == (13, kf.max(), n * kf.max() * 13) and np.array_equal(kb.sub, sub) and np.array_equal(kb.mul, mul)
    assert (int(kb.rec["pad_mode"][0]), float(kb.rec["pad_value"][0])) == (pkg.FEAT_PAD_NORMALIZED, 1.5)
    own = pkg.feature_norm("cmvn", var_floor=0.5)
    assert float(pkg.files_request(batch, features=mfcc, mono=True, normalize=own, feature_pad=2).feature_batch.rec["var_floor"][0]) == 0.5
    w = pkg.feature_norm("whisper", range=6, add=3, mul=0.5)
    wrec = pkg.files_request(batch, features="logmel", mono=True, normalize=w).feature_batch.rec
    assert (float(wrec["range"][0]), float(wrec["add"][0]), float(wrec["mul"][0])) == (6.0, 3.0, 0.5)
    # a mel_spec record at a ratio, and the multistream batch
    from test_tracks_melspec import spec_of
    tts = spec_of(pkg, "tts")
    treq = pkg.files_request(batch, features=tts, mono=True, feature_stride=700)
    assert treq.feature_batch.width == int(tts["n_mels"][0]) and treq.args[:3] == (0, 147, 320)
    assert pkg.spec_frames(tts, -(-planned * 147 // 320)).max() <= 700
    ms = pkg.files_request(ms_batch, True, 0, features="logmel", mix="mono", normalize="whisper", feature_stride=3000)
    assert ms.entry == "files_decode_mel" and ms.total == ms_batch.n_files * 240000
    # out= is held against the dense size
    ok = Tensor(req.total)
    assert pkg.files_request(batch, features="logmel", mono=True, feature_stride=3000, normalize="whisper", out=ok).out is ok
    with pytest.raises(ValueError):
        pkg.files_request(batch, features="logmel", mono=True, feature_stride=3000, normalize="whisper", out=Tensor(req.total - 1))
    assert pkg.files_request(batch, features="logmel", mono=True, out=Tensor(packed.total)).feature_batch is None


def test_value_errors(pkg, batch):
    F = int((-(-batch.info["track_samples"] // 3) // 160).max())
    sub, mul = affine_of(80)
    nan = sub.copy()
    nan[3] = np.nan
    for kw in (dict(feature_stride=3000), dict(normalize="cmn"), dict(feature_pad=0.0), dict(rate=16000, mono=True, normalize="cmn"),
               dict(features="logmel", mono=True, normalize="l2"), dict(features="logmel", mono=True, normalize=3),
               dict(features="logmel", mono=True, normalize=("affine", sub)), dict(features="logmel", mono=True, normalize=("scale", sub, mul)),
               dict(features="logmel", mono=True, normalize=("affine", sub[:79], mul[:79])),
               dict(features="logmel", mono=True, normalize=("affine", sub, mul[:79])), dict(features="logmel", mono=True, normalize=("affine", nan, mul)),
               dict(features="logmel", mono=True, normalize=("affine", sub, nan)), dict(features="logmel", mono=True, feature_stride=F - 1),
               dict(features="logmel", mono=True, feature_stride=0), dict(features="logmel", mono=True, feature_stride=3000.0),
               dict(features="logmel", mono=True, feature_stride=1 << 30), dict(features="logmel", mono=True, feature_pad=np.nan),
               dict(features="logmel", mono=True, feature_pad=(0.0, "reflect")), dict(features="logmel", mono=True, feature_pad="zero")):
        with pytest.raises(ValueError):
            pkg.files_request(batch, **kw)
    assert pkg.files_request(batch, features="logmel", mono=True, feature_stride=F).feature_batch.stride == F
    for kw in (dict(var_floor=0.0), dict(var_floor=np.nan), dict(range=np.inf), dict(sub=sub)):
        with pytest.raises(ValueError):
            pkg.feature_norm("cmvn", **kw)
    with pytest.raises(ValueError):
        pkg.feature_norm("affine")
    # the batch's own stride= with features stays refused, with the message it had
    sb = pkg.FileBatch(batch_files(pkg), channels=2, cuts=[(0, 0, 4800), (1, 960, 2880)], stride=4800)
    try:
        with pytest.raises(ValueError) as e:
            pkg.files_request(sb, features="logmel", mono=True, feature_stride=3000)
        assert str(e.value) == pkg.STRIDE_REFUSED
    finally:
        sb.close()


def batch_files(pkg):
    import files_util as fu
    return [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_requests_without_the_keywords_are_what_they_were(pkg, batch, ms_batch, row):
    kw, *want = TABLE[row]
    for b, multistream, expected in ((batch, False, want[0]), (ms_batch, True, want[1])):
        if expected is None:
            continue
        plain = pkg.files_request(b, multistream, 0, **keywords(pkg, kw))
        named = pkg.files_request(b, multistream, 0, feature_stride=None, normalize=None, feature_pad=None, **keywords(pkg, kw))
        same_request(pkg, plain, named)
        assert plain.feature_batch is None and (plain.entry, plain.channels, plain.kind) == (expected[0], expected[2], expected[3])


# ---- kernels ------------------------------------------------------------------------------------------------
def test_kernel_resources():
    """k_feat_stats and k_feat_batch once each, no scratch; static LDS only in k_feat_stats: the four-wave combine of (sum, sum of
    squares) in double over 128 bins, 4 * 128 * 2 * 8 = 8,192 bytes -- 8 waves per SIMD are 8 workgroups of 256 a CU, which 160 KB of
    LDS allow up to 20,480 bytes each.  No k_tracks_* name matches them."""
    meta = _kernel_metadata()
    for name, lds_most in (("k_feat_stats", 8192), ("k_feat_fold", 0), ("k_feat_batch", 0)):
        seen = [v for mangled, v in meta.items() if re.search(r"\d+" + name + r"(P|E|v|$)", mangled)]
        print(name, seen)
        assert len(seen) == 1, (name, sorted(meta)[:6])
        vgpr, scratch, lds = seen[0]
        assert scratch == 0 and lds <= lds_most and 8 * lds <= 160 * 1024
        assert vgpr <= 64  # 8 waves per SIMD by registers too
    assert not [m for m in meta if re.search(r"k_tracks_\w*", m) and "k_feat" in m]


# ---- the tolerance ------------------------------------------------------------------------------------------
def test_the_bound_separates_double_from_float(pkg):
    """On the F = 5000 track of the GPU test's own grid (W = 80): float64 restatements of CMN and CMVN, one-pass and two-pass, summed in
    sequence (the reference sums pairwise), stay within a quarter of the bound; CMN with a float32 accumulator leaves it."""
    W, frames = 80, WIDTHS[80]
    cells = grid_cells(W, frames)
    t = frames.index(5000)
    x32 = cells[t]
    assert np.abs(x32).max() <= 20 and x32.astype(np.float64).var(axis=0).min() >= 0.25
    x = x32.astype(np.float64)
    F = len(x)
    worst = {}
    for norm in ("cmn", "cmvn"):
        fb = request_of(pkg, W, frames, 5003, norm, "value")
        ref = feat_batch_ref([x32], W, True, fb)[:, :F]
        bound = bound_of([x32], W, True, fb, ref)
        floor = float(fb.rec["var_floor"][0])
        s, q = np.cumsum(x, axis=0)[-1], np.cumsum(x * x, axis=0)[-1]
        mean = s / F
        d1 = np.sqrt(np.maximum(q / F - mean * mean, floor)) if norm == "cmvn" else 1.0
        d2 = np.sqrt(np.maximum(np.cumsum((x - mean) ** 2, axis=0)[-1] / F, floor)) if norm == "cmvn" else 1.0
        for form, d in (("one-pass", d1), ("two-pass", d2)):
            y = (x - mean) / d  # (kept in float64: the final rounding is the bound's first term, the sums are what is judged)
            worst[norm, form] = float((np.abs(y - ref[0]) / bound[0]).max())
            assert worst[norm, form] <= 0.25, (norm, form, worst)
        if norm == "cmn":
            acc = np.cumsum(x32, axis=0, dtype=np.float32)[-1]  # a float32 accumulator, frame after frame
            y = x32 - (acc / np.float32(F)).astype(np.float32)
            worst["cmn", "float32"] = float((np.abs(y.astype(np.float64) - ref[0]) / bound[0]).max())
    print(worst)
    assert worst["cmn", "float32"] > 1.0, worst
