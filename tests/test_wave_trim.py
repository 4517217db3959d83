"""Wave trim of the whole-file path (include/opusgpu.h, WAVE TRIM), what needs no GPU: the reference that
tests/test_gpu_wave_trim.py holds the kernels to, held itself against a naive restatement and against librosa's float formula;
the exported symbols and the records; every refusal of opusgpu_set_wave_trim; trim_spec and activity_intervals; what files_request
makes of wave_trim=; the kernels' resources.

Everything in the definition is an integer but the REL threshold, floor((double)Emax * ratio): one float64 product, which Python's
float reproduces bit for bit, so wave_trim_ref is exact and the kernels must equal it field for field."""
import math
import os
import re

import numpy as np
import pytest

from test_kernel_budget import _kernel_metadata
from test_tracks_resample import batch, handles, ms_batch  # noqa: F401 (fixtures)
from test_wave_batch import good_request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_set_wave_trim", "opusgpu_ms_set_wave_trim", "opusgpu_last_wave_trim", "opusgpu_ms_last_wave_trim",
       "opusgpu_last_wave_trim_flags", "opusgpu_ms_last_wave_trim_flags", "opusgpu_tracks_wave_trim_device"]
REL, ABS = 0, 1
STAT_FIELDS = ("start", "count", "full", "emax", "thr", "frames", "first", "last", "active")


# ---- the reference ------------------------------------------------------------------------------------------
def frame_energies(y, C, fl, hop):
    """M[f] of one track, y int16 [L, C] (any shape of L * C elements): Python integers, from exact int64 running sums."""
    y = np.asarray(y, dtype=np.int16).reshape(-1, C).astype(np.int64)
    L = len(y)
    run = np.concatenate([np.zeros((1, C), dtype=np.int64), np.cumsum(y * y, axis=0)])  # below 2^63 for L < 2^33
    f = np.arange(1 + L // hop, dtype=np.int64)
    lo, hi = np.clip(f * hop - fl // 2, 0, L), np.clip(f * hop + fl // 2, 0, L)
    return [int(v) for v in (run[hi] - run[lo]).max(axis=1)]


def threshold_of(emax, req):
    """thr of the definition for a trim_spec() record."""
    if int(req["mode"][0]) == ABS:
        return int(req["threshold"][0])
    return int(math.floor(float(emax) * float(req["ratio"][0])))  # (double)Emax is exact; one rounding; an exact floor


def record_of(M, L, req):
    """The record and the flags of one track from its frame energies."""
    hop, margin = int(req["hop"][0]), int(req["margin"][0])
    emax = max(M)
    thr = threshold_of(emax, req)
    flags = np.array([1 if m > thr else 0 for m in M], dtype=np.uint8)
    on = np.flatnonzero(flags)
    rec = dict(start=0, count=0, full=L, emax=emax, thr=thr, frames=len(M), first=-1, last=-1, active=len(on))
    if len(on):
        first, last = int(on[0]), int(on[-1])
        start, end = max(0, first * hop - margin), min(L, (last + 1) * hop + margin)
        rec.update(start=start, count=end - start, first=first, last=last)
    return rec, flags


def wave_trim_ref(tracks, C, req):
    """WAVE TRIM as a function of the int16 tracks (tracks[t] int16 [L[t], C]) and a trim_spec() record -> (a list of records as
    dicts of Python integers, a list of uint8 flag arrays)."""
    fl, hop = int(req["frame_length"][0]), int(req["hop"][0])
    out = [record_of(frame_energies(y, C, fl, hop), np.asarray(y).size // C, req) for y in tracks]
    return [r for r, _ in out], [f for _, f in out]


def records_held(got, want):
    """The records of a call against the reference's: every field exactly, the reserved words 0."""
    assert len(got) == len(want)
    for t, w in enumerate(want):
        for f in STAT_FIELDS:
            assert int(got[t][f]) == w[f], (t, f, int(got[t][f]), w[f])
        assert (np.asarray(got[t]["reserved"]) == 0).all()


def naive_trim(y, C, req):
    """The definition read aloud: a loop over frames, channels and samples."""
    y = np.asarray(y, dtype=np.int16).reshape(-1, C)
    L, fl, hop = len(y), int(req["frame_length"][0]), int(req["hop"][0])
    M = []
    for f in range(1 + L // hop):
        best = 0
        for c in range(C):
            e = 0
            for m in range(f * hop - fl // 2, f * hop + fl // 2):
                if 0 <= m < L:
                    e += int(y[m, c]) ** 2
            best = max(best, e)
        M.append(best)
    return record_of(M, L, req)


def random_tracks(rng, C, count, longest):
    """Short tracks of quiet and loud stretches, so that thresholds cut them somewhere."""
    tracks = []
    for _ in range(count):
        L = int(rng.integers(0, longest))
        amp = np.repeat(rng.choice([0, 3, 40, 2000, 32767], size=L // 16 + 1), 16)[:L]
        y = (rng.uniform(-1, 1, (L, C)) * amp[:, None]).round().astype(np.int16)
        tracks.append(y)
    return tracks


def test_the_reference_against_the_naive_loop(pkg):
    rng = np.random.default_rng(60)
    checked = 0
    for C, fl, hop, margin in ((1, 16, 8, 0), (2, 48, 16, 8), (3, 64, 64, 24), (1, 32, 24, 0)):
        tracks = random_tracks(rng, C, 10, 200)
        for req in (pkg.trim_spec(20.0, fl, hop, margin=margin), pkg.trim_spec(30.0, fl, hop, ref=-10.0, margin=margin),
                    pkg.trim_spec(0.0, fl, hop)):
            recs, flags = wave_trim_ref(tracks, C, req)
            for t, y in enumerate(tracks):
                rec, fl_naive = naive_trim(y, C, req)
                assert rec == recs[t] and np.array_equal(fl_naive, flags[t]), (C, fl, hop, t)
                checked += 1
    assert checked == 120


def test_the_reference_against_the_float_formula(pkg):
    """librosa.effects.trim on float copies x = y / 32768: mse = mean over the padded frame of x^2, the maximum over the channels,
    active where 10 log10(mse / max mse) > -top_db.  No frame may lie within 1e-6 relative of the threshold -- asserted, so that the
    comparison cannot pass by skipping --, and then both say the same of every frame."""
    rng = np.random.default_rng(61)
    frames = 0
    for C, fl, hop, top_db in ((1, 64, 16, 30.0), (2, 128, 32, 40.0), (1, 2048, 512, 60.0)):
        req = pkg.trim_spec(top_db, fl, hop)
        for y in random_tracks(rng, C, 12, 40 * hop):
            if not len(y) or not np.any(y):
                continue
            M = frame_energies(y, C, fl, hop)
            rec, flags = record_of(M, len(y), req)
            edge = max(M) * float(req["ratio"][0])
            assert all(abs(m - edge) > 1e-6 * edge for m in M)
            x = np.concatenate([np.zeros((fl // 2, C)), y.astype(np.float64) / 32768, np.zeros((fl // 2, C))])
            mse = np.array([(x[f * hop:f * hop + fl] ** 2).mean(axis=0).max() for f in range(1 + len(y) // hop)])
            with np.errstate(divide="ignore"):
                db = 10 * np.log10(mse / mse.max())
            assert np.array_equal(db > -top_db, flags.astype(bool))
            on = np.flatnonzero(db > -top_db)  # librosa's indices
            assert (rec["start"], rec["start"] + rec["count"]) == (on[0] * hop, min(len(y), (on[-1] + 1) * hop))
            frames += len(M)
    assert frames > 400


# ---- ABI, records and refusals ------------------------------------------------------------------------------
def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    missing = [s for s in NEW if not hasattr(lib, s)]
    assert not missing, missing
    assert all(s in pkg.EXPORTS for s in NEW)
    req, stat = pkg.WAVE_TRIM_REQ_DTYPE, pkg.WAVE_TRIM_STAT_DTYPE
    assert (req.itemsize, stat.itemsize) == (64, 64)
    assert [req.fields[f][1] for f in ("ratio", "threshold", "enabled", "mode", "frame_length", "hop", "margin", "flags", "reserved")] == \
        [0, 8, 16, 20, 24, 28, 32, 36, 40]
    assert [stat.fields[f][1] for f in STAT_FIELDS + ("reserved",)] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56]
    header = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    assert all(re.search(r"\b%s\(" % s, header) for s in NEW)
    assert header.index("WAVE BATCHES.") < header.index("WAVE TRIM.") < header.index("STFT BATCHES.")
    assert re.search(r"#define OPUSGPU_WAVE_TRIM_REL 0\b", header) and re.search(r"#define OPUSGPU_WAVE_TRIM_ABS 1\b", header)
    assert (pkg.WAVE_TRIM_REL, pkg.WAVE_TRIM_ABS) == (REL, ABS)
    # the C struct has the dtype's fields in the dtype's order
    body = re.search(r"typedef struct opusgpu_wave_trim_req \{(.*?)\} opusgpu_wave_trim_req;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", body) == list(req.names)
    body = re.search(r"typedef struct opusgpu_wave_trim_stat \{(.*?)\} opusgpu_wave_trim_stat;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d+\])?[,;]", body) == list(stat.names)


def spec_but(pkg, **kw):
    rec = pkg.trim_spec().copy()
    for k, v in kw.items():
        rec[k] = v
    return rec


def test_set_time_refusals(pkg, handles):
    lib = pkg.load_lib()
    BAD = pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_set_wave_trim(None, None) == BAD and lib.opusgpu_ms_set_wave_trim(None, None) == BAD
    assert lib.opusgpu_last_wave_trim(None, 0, None) == BAD and lib.opusgpu_ms_last_wave_trim(None, 0, None) == BAD
    assert lib.opusgpu_last_wave_trim_flags(None, 0, None) == BAD and lib.opusgpu_ms_last_wave_trim_flags(None, 0, None) == BAD
    for prefix, h in zip(("opusgpu_", "opusgpu_ms_"), handles):
        fn, batch_fn, err = (getattr(lib, prefix + s) for s in ("set_wave_trim", "set_wave_batch", "last_error"))
        try:
            assert batch_fn(h, good_request(pkg).ctypes.data) == 0
            for kw, why in ((dict(frame_length=2040), b"frame_length"), (dict(frame_length=0), b"frame_length"),
                            (dict(frame_length=8208), b"frame_length"), (dict(frame_length=8), b"frame_length"),
                            (dict(hop=516), b"hop"), (dict(hop=0), b"hop"), (dict(hop=-8), b"hop"), (dict(hop=2056), b"hop"),
                            (dict(frame_length=16, hop=24), b"hop"), (dict(margin=4), b"margin"), (dict(margin=-8), b"margin"),
                            (dict(ratio=0.0), b"ratio"), (dict(ratio=-0.5), b"ratio"), (dict(ratio=1.0000001), b"ratio"),
                            (dict(ratio=np.nan), b"ratio"), (dict(ratio=np.inf), b"ratio"), (dict(mode=ABS, ratio=np.nan), b"ratio"),
                            (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"), (dict(flags=2), b"flags"),
                            (dict(reserved=[0, 0, 0, 0, 0, 1]), b"reserved"), (dict(reserved=[1, 0, 0, 0, 0, 0]), b"reserved")):
                assert fn(h, spec_but(pkg, **kw).ctypes.data) == BAD, kw
                assert why in err(h), (kw, err(h))
            for kw in (dict(), dict(ratio=1.0), dict(mode=ABS, ratio=7.5, threshold=2 ** 63), dict(frame_length=16, hop=8),
                       dict(frame_length=8192, hop=8192, margin=8000), dict(flags=1)):
                assert fn(h, spec_but(pkg, **kw).ctypes.data) == 0, kw
            assert fn(h, spec_but(pkg, enabled=0, mode=99, hop=3).ctypes.data) == 0  # off: nothing of it is read
            assert fn(h, None) == 0
            # on without a wave batch: refused, with the reason
            assert batch_fn(h, None) == 0
            assert fn(h, pkg.trim_spec().ctypes.data) == BAD and b"without a wave-batch request" in err(h)
            assert fn(h, None) == 0
        finally:
            fn(h, None)
            batch_fn(h, None)


def test_a_trim_whose_wave_batch_was_cleared_is_refused_before_device_work(pkg, batch, ms_batch, handles):
    lib = pkg.load_lib()
    for b, prefix, h, mono in ((batch, "opusgpu_", handles[0], (0,)), (ms_batch, "opusgpu_ms_", handles[1], ())):
        fn, batch_fn, err = (getattr(lib, prefix + s) for s in ("set_wave_trim", "set_wave_batch", "last_error"))
        arrays = [np.full(b.n_files, -7, dtype=np.int64) for _ in range(3)] + [np.full((b.n_files, 2), -7, dtype=np.int32)]
        tail = [None] + [a.ctypes.data for a in arrays]
        try:
            assert batch_fn(h, good_request(pkg, stride_samples=1 << 20).ctypes.data) == 0 and fn(h, pkg.trim_spec().ctypes.data) == 0
            assert batch_fn(h, None) == 0
            rc = getattr(lib, prefix + "files_decode_resampled")(h, b.h, 16000, *mono, pkg.TRACKS_F32, None, *tail)
            assert rc == pkg.OPUSGPU_BAD_ARG and b"without a wave-batch request" in err(h)
        finally:
            fn(h, None)
            batch_fn(h, None)
        assert all((a == -7).all() for a in arrays)


def test_the_stand_alone_call_refuses_before_device_work(pkg, handles):
    lib = pkg.load_lib()
    h = handles[0]
    spans = np.zeros(2, dtype=pkg.WAVE_SPAN_DTYPE)
    spans["in_offset"], spans["samples"], spans["scale"] = [0, 16], [10, 5], 1.0
    stats = np.zeros(2, dtype=pkg.WAVE_TRIM_STAT_DTYPE)

    def call(s=spans, ch=1, r=pkg.trim_spec(), out=stats, handle=h):
        return lib.opusgpu_tracks_wave_trim_device(handle, len(s), s.ctypes.data, ch, r.ctypes.data, None, out.ctypes.data if out is not None else None,
                                                   None, None)

    def but(**kw):
        s = spans.copy()
        for k, v in kw.items():
            s[k][1] = v
        return s
    BAD = pkg.OPUSGPU_BAD_ARG
    assert call(handle=None) == BAD
    assert call() == BAD and b"NULL" in lib.opusgpu_last_error(h)  # in order but for the tracks
    assert call(out=None) == BAD and b"no records" in lib.opusgpu_last_error(h)
    for s in (but(in_offset=4), but(in_offset=-8), but(samples=-1), but(reserved=1)):
        assert call(s) == BAD and b"span" in lib.opusgpu_last_error(h)
    assert call(but(samples=1 << 30), ch=3) == BAD and b"0x7fffffff" in lib.opusgpu_last_error(h)
    for kw in (dict(ch=0), dict(ch=9), dict(r=spec_but(pkg, hop=12)), dict(r=spec_but(pkg, ratio=2.0)), dict(r=spec_but(pkg, mode=5))):
        assert call(**kw) == BAD, kw
    assert call(spans[:0]) == 0  # nothing to do is no error
    assert (stats.view(np.uint8) == 0).all()


# ---- trim_spec, activity_intervals, files_request -------------------------------------------------------------
def test_trim_spec(pkg):
    rec = pkg.trim_spec()
    assert rec.dtype == pkg.WAVE_TRIM_REQ_DTYPE and rec.shape == (1,)
    assert (int(rec["enabled"][0]), int(rec["mode"][0]), int(rec["frame_length"][0]), int(rec["hop"][0]), int(rec["margin"][0]),
            int(rec["flags"][0])) == (1, REL, 2048, 512, 0, 0)
    assert float(rec["ratio"][0]) == 10.0 ** -6.0 and (rec["reserved"] == 0).all()
    assert float(pkg.trim_spec(0)["ratio"][0]) == 1.0 and float(pkg.trim_spec(25.5)["ratio"][0]) == 10.0 ** -2.55
    rec = pkg.trim_spec(40.0, 400, 160, ref=-3.0, margin=24, flags=True)
    assert (int(rec["mode"][0]), int(rec["frame_length"][0]), int(rec["hop"][0]), int(rec["margin"][0]), int(rec["flags"][0])) == (ABS, 400, 160, 24, 1)
    assert int(rec["threshold"][0]) == math.floor(400 * 2.0 ** 30 * 10.0 ** (-43.0 / 10)) and float(rec["ratio"][0]) == 1.0
    assert int(pkg.trim_spec(0.0, 16, 8, ref=0.0)["threshold"][0]) == 16 << 30  # full scale at 0 dBFS
    for kw in (dict(frame_length=2040), dict(frame_length=8), dict(frame_length=16384), dict(frame_length=2048.0), dict(frame_length=True),
               dict(hop_length=100), dict(hop_length=0), dict(hop_length=4096), dict(hop_length=512.0), dict(margin=4), dict(margin=-8),
               dict(margin=1.5), dict(top_db=-1.0), dict(top_db=np.nan), dict(top_db=np.inf), dict(top_db="60"), dict(top_db=4000.0),
               dict(ref="peak"), dict(ref=np.nan), dict(ref=None), dict(ref=200.0, top_db=0.0), dict(flags=1), dict(flags="yes")):
        with pytest.raises(ValueError):
            pkg.trim_spec(**kw)
    assert np.array_equal(pkg.wave_trim_frames([0, 511, 512, 1025], 512), [1, 1, 2, 3])


def test_activity_intervals(pkg):
    iv = pkg.activity_intervals
    assert iv([], 8, 0).shape == (0, 2) and iv([0, 0, 0], 8, 20).shape == (0, 2)
    assert iv([1], 8, 5).tolist() == [[0, 5]]
    assert iv([0, 1, 1, 0, 0, 1, 0], 16, 100).tolist() == [[16, 48], [80, 96]]
    assert iv([1, 1, 0, 1], 16, 50).tolist() == [[0, 32], [48, 50]]  # cut at the length
    assert iv(np.array([0, 0, 1], dtype=np.uint8), 512, 1024).tolist() == []  # a frame that begins at the length holds no sample
    assert iv([1, 0, 1, 0, 1], 8, 1000).tolist() == [[0, 8], [16, 24], [32, 40]] and iv([0, 1], 8, 9).dtype == np.int64


def test_the_new_keyword(pkg, batch, ms_batch):
    planned = batch.info["track_samples"]
    L16 = -(-planned // 3)
    base = dict(rate=16000, mono=True, format="f32")
    spec = pkg.trim_spec(40.0, 400, 160, margin=8, flags=True)
    plain = pkg.files_request(batch, wave_normalize="zmuv", wave_mask=True, **base)
    req = pkg.files_request(batch, wave_normalize="zmuv", wave_mask=True, wave_trim=spec, **base)
    assert plain.wave_trim is None and req.wave_trim is not spec and np.array_equal(req.wave_trim, spec)
    for f in req._fields:  # nothing else moves: the stride still holds the planned, untrimmed lengths
        if f not in ("wave_trim", "wave_batch"):
            x, y = getattr(req, f), getattr(plain, f)
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, f
    assert np.array_equal(req.wave_batch.rec, plain.wave_batch.rec) and req.wave_batch[1:] == plain.wave_batch[1:]
    # alone it is a wave keyword: the dense tensor with the others' defaults
    alone = pkg.files_request(batch, wave_trim=pkg.trim_spec(), **base)
    wb = alone.wave_batch
    assert (wb.stride, wb.mask, int(wb.rec["norm"][0])) == (int(L16.max()), False, pkg.WAVE_NORM_NONE) and alone.total == batch.n_files * wb.stride
    ms = pkg.files_request(ms_batch, True, 0, mix="stereo", rate=16000, format="f32_planar", wave_trim=spec, loudness=-23.0)
    assert (ms.entry, ms.channels) == ("files_decode_mixed", 2) and np.array_equal(ms.wave_trim, spec) and ms.loudness is not None
    assert pkg.files_request(batch, wave_trim=None, **base).wave_batch is None
    off = spec.copy()
    off["enabled"] = 0
    for kw in (dict(base, wave_trim=60.0), dict(base, wave_trim=True), dict(base, wave_trim=off), dict(base, wave_trim=np.concatenate([spec, spec])),
               dict(base, wave_trim=good_request(pkg)), dict(base, features="logmel", wave_trim=spec),
               dict(rate=16000, mono=True, wave_trim=spec), dict(rate=16000, mono=True, format="s16", wave_trim=spec),
               dict(base, wave_trim=spec, wave_stride=int(L16.max()) - 1)):
        with pytest.raises(ValueError):
            pkg.files_request(batch, **kw)


# ---- kernels ------------------------------------------------------------------------------------------------
def test_kernel_resources():
    """k_wave_trim_energy for 1 - 8 channels and k_wave_trim_fold: no scratch, registers for 8 waves per SIMD, no static LDS -- the
    energy kernel's is sized at the launch, at most WTRIM_LDS_CELLS cells of 8 bytes, the 64 KB its header states."""
    meta = _kernel_metadata()
    energy = {int(m.group(1)): v for name, v in meta.items() for m in [re.search(r"\d+k_wave_trim_energyILi(\d)EE", name)] if m}
    fold = [v for name, v in meta.items() if re.search(r"\d+k_wave_trim_fold(P|E|v|$)", name)]
    print(energy, fold)
    assert sorted(energy) == list(range(1, 9)) and len(fold) == 1
    for vgpr, scratch, lds in list(energy.values()) + fold:
        assert scratch == 0 and lds == 0 and vgpr <= 64
    source = open(os.path.join(ROOT, "esp32-opus-player_amd", "csrc", "og_wave_trim.hpp")).read()
    cells, tile = (int(re.search(r"constexpr int %s = (\d+);" % name, source).group(1)) for name in ("WTRIM_LDS_CELLS", "WTRIM_TILE"))
    assert cells * 8 <= 65536 and "64 KB" in source  # what a launch may ask for without opting in
    assert cells >= 8192 / 8 * 8 and tile % 8 == 0  # a frame of 8192 samples in granules of 8, eight channels
