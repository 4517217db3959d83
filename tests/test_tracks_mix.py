"""The channel mix of the whole-file path (include/opusgpu.h, CHANNEL MIX), what needs no GPU: the exported symbols and the matrix
record, the default downmix tables and their generator, mix_ref by hand, the refusals that the C calls, track_mix_args and
decode_files raise before any device work, and the budget of the new kernels.  mix_ref is the numpy restatement of the header's
VALUE rule; every bit-for-bit check (tests/test_gpu_tracks_mix.py) compares against resample_ref(mix_ref(x, M), ...)."""
import os
import re
import sys

import numpy as np
import pytest

from test_kernel_budget import _kernel_metadata
from test_tracks_formats import Tensor
from test_tracks_resample import batch, handles, ms_batch, resample_ref  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_downmix_matrix", "opusgpu_tracks_resample_mixed_device", "opusgpu_files_decode_mixed", "opusgpu_ms_files_decode_mixed"]
ORDER = {1: "M", 2: "FL FR", 3: "FL C FR", 4: "FL FR RL RR", 5: "FL C FR RL RR", 6: "FL C FR RL RR LFE", 7: "FL C FR SL SR RC LFE",
         8: "FL C FR SL SR RL RR LFE"}
SWAP = {"FL": "FR", "FR": "FL", "SL": "SR", "SR": "SL", "RL": "RR", "RR": "RL"}


def mix_ref(x, M):
    """CHANNEL MIX, VALUE: x int16 [n, C], M int16 [CO, C] in Q14 -> int16 [n, CO]."""
    return np.clip((x.astype(np.int64) @ M.astype(np.int64).T + 8192) >> 14, -32768, 32767).astype(np.int16)


def record(pkg, M, out_channels=None, in_channels=None):
    """An opusgpu_mix_matrix with M's entries, and channel counts that need not be M's."""
    M = np.asarray(M, dtype=np.int16)
    rec = np.zeros(1, dtype=pkg.MIX_MATRIX_DTYPE)
    rec["out_channels"] = M.shape[0] if out_channels is None else out_channels
    rec["in_channels"] = M.shape[1] if in_channels is None else in_channels
    rec["m"][0, :M.shape[0], :M.shape[1]] = M
    return rec


def test_symbols_and_matrix_record(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert hdr.index("TRACK RATES.") < hdr.index("CHANNEL MIX.")
    d = pkg.MIX_MATRIX_DTYPE
    assert d.itemsize == 136 and "opusgpu_mix_matrix { /* 136 bytes" in hdr
    assert [(n, d.fields[n][1]) for n in d.names] == [("out_channels", 0), ("in_channels", 4), ("m", 8)] and d["m"].shape == (8, 8)


def test_tables_are_what_the_tool_generates(pkg):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_downmix_tables as g
    assert g.build_text() == open(os.path.join(ROOT, g.REL)).read()
    assert {k: v for k, v in g.ORDER.items()} == ORDER
    for ch in range(1, 9):
        for out in (1, 2):
            assert g.matrix(ch, out) == pkg.downmix_matrix(ch, out).tolist()


def test_default_tables(pkg):
    lib = pkg.load_lib()
    for ch in range(1, 9):
        names = ORDER[ch].split()
        for out in (1, 2):
            M = pkg.downmix_matrix(ch, out)
            assert M.dtype == np.int16 and M.shape == (out, ch)
            assert (M.astype(np.int64).sum(axis=1) == 16384).all() and (M >= 0).all(), (ch, out, M)
            if "LFE" in names:
                assert (M[:, names.index("LFE")] == 0).all()
            rec = np.full(1, -1, dtype=np.int8).repeat(136).view(pkg.MIX_MATRIX_DTYPE)  # unused entries come back 0
            assert lib.opusgpu_downmix_matrix(ch, out, rec.ctypes.data) == 0
            assert (rec["out_channels"][0], rec["in_channels"][0]) == (out, ch) and rec["m"][0].astype(np.int64).sum() == 16384 * out
        st = pkg.downmix_matrix(ch, 2)
        mirror = [names.index(SWAP.get(s, s)) for s in names]
        assert np.array_equal(st[0], st[1][mirror]), (ch, st)
        # the rule itself, restated: the stereo row before the correction
        w = {"FL": 1, "C": 2 ** -0.5, "M": 2 ** -0.5, "SL": 2 ** -0.5, "RL": 2 ** -0.5, "RC": 0.5}
        left = np.array([w.get(s, 0.0) for s in names])
        assert np.abs(st[0] - 16384 * left / left.sum()).max() <= 2.5, (ch, st[0])
    assert pkg.downmix_matrix(2, 1).tolist() == [[8192, 8192]]
    assert pkg.downmix_matrix(2, 2).tolist() == [[16384, 0], [0, 16384]]
    assert pkg.downmix_matrix(1, 1).tolist() == [[16384]]
    assert pkg.downmix_matrix(1, 2).tolist() == [[16384], [16384]]
    rec = np.zeros(1, dtype=pkg.MIX_MATRIX_DTYPE)
    for ch, out in ((0, 1), (9, 2), (6, 0), (6, 3), (-1, 1)):
        assert lib.opusgpu_downmix_matrix(ch, out, rec.ctypes.data) == pkg.OPUSGPU_BAD_ARG
        with pytest.raises(ValueError):
            pkg.downmix_matrix(ch, out)
    assert lib.opusgpu_downmix_matrix(6, 2, None) == pkg.OPUSGPU_BAD_ARG


def test_mix_ref_by_hand():
    lr = np.array([[1, 2], [-1, -2], [32767, 32767], [-32768, -32768], [-3, 0]], dtype=np.int16)
    assert list(mix_ref(lr, np.array([[8192, 8192]], dtype=np.int16))[:, 0]) == [2, -1, 32767, -32768, -1]
    assert np.array_equal(mix_ref(lr, np.array([[8192, 8192]], dtype=np.int16)), resample_ref(lr, 48000, mono=True))
    rng = np.random.default_rng(1)
    x = rng.integers(-32768, 32768, (500, 5), dtype=np.int16)
    x[:2] = [[32767] * 5, [-32768] * 5]
    assert np.array_equal(mix_ref(x, (16384 * np.eye(5)).astype(np.int16)), x)
    row = np.array([[32767, -32768]], dtype=np.int16)  # abs-sum 65535
    full = np.array([[32767, -32768], [-32768, 32767], [1, 0], [0, 1]], dtype=np.int16)
    # (32767 * 32767 + 32768 * 32768 + 8192) >> 14 = 131070 and (-2 * 32768 * 32767 + 8192) >> 14 = -131068: both clamp
    assert list(mix_ref(full, row)[:, 0]) == [32767, -32768, 2, -2]


def test_c_calls_refuse_before_device_work(pkg, batch, ms_batch, handles):
    """Every refusal of the three calls comes back as OPUSGPU_BAD_ARG with d_in / d_out NULL, from real decoders where there is
    a device and from zeroed memory where there is none (test_tracks_resample.py::handles)."""
    lib = pkg.load_lib()
    S16, F32, PL = pkg.TRACKS_S16, pkg.TRACKS_F32, pkg.TRACKS_F32_PLANAR
    BAD = pkg.OPUSGPU_BAD_ARG
    fake, fake_ms = handles
    n = batch.n_files
    one = np.ones(n, dtype=np.float32)
    nan = np.array([1, np.nan] + [1] * (n - 2), dtype=np.float32)
    ok2, ok6 = record(pkg, [[8192, 8192]]), record(pkg, pkg.downmix_matrix(6, 2))
    over2 = record(pkg, [[16384, 0], [32767, -32768], [0, 1]])
    over2["m"][0, 1, 0] = -32768  # a row of abs-sum 65536
    over6 = record(pkg, [[10923, -10923, 10923, -10923, 10923, -10921]])
    assert np.abs(over6["m"][0, 0].astype(int)).sum() == 65536

    def bad_records(ok, over, C):
        return [over, record(pkg, ok["m"][0, :1, :C], out_channels=0), record(pkg, ok["m"][0, :1, :C], out_channels=9),
                record(pkg, ok["m"][0, :1, :C - 1]), record(pkg, ok["m"][0, :1, :C], in_channels=C + 1),
                record(pkg, ok["m"][0, :1, :C], in_channels=0), record(pkg, ok["m"][0, :1, :C], in_channels=9)]

    def files(rate, mix, fmt, scale):
        return lib.opusgpu_files_decode_mixed(fake, batch.h, rate, None if mix is None else mix.ctypes.data, fmt,
                                              None if scale is None else scale.ctypes.data, None, None, None, None, None)

    def ms_files(rate, mix, fmt, scale):
        return lib.opusgpu_ms_files_decode_mixed(fake_ms, ms_batch.h, rate, None if mix is None else mix.ctypes.data, fmt,
                                                 None if scale is None else scale.ctypes.data, None, None, None, None, None)
    assert lib.opusgpu_files_decode_mixed(None, batch.h, 16000, ok2.ctypes.data, S16, None, None, None, None, None, None) == BAD
    assert lib.opusgpu_files_decode_mixed(fake, None, 16000, ok2.ctypes.data, S16, None, None, None, None, None, None) == BAD
    assert lib.opusgpu_ms_files_decode_mixed(None, ms_batch.h, 16000, ok6.ctypes.data, S16, None, None, None, None, None, None) == BAD
    assert lib.opusgpu_ms_files_decode_mixed(fake_ms, None, 16000, ok6.ctypes.data, S16, None, None, None, None, None, None) == BAD
    for call, ok, over, C in ((files, ok2, over2, 2), (ms_files, ok6, over6, 6)):
        assert call(16000, None, S16, None) == BAD
        for rec in bad_records(ok, over, C):
            assert call(16000, rec, S16, None) == BAD, (C, rec)
        for rate, fmt, scale in ((44100, S16, None), (0, F32, None), (16000, 3, None), (48000, -1, None),  # unknown rates and formats
                                 (16000, S16, one), (48000, S16, one),                                      # a scale with S16
                                 (24000, F32, nan), (48000, PL, nan)):                                      # a scale that is not finite
            assert call(rate, ok, fmt, scale) == BAD, (C, rate, fmt)

    spans = np.zeros(2, dtype=pkg.RESAMPLE_SPAN_DTYPE)
    spans["in_samples"], spans["scale"], spans["out_plane"] = 100, 1.0, 128
    spans["in_offset"], spans["out_offset"] = [0, 128], [0, 128]

    def kernel(s, channels, rate, mix, fmt, ctx=fake):
        return lib.opusgpu_tracks_resample_mixed_device(ctx, len(s), s.ctypes.data, None, channels, rate, None if mix is None else mix.ctypes.data,
                                                        fmt, None, None)
    assert kernel(spans, 2, 16000, ok2, S16, ctx=None) == BAD and kernel(spans, 2, 16000, None, S16) == BAD
    for rec in bad_records(ok2, over2, 2):
        assert kernel(spans, 2, 16000, rec, S16) == BAD
    assert kernel(spans, 6, 16000, ok2, S16) == BAD and kernel(spans, 2, 16000, ok6, S16) == BAD  # in_channels is not the tracks'
    for rate, fmt in ((44100, S16), (0, F32), (16000, 3)):
        assert kernel(spans, 2, rate, ok2, fmt) == BAD
    bad_span = spans.copy()
    bad_span["in_offset"][1] = 4
    assert kernel(bad_span, 2, 16000, ok2, S16) == BAD
    for rate in (16000, 48000):  # in order: refused for the NULL buffers, still before the device
        assert kernel(spans, 2, rate, ok2, PL) == BAD and kernel(spans, 6, rate, ok6, S16) == BAD
    empty = spans.copy()
    empty["in_samples"] = 0
    assert kernel(empty, 2, 48000, ok2, S16) == 0 and kernel(spans[:0], 6, 16000, ok6, F32) == 0  # nothing to do is no error


def test_python_refusals_need_no_device(pkg, batch):
    """mix_matrix, track_mix_args, and decode_files raising before it touches its decoder (an object without one is enough)."""
    D, ch, offs, total, out, rec = pkg.track_mix_args(batch, "mono", 16000, "f32")
    assert (D, ch, out) == (3, 1, None) and total == pkg.resample_layout(batch.info["track_samples"], 16000)[1]
    assert rec.dtype == pkg.MIX_MATRIX_DTYPE and rec["m"][0, 0, :2].tolist() == [8192, 8192] and len(offs) == batch.n_files
    assert pkg.track_mix_args(batch, "stereo")[:2] == (1, 2) and pkg.track_mix_args(batch, [[1.0, 0.0]], 24000)[:2] == (2, 1)
    assert pkg.mix_matrix([[0.5, -0.5], [1.99995, 0]], 2)["m"][0, :2, :2].tolist() == [[8192, -8192], [32767, 0]]
    assert pkg.mix_matrix(np.array([[3, -4]], dtype=np.int64), 2)["m"][0, 0, :2].tolist() == [3, -4]  # integers are Q14 as they are
    six = type("B", (), {"channels": 6, "info": batch.info, "n_files": batch.n_files, "track_samples": batch.track_samples})()
    assert pkg.track_mix_args(six, "stereo", 16000)[:2] == (3, 2) and pkg.track_mix_args(six, np.eye(6), 8000)[:2] == (6, 6)
    for mix in ("Stereo", "sterio", "", [[2.0, 0.0]], [[0.0, -2.001]], [[np.nan, 0.0]], [8192, 8192], np.zeros((1, 3)), np.zeros((0, 2)),
                np.zeros((9, 2)), np.zeros((2, 2, 2)), [[40000, 0]], [[32767, -32768], [-32768, -32768]], [["a", "b"]], None):
        with pytest.raises(ValueError):
            pkg.track_mix_args(batch, mix, 16000)
    with pytest.raises(ValueError):
        pkg.track_mix_args(six, np.eye(2), 16000)
    for kw in (dict(rate=44100), dict(rate=0), dict(rate=16000, format="f64")):
        with pytest.raises(ValueError):
            pkg.track_mix_args(batch, "mono", **kw)
    # `out` is held against the MIXED size
    assert pkg.track_mix_args(batch, "mono", 16000, "f32", Tensor(total), 0)[4] is not None
    assert pkg.track_mix_args(batch, "stereo", 16000, "f32", Tensor(2 * total), 0)[4] is not None
    assert pkg.track_mix_args(six, "stereo", 16000, "f32", Tensor(2 * total), 0)[4] is not None  # two channels, not six
    for b, mix, t, fmt in ((batch, "mono", Tensor(total - 1), "f32"), (batch, "stereo", Tensor(2 * total - 1), "f32"),
                           (six, "stereo", Tensor(2 * total - 1), "f32"), (batch, np.ones((3, 2)), Tensor(3 * total - 1), "f32"),
                           (batch, "mono", Tensor(total), "s16"), (batch, "mono", Tensor(total, ptr=4096 + 64), "f32")):
        with pytest.raises(ValueError):
            pkg.track_mix_args(b, mix, 16000, fmt, t, 0)
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    for kw in (dict(mix="mono", mono=True), dict(mix="mono", rate=16000, mono=True), dict(mix=[[2.0, 0.0]]), dict(mix=np.zeros((1, 3))),
               dict(mix="sterio"), dict(mix="mono", rate=44100), dict(mix="mono", rate=16000, format="f32", out=Tensor(total - 1)),
               dict(mix="mono", format="s16", scale=np.ones(batch.n_files)), dict(mix="mono", format="f32", scale=[np.nan] * batch.n_files)):
        with pytest.raises(ValueError):
            ctx.decode_files(None, batch=batch, **kw)
    ms = pkg.MultistreamContext.__new__(pkg.MultistreamContext)
    ms.h, ms.device = None, 0
    for kw in (dict(mix="sterio"), dict(mix=np.eye(2)), dict(mix="stereo", rate=44100),
               dict(mix="stereo", rate=16000, format="f32", out=Tensor(2 * total - 1)), dict(mix="mono", scale=np.ones(batch.n_files))):
        with pytest.raises(ValueError):
            ms.decode_files(None, batch=six, **kw)
    with pytest.raises(TypeError):
        ms.decode_files(None, batch=six, mix="mono", mono=True)  # there is still no such argument


def test_mix_kernels_keep_out_of_scratch():
    """k_tracks_resample_mix<D>, every D: no scratch, no static LDS, at most 128 vector registers -- with eight staging bodies
    inlined, whose 4 C words are indexed by literals only; the matrix is indexed with the output channel, in the kernel's
    arguments, and must not be copied to scratch for it."""
    meta = _kernel_metadata()
    seen = {}
    for mangled, (vgpr, scratch, lds) in meta.items():
        m = re.search(r"\d+k_tracks_resample_mixILi(\d+)E", mangled)
        if m:
            seen[int(m.group(1))] = (vgpr, scratch, lds)
    print(seen)
    assert sorted(seen) == [1, 2, 3, 4, 6], sorted(meta)[:6]
    assert all(v[0] <= 128 and v[1] == 0 and v[2] == 0 for v in seen.values()), seen
