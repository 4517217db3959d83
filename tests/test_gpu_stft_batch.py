"""STFT batches on the GPU (include/opusgpu.h STFT BATCHES: k_stft_stats, k_stft_fold, k_stft_batch, k_stft_pad,
opusgpu_tracks_stft_batch_device, and the whole-file STFT calls under opusgpu_set_stft_batch).  The stage alone on the synthetic
grids of tests/test_stft_batch.py, whose padding holds NaN, into a buffer of NaN between two guard lines: NONE, WHISPER, REFMAX and
AFFINE bit for bit against stft_batch_f32, CMN and CMVN within FEATURE BATCHES' bound (tests/test_feat_batch.py::bound_of, derived
there, not measured) of stft_batch_ref on every cell, and the same bits as opusgpu_tracks_feature_batch_device on the first 128
bins.  Through the files: the dense result -- by the direct path (norm NONE, a stride of a multiple of 64) and by the general one --
against stft_batch_f32 applied to the PACKED call's own result, bit for bit."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS as MS_LAYOUTS
from test_gpu_tracks_resample import stereo_files
from test_stft_batch import (CASES, CONSTANT, PAIR_NORMS, REAL_NORMS, VAR_FLOOR, bound_of, grid_cells, request_of, stft_batch_f32, stft_batch_ref,
                             strides_of)
from test_tracks_stft import stft_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32, NAN32 = 0x5A5A5A5A, 0x7FC12345
GUARD = 64  # floats of guard at either end: the tensor stays 128-byte aligned


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def packed_grid(pkg, cells, bins, c, frames_major):
    """The packed grid of TRACK STFT for these cells, NaN wherever no real cell lies -> (float32 grid, STFT_BATCH_SPAN_DTYPE spans)."""
    rng = np.random.default_rng(bins + c + frames_major)
    spans = np.zeros(len(cells), dtype=pkg.STFT_BATCH_SPAN_DTYPE)
    at = 0
    for t, x in enumerate(cells):
        plane = (len(x) + 63) // 64 * 64 + 64 * int(rng.integers(0, 2))
        spans[t] = (at, plane, len(x))
        at += bins * c * plane
    grid = np.full(at + 64, np.nan, dtype=np.float32)
    for sp, x in zip(spans, cells):
        F, o, plane = len(x), int(sp["grid_offset"]), int(sp["plane"])
        x = x.reshape(F, bins, c)
        if frames_major:
            grid[o:o + F * bins * c] = x.reshape(-1)
        else:
            grid[o:o + bins * plane * c].reshape(bins, plane, c)[:, :F] = x.transpose(1, 0, 2)
    return grid, spans


def run_into_guards(ctx, n_floats, call, runs=1):
    """call(d_tensor) into NaN words between two guard lines -> the tensor's words, once per run."""
    fill = np.full(n_floats + 2 * GUARD, NAN32, dtype=np.uint32)
    fill[:GUARD] = fill[len(fill) - GUARD:] = GUARD32
    d_out = ctx.dev_alloc(fill.nbytes)
    got = []
    try:
        for _ in range(runs):
            ctx.h2d(d_out, fill)
            call(d_out.value + 4 * GUARD)
            g = np.zeros_like(fill)
            ctx.d2h(g, d_out)
            assert (g[:GUARD] == GUARD32).all() and (g[len(g) - GUARD:] == GUARD32).all()  # nothing outside the tensor
            body = g[GUARD:len(g) - GUARD]
            assert not np.isnan(body.view(np.float32)).any()  # every element written
            got.append(body)
    finally:
        ctx.dev_free(d_out)
    return got


def run_stage(ctx, d_grid, spans, layout, sb, runs=1):
    n = len(spans)
    shape = ((n, sb.stride, sb.bins) if layout == "frames" else (n, sb.bins, sb.stride)) + ((2,) if sb.c == 2 else ())
    got = run_into_guards(ctx, n * sb.stride * sb.bins * sb.c, lambda d: ctx.tracks_stft_batch_device(spans, layout, sb, d_grid, d), runs)
    return [g.reshape(shape) for g in got]


def held_to(got, cells, bins, c, frames_major, sb, norm):
    """The tensor's words against the definition: bits for NONE, WHISPER, REFMAX and AFFINE, the bound for CMN and CMVN, every cell."""
    if norm not in ("cmn", "cmvn"):
        want = stft_batch_f32(cells, bins, c, frames_major, sb)
        assert got.shape == want.shape and np.array_equal(got, want.view(np.uint32)), norm
        return 0.0
    ref = stft_batch_ref(cells, bins, c, frames_major, sb)
    bound = bound_of(cells, bins, frames_major, sb, ref)
    err = np.abs(got.view(np.float32).astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"  {norm} bins {bins} {'frames' if frames_major else 'bands'} S {sb.stride}: worst error {worst:.3g} of the bound")
    assert (err <= bound).all(), (norm, worst)
    return worst


@pytest.mark.parametrize("layout", ["bands", "frames"])
@pytest.mark.parametrize("case", list(CASES))
def test_stage_alone(pkg, ctx, case, layout):
    """Every norm the case takes x two pad modes over one uploaded grid, the stride walking through strides_of: guards, no NaN left,
    the definition on every cell, a constant track exactly 0 under CMN and CMVN, a track without frames all pad (pad_value verbatim
    under REFMAX whatever the pad mode), two runs the same bits, and a track alone the same bits as among the others."""
    (bins, c), frames, frames_major = case, CASES[case], layout == "frames"
    cells = grid_cells(bins, c, frames)
    grid, spans = packed_grid(pkg, cells, bins, c, frames_major)
    d_grid = ctx.dev_alloc(grid.nbytes)
    strides = strides_of(frames)
    assert strides[1] * bins * c % 4 and strides[2] % 64 == 0  # track 1 starts inside a 16-byte piece under the odd stride
    try:
        ctx.h2d(d_grid, grid)
        for k, (norm, pad_mode) in enumerate(itertools.product(REAL_NORMS if c == 1 else PAIR_NORMS, ["value", "normalized"])):
            S = strides[(k + bins) % 3]
            sb = request_of(pkg, bins, c, frames, S, norm, pad_mode)
            first, second = run_stage(ctx, d_grid, spans, layout, sb, runs=2)
            assert np.array_equal(first, second), (norm, pad_mode)
            held_to(first, cells, bins, c, frames_major, sb, norm)
            f32 = first.view(np.float32)
            by_frame = f32 if frames_major else np.swapaxes(f32, 1, 2)  # [n, S, bins(, 2)]
            if norm in ("cmn", "cmvn"):
                assert (by_frame[-1, :frames[-1]] == 0).all() and (cells[-1] == CONSTANT).all()  # the constant track: exactly 0
            t0 = frames.index(0)
            if pad_mode == "value" or norm == "refmax":
                assert (by_frame[t0] == np.float32(-10.0)).all()
            if norm in ("refmax", "cmvn", "affine"):  # a track's cells do not depend on its neighbours
                t = frames.index(1025) if 1025 in frames else frames.index(65)
                alone = run_stage(ctx, d_grid, spans[t:t + 1], layout, sb)[0]
                assert np.array_equal(alone[0], first[t]), (norm, pad_mode)
        with pytest.raises(pkg.OpusGpuError):  # a stride below a track's frames, and (pairs) a norm they do not take: refused
            short = request_of(pkg, bins, c, [1], max(frames) - 1, "none", "value")
            ctx.tracks_stft_batch_device(spans, layout, short, d_grid, d_grid)
        if c == 2:
            bad = request_of(pkg, bins, 1, frames, max(frames), "cmn", "value")._replace(c=2)
            with pytest.raises(pkg.OpusGpuError):
                ctx.tracks_stft_batch_device(spans, layout, bad, d_grid, d_grid)
            assert b"pairs" in ctx.lib.opusgpu_last_error(ctx.h)
    finally:
        ctx.dev_free(d_grid)


@pytest.mark.parametrize("layout", ["bands", "frames"])
def test_first_128_bins_are_the_feature_stage(pkg, ctx, layout):
    """CMN and CMVN of the first 128 bins of the (257, 1) grid through opusgpu_tracks_feature_batch_device at width 128 -- bins-major
    over the same memory (the first 128 rows of every track), frames-major over a repacked slice -- equal the same rows of the wide
    stage bit for bit: a bin's statistics do not depend on `bins`."""
    bins, frames, frames_major = 257, CASES[(257, 1)], layout == "frames"
    cells = grid_cells(bins, 1, frames)
    grid, spans = packed_grid(pkg, cells, bins, 1, frames_major)
    narrow_grid, narrow_spans = (packed_grid(pkg, [np.ascontiguousarray(x[:, :128]) for x in cells], 128, 1, True) if frames_major
                                 else (grid, spans))
    fspans = np.zeros(len(frames), dtype=pkg.FEAT_SPAN_DTYPE)
    for f in fspans.dtype.names:
        fspans[f] = narrow_spans[f]
    d_grid, d_narrow = ctx.dev_alloc(grid.nbytes), ctx.dev_alloc(narrow_grid.nbytes)
    try:
        ctx.h2d(d_grid, grid)
        ctx.h2d(d_narrow, narrow_grid)
        for norm, S in (("cmn", strides_of(frames)[1]), ("cmvn", strides_of(frames)[2])):
            sb = request_of(pkg, bins, 1, frames, S, norm, "normalized")
            fb = pkg.feature_batch_request(frames, 128, S, {"cmn": "cmn", "cmvn": pkg.feature_norm("cmvn", var_floor=VAR_FLOOR)}[norm],
                                           (-10.0, "normalized"))
            wide = run_stage(ctx, d_grid, spans, layout, sb)[0]
            n = len(frames)
            narrow = run_into_guards(ctx, n * S * 128, lambda d: ctx.tracks_feature_batch_device(fspans, 128, layout, fb, d_narrow, d))[0]
            if frames_major:
                assert np.array_equal(narrow.reshape(n, S, 128), wide[:, :, :128]), norm
            else:
                assert np.array_equal(narrow.reshape(n, 128, S), wide[:, :128]), norm
    finally:
        ctx.dev_free(d_grid)
        ctx.dev_free(d_narrow)


# ---- through the files --------------------------------------------------------------------------------------
def cells_of(feats, rec):
    """A packed call's result as stft_batch_f32 takes it: float32 [F, bins] per track, [F, bins, 2] for pairs."""
    frames_major = int(rec["layout"][0]) == 1
    out = []
    for g in feats:
        g = np.ascontiguousarray(g if frames_major else g.T)
        out.append(g.view(np.float32).reshape(g.shape + (2,)) if np.iscomplexobj(g) else g)
    return out


def dense_equals(pkg, dense, dinfo, packed, pinfo, rec, sb):
    """A dense result against stft_batch_f32 of the packed call's own result, bit for bit; info as the packed call's but for
    feat_offset -> the real cells compared."""
    n, bins, c, frames_major = len(packed), sb.bins, sb.c, int(rec["layout"][0]) == 1
    for field in pinfo.dtype.names:
        if field != "feat_offset":
            assert np.array_equal(pinfo[field], dinfo[field]), field
    assert np.array_equal(dinfo["feat_offset"], np.arange(n) * sb.stride * bins * c)
    assert dense.dtype == (np.complex64 if c == 2 else np.float32) and dense.shape == ((n, sb.stride, bins) if frames_major else (n, bins, sb.stride))
    cells = cells_of(packed, rec)
    assert [len(x) for x in cells] == list(pinfo["frames"])
    want = stft_batch_f32(cells, bins, c, frames_major, sb)
    got = np.ascontiguousarray(dense).view(np.float32).reshape(want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return sum(x.size for x in cells)


def strides_for(planned_f):
    """A multiple of 64 (with norm NONE: the direct path) and an odd stride (the general path), both holding every planned track."""
    m = int(planned_f.max())
    return (m + 63) // 64 * 64, m + 1 + m % 2


@pytest.mark.parametrize("name,layout", [("tiny", "bands"), ("tiny", "frames"), ("enh", "bands"), ("enh", "frames")])
def test_files_dense(pkg, ctx, name, layout):
    """decode_files(features=rec, mono=True, stft_stride=S, ...) of the stereo corpus and the files whose frame fails equals the packed
    call of the same batch collated by stft_batch_f32, bit for bit: S a multiple of 64 with NONE (the direct path), an odd S (the
    general path) -- so both paths give the same tensor --, a pad value of its own, REFMAX on the real set and AFFINE on the pairs.
    A failed track has its shorter F and pad cells behind it.  The packed call with the request off is what it was before any
    request was set."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    rec = stft_of(pkg, name, layout)
    rate = int(rec["sample_rate"][0])
    planned_f = pkg.stft_frames(rec, -(-b.info["track_samples"] * rate // 48000))
    kw = dict(batch=b, features=rec, mono=True)
    packed, pinfo = ctx.decode_files(None, **kw)
    direct, odd = strides_for(planned_f)
    bins = int(rec["n_fft"][0]) // 2 + 1
    more = [dict(stft_stride=odd, stft_normalize="refmax", stft_pad=(-11.0, "normalized")), dict(stft_normalize="whisper")] if name == "tiny" else \
        [dict(stft_stride=odd, stft_normalize=("affine", np.linspace(-1, 1, bins), np.linspace(0.5, 2, bins)), stft_pad=(0.25, "normalized"))]
    for extra in [dict(stft_stride=direct), dict(stft_stride=odd), dict(stft_stride=direct, stft_pad=-3.5)] + more:
        req = pkg.files_request(b, features=rec, mono=True, **extra)
        dense, dinfo = ctx.decode_files(None, **kw, **extra)
        assert dense_equals(pkg, dense, dinfo, packed, pinfo, rec, req.stft_batch) > 10000, extra
        if extra == dict(stft_stride=direct):
            assert any(x is not None for x in bad)
            by_frame = dense if layout == "frames" else dense.transpose(0, 2, 1)
            for i, seq in enumerate(bad):
                if seq is not None:  # a failed track: its cells behind the shorter F are pad cells
                    F = int(dinfo["frames"][i])
                    assert F < planned_f[i] and dinfo["final_status"][i] == -18 and (by_frame[i, F:] == 0).all()
    again, ainfo = ctx.decode_files(None, **kw)  # the request is gone
    assert np.array_equal(ainfo, pinfo) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(again, packed))
    b.close()


def test_files_loudness_and_cuts(pkg, ctx):
    """A loudness target composes (its gain is in the kernel's scale), with resample= and scale=; and a packed batch of cuts is a
    batch like any other, on both paths."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)]
    rec = stft_of(pkg, "enh", "bands", power=2, log="log10", floor=1e-10)
    for cuts in (None, [(0, 0, None), (1, 100, 3000), (2, 960, 6000), (3, 0, 1), (1, 4000, 2500)]):
        n = len(files) if cuts is None else len(cuts)
        ctx.streams_alloc(n, 2)
        b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
        planned_f = pkg.stft_frames(rec, -(-b.info["track_samples"] // 3))
        kw = dict(batch=b, features=rec, resample=16000, mono=True)
        if cuts is None:
            kw.update(loudness=-23.0, scale=np.linspace(0.5, 2.0, n).astype(np.float32) / 32768)
        packed, pinfo = ctx.decode_files(None, **kw)
        for extra in (dict(stft_stride=strides_for(planned_f)[0]), dict(stft_normalize="refmax"), dict(stft_stride=strides_for(planned_f)[1])):
            req = pkg.files_request(**{k: v for k, v in kw.items() if k != "batch"}, batch=b, **extra)
            dense, dinfo = ctx.decode_files(None, **kw, **extra)
            assert dense_equals(pkg, dense, dinfo, packed, pinfo, rec, req.stft_batch) > (10000 if cuts is None else 1000)
        if cuts is None:
            assert (dinfo["gain"] != 1.0).any()
        else:
            assert np.array_equal(dinfo["cut_start"], b.cut_info["start"])
        b.close()


def test_surround_dense(pkg):
    """The 5.1 corpus through mix="mono" on a MultistreamContext, pairs: both paths equal the packed call collated, and the packed
    call is unchanged behind them."""
    layout = MS_LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    rec = stft_of(pkg, "enh", "frames")
    kw = dict(batch=b, features=rec, mix="mono")
    packed, pinfo = ms.decode_files(None, **kw)
    planned_f = pkg.stft_frames(rec, -(-b.info["track_samples"] // 3))
    for S in strides_for(planned_f):
        req = pkg.files_request(b, True, 0, features=rec, mix="mono", stft_stride=S)
        dense, dinfo = ms.decode_files(None, stft_stride=S, **kw)
        assert dense_equals(pkg, dense, dinfo, packed, pinfo, rec, req.stft_batch) > 5000
    again, ainfo = ms.decode_files(None, **kw)
    assert np.array_equal(ainfo, pinfo) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(again, packed))
    with pytest.raises(ValueError):
        ms.decode_files(None, stft_normalize="refmax", **kw)  # pairs
    b.close()
    ms.close()


def test_refusals_through_the_c_abi(pkg, ctx):
    """opusgpu_files_decode_stft with a real context, batch and buffer under a request whose stride is too small, whose norm pairs do
    not take or whose AFFINE vectors have another length: OPUSGPU_BAD_ARG, the buffer and the arrays as they were; a mel call ignores
    the request; with the request in order the call reports the dense offsets, and with it off the packed ones."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2)
    n, lib = b.n_files, ctx.lib
    enh, mel = stft_of(pkg, "enh"), pkg.mel_params(80, "bands")
    planned_f = int(pkg.stft_frames(enh, -(-b.info["track_samples"] // 3)).max())
    S = (planned_f + 63) // 64 * 64
    packed_offs, _, packed_total = pkg.stft_layout(b.info["track_samples"], 1, 3, enh)
    total = max(packed_total, n * S * 514, pkg.mel_layout(b.info["track_samples"], 80, "bands")[2])
    fill = np.full(total + 64, GUARD32, dtype=np.uint32)
    d_out = ctx.dev_alloc(fill.nbytes)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]
    tail = [a.ctypes.data for a in arrays]
    sub = np.ones(129, dtype=np.float32)

    def call():
        return lib.opusgpu_files_decode_stft(ctx.h, b.h, 16000, 0, 0, 1, None, enh.ctypes.data, None, d_out, *tail)

    def request(**kw):
        rec = pkg.stft_batch_request([planned_f], 257, 2, S).rec.copy()
        for k, v in kw.items():
            rec[k] = v
        return rec
    try:
        ctx.h2d(d_out, fill)
        for rec, vecs, why in ((request(stride_frames=planned_f - 1), (None, None, 0), b"stride_frames is below"),
                               (request(norm=pkg.STFT_NORM_REFMAX), (None, None, 0), b"pairs"),
                               (request(norm=pkg.FEAT_NORM_AFFINE), (sub.ctypes.data, sub.ctypes.data, 129), b"AFFINE")):
            assert lib.opusgpu_set_stft_batch(ctx.h, rec.ctypes.data, *vecs) == 0
            assert call() == pkg.OPUSGPU_BAD_ARG and why in lib.opusgpu_last_error(ctx.h)
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all() and all((a == -7).all() for a in arrays)
        assert lib.opusgpu_files_decode_mel(ctx.h, b.h, 1, None, mel.ctypes.data, None, d_out, *tail) == 0  # ignores the request
        assert np.array_equal(arrays[0], pkg.mel_layout(b.info["track_samples"], 80, "bands")[0])
        ok = request()
        assert lib.opusgpu_set_stft_batch(ctx.h, ok.ctypes.data, None, None, 0) == 0
        assert call() == 0 and np.array_equal(arrays[0], np.arange(n) * S * 514)
        assert lib.opusgpu_set_stft_batch(ctx.h, None, None, None, 0) == 0
        assert call() == 0 and np.array_equal(arrays[0], packed_offs)
    finally:
        lib.opusgpu_set_stft_batch(ctx.h, None, None, None, 0)
        ctx.dev_free(d_out)
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
FILL = 12345.5
for rec, dtype, norm in ((pkg.stft_spec(16000, 512, 128, 400, power=None), torch.complex64, None),
                         (pkg.stft_spec(16000, 512, 128, 400, power=2, log="log10", floor=1e-10, feature_layout="frames"), torch.float32, "refmax")):
    bins, c = 257, 2 if dtype == torch.complex64 else 1
    most = int(pkg.stft_frames(rec, -(-b.info["track_samples"] // 3)).max())
    for S in ((most + 63) // 64 * 64, most + 1 + most % 2):
        kw = dict(batch=b, features=rec, mono=True, stft_stride=S, stft_normalize=norm)
        want, winfo = ctx.decode_files(None, **kw)
        shape = (n, S, bins) if c == 1 else (n, bins, S)
        assert want.shape == shape
        floats = n * S * bins * c
        out = torch.full((floats + 256,), FILL, dtype=torch.float32, device="cuda:0")
        got, info = ctx.decode_files(None, out=out, **kw)
        assert np.array_equal(info, winfo)
        assert got.is_cuda and got.dtype == dtype and tuple(got.shape) == shape
        assert got.untyped_storage().data_ptr() == out.untyped_storage().data_ptr() and got.data_ptr() == out.data_ptr()  # a view of `out`
        assert np.array_equal(np.ascontiguousarray(got.cpu().numpy()).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
        assert bool((out[floats:] == FILL).all()) and not bool((out[:floats] == FILL).any())
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
    """decode_files(features=rec, stft_stride=S, out=tensor) on both paths: the result is a view of the caller's float32 tensor --
    complex64 [n, bins, S] over the pairs, float32 [n, S, bins] frames-major --, equal to the numpy route, the elements behind it as
    they were; a tensor that does not fit raises before any device work.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
