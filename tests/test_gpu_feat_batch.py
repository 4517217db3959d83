"""Feature batches on the GPU (include/opusgpu.h FEATURE BATCHES: k_feat_stats, k_feat_fold, k_feat_batch,
opusgpu_tracks_feature_batch_device, and the whole-file feature calls under opusgpu_set_feature_batch).  The stage alone on the
synthetic grids of tests/test_feat_batch.py, whose padding holds NaN, into a buffer of NaN between two guard lines: NONE, WHISPER
and AFFINE bit for bit against feat_batch_f32, CMN and CMVN within bound_of (derived there, not measured) of feat_batch_ref on every
cell.  Through the files: the dense result against the same restatements applied to the PACKED call's own result."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS
from test_feat_batch import CONSTANT, NORMS, WIDTHS, bound_of, feat_batch_f32, feat_batch_ref, good_request, grid_cells, request_of, strides_of
from test_gpu_tracks_resample import stereo_files
from test_tracks_fbank import spec_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD32, NAN32 = 0x5A5A5A5A, 0x7FC12345
GUARD = 64  # floats of guard at either end: the tensor stays 128-byte aligned


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def packed_grid(pkg, cells, W, frames_major):
    """The packed grid of TRACK FEATURES for these cells, NaN wherever no real cell lies -> (float32 grid, FEAT_SPAN_DTYPE spans)."""
    rng = np.random.default_rng(W + frames_major)
    spans = np.zeros(len(cells), dtype=pkg.FEAT_SPAN_DTYPE)
    at = 0
    for t, x in enumerate(cells):
        plane = (len(x) + 63) // 64 * 64 + 64 * int(rng.integers(0, 2))
        spans[t] = (at, plane, len(x))
        at += W * plane
    grid = np.full(at + 64, np.nan, dtype=np.float32)
    for sp, x in zip(spans, cells):
        F, o, plane = len(x), int(sp["grid_offset"]), int(sp["plane"])
        if frames_major:
            grid[o:o + F * W] = x.reshape(-1)
        else:
            grid[o:o + W * plane].reshape(W, plane)[:, :F] = x.T
    return grid, spans


def run_stage(ctx, d_grid, spans, W, layout, fb, runs=1):
    """The stage into NaN words between two guard lines -> the tensor's words [n, S, W] or [n, W, S], once per run."""
    n, S = len(spans), fb.stride
    fill = np.full(n * S * W + 2 * GUARD, NAN32, dtype=np.uint32)
    fill[:GUARD] = fill[len(fill) - GUARD:] = GUARD32
    d_out = ctx.dev_alloc(fill.nbytes)
    got = []
    try:
        for _ in range(runs):
            ctx.h2d(d_out, fill)
            ctx.tracks_feature_batch_device(spans, W, layout, fb, d_grid, d_out.value + 4 * GUARD)
            g = np.zeros_like(fill)
            ctx.d2h(g, d_out)
            assert (g[:GUARD] == GUARD32).all() and (g[len(g) - GUARD:] == GUARD32).all()  # nothing outside the tensor
            body = g[GUARD:len(g) - GUARD]
            assert not np.isnan(body.view(np.float32)).any()  # every element written
            got.append(body.reshape((n, S, W) if layout == "frames" else (n, W, S)))
    finally:
        ctx.dev_free(d_out)
    return got


def held_to(got, cells, W, frames_major, fb, norm):
    """The tensor's words against the definition: bits for NONE, WHISPER and AFFINE, bound_of for CMN and CMVN, on every cell."""
    if norm in ("none", "whisper", "affine"):
        want = feat_batch_f32(cells, W, frames_major, fb)
        assert np.array_equal(got, np.ascontiguousarray(want).view(np.uint32)), norm
        return 0.0
    ref = feat_batch_ref(cells, W, frames_major, fb)
    bound = bound_of(cells, W, frames_major, fb, ref)
    err = np.abs(got.view(np.float32).astype(np.float64) - ref)
    assert (err <= bound).all(), (norm, float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("layout", ["bands", "frames"])
@pytest.mark.parametrize("W", list(WIDTHS))
def test_stage_alone(pkg, ctx, W, layout):
    """Five norms x two pad modes over one uploaded grid, the stride walking through strides_of: guards, no NaN left, the definition on
    every cell, a constant track exactly 0 under CMN and CMVN, a track without frames all pad, two runs the same bits, and a track
    alone the same bits as among the others."""
    frames, frames_major = WIDTHS[W], layout == "frames"
    cells = grid_cells(W, frames)
    grid, spans = packed_grid(pkg, cells, W, frames_major)
    d_grid = ctx.dev_alloc(grid.nbytes)
    worst = 0.0
    try:
        ctx.h2d(d_grid, grid)
        for k, (norm, pad_mode) in enumerate(itertools.product(NORMS, ["value", "normalized"])):
            S = strides_of(frames)[(k + W) % 5]
            fb = request_of(pkg, W, frames, S, norm, pad_mode)
            first, second = run_stage(ctx, d_grid, spans, W, layout, fb, runs=2)
            assert np.array_equal(first, second), (norm, pad_mode)
            worst = max(worst, held_to(first, cells, W, frames_major, fb, norm))
            f32 = first.view(np.float32)
            by_frame = f32 if frames_major else f32.transpose(0, 2, 1)  # [n, S, W]
            if norm in ("cmn", "cmvn"):
                assert (by_frame[-1, :frames[-1]] == 0).all() and (cells[-1] == CONSTANT).all()  # the constant track: exactly 0
            t0 = frames.index(0) if 0 in frames else None
            if t0 is not None and pad_mode == "value":
                assert (by_frame[t0] == np.float32(-10.0)).all()
            if norm in ("whisper", "cmvn"):  # a track's cells do not depend on its neighbours
                t = frames.index(1025) if 1025 in frames else frames.index(257)
                alone = run_stage(ctx, d_grid, spans[t:t + 1], W, layout, fb)[0]
                assert np.array_equal(alone[0], first[t]), (norm, pad_mode)
    finally:
        ctx.dev_free(d_grid)
    print(f"W {W} {layout}: worst CMN / CMVN error {worst:.3g} of the bound")


# ---- through the files --------------------------------------------------------------------------------------
def cells_of(feats, frames_major):
    return [np.ascontiguousarray(g if frames_major else g.T) for g in feats]


def dense_equals(pkg, dense, dinfo, packed, pinfo, W, frames_major, fb, norm):
    """A dense result against the restatement applied to the packed call's own result; info as the packed call's but for feat_offset."""
    n = len(packed)
    for field in pinfo.dtype.names:
        if field != "feat_offset":
            assert np.array_equal(pinfo[field], dinfo[field]), field
    assert np.array_equal(dinfo["feat_offset"], np.arange(n) * fb.stride * W)
    assert dense.dtype == np.float32 and dense.shape == ((n, fb.stride, W) if frames_major else (n, W, fb.stride))
    cells = cells_of(packed, frames_major)
    assert [len(x) for x in cells] == list(pinfo["frames"])
    held_to(np.ascontiguousarray(dense).view(np.uint32), cells, W, frames_major, fb, norm)
    return sum(x.size for x in cells)


def test_files_whisper(pkg, ctx):
    """decode_files(features="logmel", feature_stride=S, normalize="whisper") of the stereo corpus and the files whose frame fails:
    feat_batch_f32 of the packed call's result, bit for bit; a failed file has its shorter F and pad behind it; the packed call
    returns the same before and after (the request is cleared); loudness=-23.0 composes with normalize="cmn"."""
    files, bad = stereo_files(2)
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    planned_f = -(-b.info["track_samples"] // 3) // 160
    packed, pinfo = ctx.decode_files(None, batch=b, features="logmel", mono=True)
    for S in (int(planned_f.max()), int(planned_f.max()) + 3):
        req = pkg.files_request(b, features="logmel", mono=True, feature_stride=S, normalize="whisper")
        dense, dinfo = ctx.decode_files(None, batch=b, features="logmel", mono=True, feature_stride=S, normalize="whisper")
        assert dense_equals(pkg, dense, dinfo, packed, pinfo, 80, False, req.feature_batch, "whisper") > 10000
    assert any(x is not None for x in bad)
    for i, seq in enumerate(bad):
        if seq is not None:
            F = int(dinfo["frames"][i])
            assert F < planned_f[i] and dinfo["final_status"][i] == -18
            m = packed[i].max() if F else -np.inf
            pad = np.float32((np.float32(max(np.float32(-10.0), np.float32(m - np.float32(8.0)))) + np.float32(4.0)) * np.float32(0.25))
            assert (dense[i][:, F:] == pad).all()
    again, ainfo = ctx.decode_files(None, batch=b, features="logmel", mono=True)  # the request is gone
    assert np.array_equal(ainfo, pinfo) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(again, packed))
    # normalisation alone: S is the largest planned F; frames-major; with a loudness target in the feature kernel's scale
    lp, lpinfo = ctx.decode_files(None, batch=b, features="logmel", mono=True, feature_layout="frames", loudness=-23.0)
    req = pkg.files_request(b, features="logmel", mono=True, feature_layout="frames", normalize="cmn", loudness=-23.0)
    assert req.feature_batch.stride == planned_f.max()
    ld, ldinfo = ctx.decode_files(None, batch=b, features="logmel", mono=True, feature_layout="frames", normalize="cmn", loudness=-23.0)
    assert (ldinfo["gain"] != 1.0).any()
    assert dense_equals(pkg, ld, ldinfo, lp, lpinfo, 80, True, req.feature_batch, "cmn") > 10000
    b.close()


def test_files_kaldi_cmvn_and_cuts(pkg, ctx):
    """kaldi_fbank with "cmvn" over whole files, and over a packed batch of cuts with feature_stride=: within the bound of the
    packed call's result."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)]
    rec = pkg.kaldi_fbank(num_mel_bins=23)
    for cuts in (None, [(0, 0, None), (1, 100, 3000), (2, 960, 6000), (3, 0, 1)]):
        n = len(files) if cuts is None else len(cuts)
        ctx.streams_alloc(n, 2)
        b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
        kw = dict(batch=b, features=rec, mono=True, scale=1.0)
        packed, pinfo = ctx.decode_files(None, **kw)
        S = int(pkg.fbank_frames(rec, -(-b.info["track_samples"] // 3)).max()) + 5
        norm = pkg.feature_norm("cmvn", var_floor=1e-4)
        req = pkg.files_request(b, features=rec, mono=True, scale=1.0, feature_stride=S, normalize=norm)
        dense, dinfo = ctx.decode_files(None, feature_stride=S, normalize=norm, **kw)
        cells = dense_equals(pkg, dense, dinfo, packed, pinfo, 23, True, req.feature_batch, "cmvn")
        assert cells > (2000 if cuts is None else 200)
        if cuts is not None:
            assert np.array_equal(dinfo["cut_start"], b.cut_info["start"]) and (dinfo["frames"] < S).all()
        b.close()


def test_surround_mfcc_cmn(pkg):
    """kaldi_mfcc on a 5.1 MultistreamContext through mix="mono" with "cmn": within the bound of the packed call's result, and the
    packed call unchanged behind it."""
    layout = LAYOUTS["5.1"]
    n = 9
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 7)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, threads=2)
    rec = spec_of(pkg, "mfcc8k")
    kw = dict(batch=b, features=rec, rate=8000, mix="mono", scale=1.0)
    packed, pinfo = ms.decode_files(None, **kw)
    req = pkg.files_request(b, True, 0, features=rec, rate=8000, mix="mono", scale=1.0, normalize="cmn", feature_pad=(2.5, "normalized"))
    dense, dinfo = ms.decode_files(None, normalize="cmn", feature_pad=(2.5, "normalized"), **kw)
    assert dense_equals(pkg, dense, dinfo, packed, pinfo, 13, True, req.feature_batch, "cmn") > 500
    again, ainfo = ms.decode_files(None, **kw)
    assert np.array_equal(ainfo, pinfo) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(again, packed))
    b.close()
    ms.close()


def test_refusals_through_the_c_abi(pkg, ctx):
    """opusgpu_files_decode_mel with a request whose stride is too small, and opusgpu_files_decode_fbank under AFFINE vectors of
    another width: OPUSGPU_BAD_ARG, the buffer and the arrays as they were; with the request off the call works."""
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2)
    n = b.n_files
    lib = ctx.lib
    params, kaldi = pkg.mel_params(80, "bands"), pkg.kaldi_fbank(num_mel_bins=23)
    planned_f = int((-(-b.info["track_samples"] // 3) // 160).max())
    total = max(pkg.mel_layout(b.info["track_samples"], 80, "bands")[2], n * planned_f * 80)
    fill = np.full(total + 64, GUARD32, dtype=np.uint32)
    d_out = ctx.dev_alloc(fill.nbytes)
    arrays = [np.full(n, -7, dtype=np.int64) for _ in range(3)] + [np.full((n, 2), -7, dtype=np.int32)]
    tail = [a.ctypes.data for a in arrays]
    sub, mul = np.zeros(80, dtype=np.float32), np.ones(80, dtype=np.float32)
    try:
        ctx.h2d(d_out, fill)
        short = good_request(pkg, stride_frames=planned_f - 1)
        assert lib.opusgpu_set_feature_batch(ctx.h, short.ctypes.data, None, None, 0) == 0
        assert lib.opusgpu_files_decode_mel(ctx.h, b.h, 1, None, params.ctypes.data, None, d_out, *tail) == pkg.OPUSGPU_BAD_ARG
        assert b"stride_frames is below" in lib.opusgpu_last_error(ctx.h)
        affine = good_request(pkg, norm=pkg.FEAT_NORM_AFFINE, stride_frames=planned_f)
        assert lib.opusgpu_set_feature_batch(ctx.h, affine.ctypes.data, sub.ctypes.data, mul.ctypes.data, 80) == 0
        assert lib.opusgpu_files_decode_fbank(ctx.h, b.h, 16000, 0, 0, 1, None, kaldi.ctypes.data, None, d_out, *tail) == pkg.OPUSGPU_BAD_ARG
        got = np.zeros_like(fill)
        ctx.d2h(got, d_out)
        assert (got == GUARD32).all() and all((a == -7).all() for a in arrays)
        assert lib.opusgpu_files_decode_mel(ctx.h, b.h, 1, None, params.ctypes.data, None, d_out, *tail) == 0  # width 80: in order
        assert np.array_equal(arrays[0], np.arange(n) * planned_f * 80)
        assert lib.opusgpu_set_feature_batch(ctx.h, None, None, None, 0) == 0
        assert lib.opusgpu_files_decode_mel(ctx.h, b.h, 1, None, params.ctypes.data, None, d_out, *tail) == 0
        assert np.array_equal(arrays[0], pkg.mel_layout(b.info["track_samples"], 80, "bands")[0])
    finally:
        lib.opusgpu_set_feature_batch(ctx.h, None, None, None, 0)
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
S = int((-(-b.info["track_samples"] // 3) // 160).max()) + 7
kw = dict(batch=b, features="logmel", mono=True, feature_stride=S, normalize="whisper")
want, winfo = ctx.decode_files(None, **kw)
assert want.shape == (n, 80, S)
FILL = 12345.5
out = torch.full((n * 80 * S + 256,), FILL, dtype=torch.float32, device="cuda:0")
got, info = ctx.decode_files(None, out=out, **kw)
assert np.array_equal(info, winfo)
assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, 80, S)
assert got.untyped_storage().data_ptr() == out.untyped_storage().data_ptr() and got.data_ptr() == out.data_ptr()  # a view of `out`
assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
assert bool((out[n * 80 * S:] == FILL).all())
before = out.clone()
for bad in (out[1:], out[:n * 80 * S - 1], out.to(torch.float64), out.cpu()):
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
    """decode_files(features="logmel", feature_stride=S, normalize="whisper", out=tensor): the result is a view of the tensor of shape
    [n, 80, S], equal to the numpy route, the elements behind it as they were; a tensor that does not fit raises before any device
    work.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
