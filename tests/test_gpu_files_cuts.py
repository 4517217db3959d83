"""Cuts of files on the GPU (Context.decode_files(cuts=...), opusgpu_files_plan_cuts, k_tracks_fill_tail; include/opusgpu.h WHOLE
FILES / CUTS): every cut against the model of the device path on the oracle, exact cuts against the whole files' tracks, strided
batches against packed ones, and the tail kernel alone against numpy.  Nothing here asserts closeness to a continuous decode."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cuts_util as cu
import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import same_as_resampled_s16
from test_tracks_fbank import TOL, error_of, fbank_ref, kept_cells, spec_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = 128  # bytes: what the tests leave in front of and behind a track buffer


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def corpus_and_cuts(pkg, channels, rfc):
    """Files and the cut list: cu.long_corpus, in RFC mode with fu.corpus_rfc's files of 2.5 to 60 ms packets behind them."""
    files = [c[1] for c in cu.long_corpus(channels)] + ([c[1] for c in fu.corpus_rfc(channels)] if rfc else [])
    whole = pkg.FileBatch(files, channels=channels, rfc=rfc)
    cuts = []
    for i in range(len(files)):
        _, packets = cu.file_tables(whole, i)
        cuts += cu.cut_list(i, packets, int(whole.info["track_samples"][i]))
        for p in range(1, len(packets)):  # inside a frame of a multi-frame packet, with and without pre-roll
            if i >= 4 and packets[p][2] is not None and packets[p][0] in (2880, 5760) and p % 5 == 2:
                cuts += [(i, packets[p][1] + 960 + 100, 300), (i, packets[p][1] + 960 + 100, 300, 0)]
    whole.close()
    return files, cuts


MODEL = {}


def model_of(pkg, oracle, channels, rfc):
    """The model's tracks of the cut batch, computed once per (channels, mode) and shared."""
    if (channels, rfc) not in MODEL:
        files, cuts = corpus_and_cuts(pkg, channels, rfc)
        b = pkg.FileBatch(files, channels=channels, rfc=rfc, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts)
        tracks, lengths, status, _ = fu.model_decode(pkg, oracle, b)
        MODEL[(channels, rfc)] = (files, cuts, [t.copy() for t in tracks], lengths, status, b.cut_info.copy())
        b.close()
    return MODEL[(channels, rfc)]


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("rfc", [False, True])
@pytest.mark.parametrize("channels", [2, 1])
def test_cuts_equal_the_model_and_exact_cuts_the_whole_files(pkg, ctx, oracle, channels, rfc, pipeline):
    files, cuts, want, lengths, status, ci = model_of(pkg, oracle, channels, rfc)
    ctx.streams_alloc(len(cuts), channels)
    ctx.set_pipeline(pipeline)
    tracks, info = ctx.decode_files(files, rfc=rfc, cuts=cuts, threads=2)
    whole, winfo = ctx.decode_files(files, rfc=rfc, threads=2)
    assert (winfo["final_status"] == 0).all() and len(tracks) == len(cuts) > 70
    exact = 0
    for t, c in enumerate(cuts):
        assert (info["final_status"][t], info["bad_packet"][t]) == tuple(status[t]) == (0, -1), t
        assert info["track_samples"][t] == len(tracks[t]) == lengths[t], t
        assert np.array_equal(tracks[t], want[t]), (t, c)
        for f in ci.dtype.names:
            assert info["cut_" + f][t] == ci[f][t]
        if ci["exact"][t]:
            exact += 1
            s = int(ci["start"][t])
            assert np.array_equal(tracks[t], whole[c[0]][s:s + len(tracks[t])]), (t, c)
    assert 10 < exact < len(cuts) and sum(len(x) for x in tracks) > 200000


def test_surround_cuts(pkg, oracle):
    layout = LAYOUTS["5.1"]
    rng = np.random.default_rng(77)
    files = [c[0] for c in mf.corpus(pkg, rng, layout, 3, 30)]
    w = pkg.MsFileBatch(files, layout)
    cuts = []
    for i in range(len(files)):
        cuts += cu.cut_list(i, cu.file_tables(w, i)[1], int(w.info["track_samples"][i]))
    w.close()
    ms = pkg.MultistreamContext(0, len(cuts), *layout)
    b = pkg.MsFileBatch(files, layout, cuts=cuts, threads=2)
    want, lengths, status = mf.model_decode(pkg, oracle, b, layout)
    tracks, info = ms.decode_files(None, batch=b)
    whole, _ = ms.decode_files(files)
    exact = 0
    for t, c in enumerate(cuts):
        assert (info["final_status"][t], info["bad_packet"][t]) == tuple(status[t]) == (0, -1)
        assert len(tracks[t]) == lengths[t] and tracks[t].shape[1] == 6 and np.array_equal(tracks[t], want[t]), (t, c)
        if b.cut_info["exact"][t]:
            exact += 1
            s = int(b.cut_info["start"][t])
            assert np.array_equal(tracks[t], whole[c[0]][s:s + len(tracks[t])]), (t, c)
    assert 3 < exact < len(cuts)
    b.close()
    ms.close()


def failing_cuts(pkg):
    """fu.failing_files(2) and cuts of them: -> (files, cuts, expected (length, status, bad packet) per cut)."""
    files = fu.failing_files(2)
    names = [f[0] for f in files]
    w = pkg.FileBatch([f[1] for f in files], channels=2)
    i, j = names.index("only_frame"), names.index("second_frame")
    at, at2 = w.packet_start(i, 3), w.packet_start(j, 2)
    w.close()
    cuts = [(i, at + 960 + 200, 1000),          # the bad packet in the pre-roll: nothing
            (i, 100, at - 150),                 # ends before it: untouched
            (i, at - 1000, 2500),               # spans it: ends at the packet's start
            (j, at2 - 700, 3000),               # spans a packet whose SECOND frame fails: its first frame lands behind the final length
            (names.index("clean_a"), 500, 3008), (names.index("clean_b"), 0, 1111)]
    return [f[1] for f in files], cuts, [(0, -18, 3), (at - 150, 0, -1), (1000, -18, 3), (700, -18, 2), (3008, 0, -1), (1111, 0, -1)]


@pytest.mark.parametrize("pipeline", [0, 1])
def test_failed_frames(pkg, ctx, pipeline):
    files, cuts, want = failing_cuts(pkg)
    ctx.streams_alloc(len(cuts), 2)
    ctx.set_pipeline(pipeline)
    tracks, info = ctx.decode_files(files, cuts=cuts)
    whole, _ = ctx.decode_files(files)
    assert [(len(t), int(s), int(p)) for t, s, p in zip(tracks, info["final_status"], info["bad_packet"])] == want
    assert list(info["cut_first_packet"]) == [0] * 6 and list(info["cut_exact"]) == [1] * 6  # short files: every cut starts at packet 0
    for t, c in enumerate(cuts):
        s = int(info["cut_start"][t])
        assert np.array_equal(tracks[t], whole[c[0]][s:s + len(tracks[t])]), t


def _tensor_of(packed, fmt, n, stride, ch):
    return packed.reshape(n, ch, stride).transpose(0, 2, 1) if fmt == "f32_planar" else packed.reshape(n, stride, ch)


@pytest.mark.parametrize("slack", [64, 0])
@pytest.mark.parametrize("fmt", ["s16", "f32", "f32_planar"])
def test_strided_batch(pkg, ctx, fmt, slack):
    """Cuts of unequal length, one of them failing with samples left behind its final length, at a stride of the longest cut (3008) and
    64 more, into a buffer filled with a pattern: every track is the packed batch's up to its length and zero from there to the
    stride, and the line in front of the buffer and the one behind it are as they were."""
    files, cuts, want = failing_cuts(pkg)
    stride = 3008 + slack
    n, ch = len(cuts), 2
    ctx.streams_alloc(n, ch)
    ref, rinfo = ctx.decode_files(files, cuts=cuts, format=fmt)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts, stride=stride)
    dtype = np.int16 if fmt == "s16" else np.float32
    guard = LINE // np.dtype(dtype).itemsize
    host = np.full(n * stride * ch + 2 * guard, 0x5A5A if fmt == "s16" else -7.25, dtype=dtype)
    pattern = host[0].copy()
    d = ctx.dev_alloc(host.nbytes)
    try:
        ctx.h2d(d, host)
        lengths, status = np.zeros(n, dtype=np.int64), np.zeros((n, 2), dtype=np.int32)
        ctx.set_mode(False)
        rc = pkg.load_lib().opusgpu_files_decode_as(ctx.h, b.h, pkg.TRACK_FORMATS[fmt], None, C.c_void_p(d.value + LINE), lengths.ctypes.data,
                                                    status.ctypes.data)
        assert rc == 0
        ctx.d2h(host, d)
    finally:
        ctx.dev_free(d)
    assert (host[:guard] == pattern).all() and (host[-guard:] == pattern).all()
    got = _tensor_of(host[guard:-guard], fmt, n, stride, ch)
    assert [(int(ln), int(s), int(p)) for ln, (s, p) in zip(lengths, status)] == want
    for t in range(n):
        r = ref[t].T if fmt == "f32_planar" else ref[t]
        assert np.array_equal(got[t, :lengths[t]], r), t
        assert not got[t, lengths[t]:].any(), (t, np.argwhere(got[t, lengths[t]:] != 0)[:4])
    # the Python route without out=: the tracks per cut
    tracks, info = ctx.decode_files(None, batch=b, format=fmt)
    assert np.array_equal(info["track_samples"], lengths) and all(np.array_equal(x, y) for x, y in zip(tracks, ref))
    for kw in (dict(rate=16000, mono=True), dict(features=pkg.kaldi_fbank(num_mel_bins=80), rate=16000, mono=True)):
        with pytest.raises(ValueError, match="stride"):
            ctx.decode_files(None, batch=b, **kw)
    # and the C calls refuse it with the reason
    offs, cnts = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    rc = pkg.load_lib().opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, 0, None, None, offs.ctypes.data, cnts.ctypes.data,
                                                       lengths.ctypes.data, status.ctypes.data)
    assert rc == -1 and b"stride" in pkg.load_lib().opusgpu_last_error(ctx.h)
    b.close()


@pytest.mark.parametrize("fmt", ["s16", "f32_planar"])
def test_strided_surround_batch(pkg, fmt):
    """The multistream twin: 5.1 cuts of unequal length at a stride, six planes a track in the planar format."""
    layout = LAYOUTS["5.1"]
    rng = np.random.default_rng(78)
    files = [c[0] for c in mf.corpus(pkg, rng, layout, 3, 30)]
    cuts = [(0, 5000, 3000), (1, 100, 3008), (2, 9000, 1), (0, 0, 0), (2, 20000, 2500, 0), (1, 7000, 777)]
    n, ch, stride = len(cuts), 6, 3072
    ms = pkg.MultistreamContext(0, n, *layout)
    mem = pkg.Context(0)
    ref, _ = ms.decode_files(files, cuts=cuts, format=fmt)
    b = pkg.MsFileBatch(files, layout, cuts=cuts, stride=stride)
    dtype = np.int16 if fmt == "s16" else np.float32
    guard = LINE // np.dtype(dtype).itemsize
    host = np.full(n * stride * ch + 2 * guard, 0x5A5A if fmt == "s16" else -7.25, dtype=dtype)
    pattern = host[0].copy()
    d = mem.dev_alloc(host.nbytes)
    try:
        mem.h2d(d, host)
        lengths, status = np.zeros(n, dtype=np.int64), np.zeros((n, 2), dtype=np.int32)
        ms.set_mode(False)
        rc = pkg.load_lib().opusgpu_ms_files_decode_as(ms.h, b.h, pkg.TRACK_FORMATS[fmt], None, C.c_void_p(d.value + LINE), lengths.ctypes.data,
                                                       status.ctypes.data)
        assert rc == 0
        mem.d2h(host, d)
    finally:
        mem.dev_free(d)
    assert (host[:guard] == pattern).all() and (host[-guard:] == pattern).all()
    got = _tensor_of(host[guard:-guard], fmt, n, stride, ch)
    assert list(lengths) == [3000, 3008, 1, 0, 2500, 777] and (status == [0, -1]).all()
    for t in range(n):
        r = ref[t].T if fmt == "f32_planar" else ref[t]
        assert np.array_equal(got[t, :lengths[t]], r) and not got[t, lengths[t]:].any(), t
    tracks, info = ms.decode_files(None, batch=b, format=fmt)
    assert all(np.array_equal(x, y) for x, y in zip(tracks, ref))
    with pytest.raises(ValueError, match="stride"):
        ms.decode_files(None, batch=b, rate=16000)
    b.close()
    mem.close()
    ms.close()


OUT_SCRIPT = r"""
import importlib.util, os, sys
import numpy as np
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "tests"))
spec = importlib.util.spec_from_file_location("esp32_opus_player_amd", os.path.join(root, "esp32-opus-player_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pkg)
import torch
from test_gpu_files_cuts import failing_cuts
files, cuts, want = failing_cuts(pkg)
n, ch = len(cuts), 2
ctx = pkg.Context(0)
ctx.streams_alloc(n, ch)
for fmt, dtype, fill in (("s16", torch.int16, 0x5A5A), ("f32", torch.float32, -7.25), ("f32_planar", torch.float32, -7.25)):
    ref, _ = ctx.decode_files(files, cuts=cuts, format=fmt)
    for stride in (3008, 3072):
        guard = 128 // (2 if fmt == "s16" else 4)
        whole = torch.full((n * stride * ch + 2 * guard,), fill, dtype=dtype, device="cuda:0")
        out = whole[guard:-guard]
        got, info = ctx.decode_files(files, cuts=cuts, stride=stride, format=fmt, out=out)
        assert tuple(got.shape) == ((n, ch, stride) if fmt == "f32_planar" else (n, stride, ch))
        assert got.untyped_storage().data_ptr() == whole.untyped_storage().data_ptr() and got.data_ptr() == out.data_ptr()
        assert [(int(a), int(b), int(c)) for a, b, c in zip(info["track_samples"], info["final_status"], info["bad_packet"])] == want
        host = whole.cpu().numpy()
        assert (host[:guard] == host[0]).all() and (host[-guard:] == host[0]).all() and host[0] != 0
        g = got.cpu().numpy()
        g = g.transpose(0, 2, 1) if fmt == "f32_planar" else g
        for t in range(n):
            ln = int(info["track_samples"][t])
            r = ref[t].T if fmt == "f32_planar" else ref[t]
            assert np.array_equal(g[t, :ln], r) and not g[t, ln:].any(), (fmt, stride, t)
    try:
        ctx.decode_files(files, cuts=cuts, stride=3008, format=fmt, out=out[:n * 3008 * ch - 1])
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
ctx.close()
print("strided-out ok")
"""


def test_strided_batch_into_a_tensor(tmp_path):
    """decode_files(cuts=, stride=, out=tensor) for the three formats and both strides: the result is the caller's memory as
    [n_cuts, stride, channels] ([n_cuts, channels, stride] planar).  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "strided_out.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "strided-out ok" in r.stdout


def _fill_case(pkg, ctx, fmt, channels, spans):
    """opusgpu_tracks_fill_tail_device over `spans` (rows of track_offset, plane, first, end) against numpy, in a buffer of a pattern
    with a line more at each end."""
    dtype = np.int16 if fmt == "s16" else np.float32
    guard = LINE // np.dtype(dtype).itemsize
    planar = fmt == "f32_planar" and channels > 1
    need = max([(o + max(p if planar else 0, e)) * channels for o, p, f, e in spans] + [1])
    rng = np.random.default_rng(need)
    host = (rng.integers(1, 30000, need + 2 * guard)).astype(dtype)  # never 0
    want = host.copy()
    body = want[guard:guard + need]
    for o, p, f, e in spans:
        if planar:
            for c in range(channels):
                body[o * channels + c * p + f:o * channels + c * p + e] = 0
        else:
            body[(o + f) * channels:(o + e) * channels] = 0
    d = ctx.dev_alloc(host.nbytes)
    try:
        ctx.h2d(d, host)
        ctx.tracks_fill_tail(spans, fmt, channels, C.c_void_p(d.value + LINE))
        ctx.d2h(host, d)
    finally:
        ctx.dev_free(d)
    bad = np.nonzero(host != want)[0]
    assert not len(bad), (fmt, channels, bad[:8] - guard, len(bad))
    return int((want == 0).sum())


@pytest.mark.parametrize("fmt,channels", [("s16", 1), ("s16", 2), ("f32", 1), ("f32", 2), ("f32_planar", 2), ("f32_planar", 6), ("s16", 6)])
def test_fill_tail_alone(pkg, ctx, fmt, channels):
    """first and end at every residue of a 16-byte piece (8 samples of mono int16; 4 of the floats), an empty range, a range shorter
    than a piece, one of 3 pieces, and 1, 2 and 1,000 tracks."""
    R = 8 if fmt == "s16" else 4
    per = 16 // (2 if fmt == "s16" else 4)  # elements of a piece
    spans = []
    for a in range(R):
        for b in range(R):
            first, end = 64 + a, 64 + 3 * per + 8 + b  # (a range of 3 pieces and a bit, both ends at every residue)
            spans.append((len(spans) * 192, 192, first, end))
    zeroed = _fill_case(pkg, ctx, fmt, channels, spans)
    assert zeroed == sum(e - f for _, _, f, e in spans) * channels
    short = [(0, 64, 5, 5), (64, 64, 3, 3 + max(1, per // channels - 1)), (128, 64, 1, 2), (192, 64, 0, 3 * per), (256, 64, 64, 64), (320, 64, 0, 0)]
    for n in (1, 2):
        _fill_case(pkg, ctx, fmt, channels, short[:n] if n == 1 else short[1:3])
    _fill_case(pkg, ctx, fmt, channels, short)
    rng = np.random.default_rng(3)
    many = []
    for t in range(1000):
        f = int(rng.integers(0, 257))
        many.append((t * 256, 256, f, int(rng.integers(f, 257))))
    many[17] = (17 * 256, 256, 0, 256)
    assert _fill_case(pkg, ctx, fmt, channels, many) > 50000 * channels
    if fmt == "s16" and channels == 2:  # a tail of megabytes: more pieces than one wave walks in a few steps
        assert _fill_case(pkg, ctx, fmt, channels, [(0, 0, 3, 700001), (700032, 0, 699999, 700000)]) == 2 * (700001 - 3 + 1)
        lib = pkg.load_lib()
        one = np.array([(0, 64, 5, 4)], dtype=pkg.TAIL_SPAN_DTYPE)
        assert lib.opusgpu_tracks_fill_tail_device(ctx.h, 1, one.ctypes.data, 0, 2, None, None) == -1   # end < first
        assert lib.opusgpu_tracks_fill_tail_device(ctx.h, 1, one.ctypes.data, 3, 2, None, None) == -1   # no such format
        one[0] = (0, 64, 0, 65)
        assert lib.opusgpu_tracks_fill_tail_device(ctx.h, 1, one.ctypes.data, 2, 2, None, None) == -1   # planar: past the plane
        assert lib.opusgpu_tracks_fill_tail_device(ctx.h, 1, one.ctypes.data, 0, 9, None, None) == -1   # channels
        assert lib.opusgpu_tracks_fill_tail_device(ctx.h, 0, None, 0, 2, None, None) == 0


def test_cuts_ahead_of_rate_and_features(pkg, ctx):
    """A packed cut batch is a batch like any other: rate=16000, mono=True equals the decimator's numpy restatement of the cut tracks,
    bit for bit, and Kaldi fbank features of 80 bands its float64 reference within the feature tests' tolerance."""
    files, cuts = corpus_and_cuts(pkg, 2, False)
    cuts = [c for c in cuts if c[2] is None or c[2] != 0][:40]
    ctx.streams_alloc(len(cuts), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, cuts=cuts, threads=2)
    s16 = ctx.decode_files(None, batch=b)
    res = ctx.decode_files(None, batch=b, rate=16000, mono=True)
    assert same_as_resampled_s16(pkg, s16, res, 16000, True, "s16", [None] * len(cuts), b.info["track_samples"]) > 30000
    rec = pkg.kaldi_fbank(num_mel_bins=80)  # (the feature tests' set "wenet", whose tolerance this is)
    assert np.array_equal(rec, spec_of(pkg, "wenet"))
    feats, info = ctx.decode_files(None, batch=b, features=rec, rate=16000, mono=True, scale=np.ones(len(cuts), np.float32))
    cells = 0
    worst = 0.0
    for t, (y, g) in enumerate(zip(res[0], feats)):
        ref, mel = fbank_ref(y[:, 0], 1.0, rec)
        assert g.shape == ref.shape and info["frames"][t] == len(ref), t
        keep = kept_cells(mel, rec)
        err = error_of(g, ref, rec)
        worst = max(worst, float(err[keep].max(initial=0)))
        assert (err[keep] <= TOL["wenet"]).all(), (t, float(err[keep].max()))
        cells += int(keep.sum())
    print(f"{cells} cells, worst error {worst:.3g} (allowed {TOL['wenet']:.3g})")
    assert cells > 20000
    for f in b.cut_info.dtype.names:
        assert np.array_equal(info["cut_" + f], b.cut_info[f])
    b.close()
