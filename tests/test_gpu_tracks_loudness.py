"""Track loudness on the GPU (include/opusgpu.h TRACK LOUDNESS: k_tracks_loudness_seg, k_tracks_loudness_gate,
opusgpu_tracks_loudness_device, opusgpu_set_loudness and the whole-file calls under a request).  The kernels alone on the crafted
tracks of tests/test_tracks_loudness.py in a buffer of guard words, against loudness_ref (float64) within TOL; their exact
properties; whole files: a measuring call changes no sample and reports what the kernels alone report on the S16 tracks, a
normalising call equals decode_files(scale=s) bit for bit, s computed here from the records by the gain formula.

TOL: 8 x the largest |lufs| difference of loudness_f32 -- the kernels' arithmetic in float32 numpy -- against loudness_ref over the
crafted tracks (the project's rule for float sums; 8 covers another legitimate summation order), and in
any case the standard's own 0.1 LU.  YARDSTICK_* hold what a CPU measured; tests/test_tracks_loudness.py::yardstick recomputes
them, and its test_the_yardstick_is_what_the_gpu_test_records holds them to that."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
from ms_util import LAYOUTS
from test_gpu_tracks_resample import stereo_files
from test_tracks_loudness import CASES, WEIGHTS, crafted_tracks, loudness_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YARDSTICK_LUFS = 1.14e-03  # LU: the 30 Hz tone on DC, 64 segments
YARDSTICK_ENERGY = 3.26e-02  # relative, per segment energy: a -60 dB segment right behind a full-scale one (tone: 4.5e-4, noise: 3e-6)
TOL = 8 * YARDSTICK_LUFS
GUARD = np.array([32767, -32768], dtype=np.int16)  # between the tracks: full scale, so that a sample read behind a track shows


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def lay_out(pkg, tracks, ch, lead=24):
    """The tracks packed into one int16 buffer, each at a multiple of 8 samples, guard words in front, between and behind them; the
    buffer reaches to the end of the 16-byte piece that holds a track's last sample and no further than the guards."""
    spans = np.zeros(len(tracks), dtype=pkg.LOUDNESS_SPAN_DTYPE)
    at = lead
    for i, x in enumerate(tracks):
        spans[i] = (at, len(x))
        at = (at + len(x) + 7) // 8 * 8 + 8 * (1 + i % 3)
    buf = np.tile(GUARD, (at * ch + 1) // 2)[:at * ch].copy()
    for sp, x in zip(spans, tracks):
        buf[ch * sp["in_offset"]:ch * (sp["in_offset"] + len(x))] = x.ravel()
    return buf, spans


def measured(pkg, ctx, tracks, ch, weights=None, lead=24):
    """tracks_loudness_device over the tracks laid out in one buffer; the buffer comes back as it went."""
    buf, spans = lay_out(pkg, tracks, ch, lead)
    d_in = ctx.dev_alloc(buf.nbytes)
    try:
        ctx.h2d(d_in, buf)
        rec = ctx.tracks_loudness_device(spans, d_in, ch, weights)
        back = np.zeros_like(buf)
        ctx.d2h(back, d_in)
        assert np.array_equal(back, buf)  # every guard word intact, and every sample
    finally:
        ctx.dev_free(d_in)
    return rec


def bits(rec):
    return np.ascontiguousarray(rec).view(np.uint32)


@pytest.mark.parametrize("ch", sorted(CASES))
def test_kernels_alone(pkg, ctx, ch):
    """All crafted tracks of `ch` channels in one call, a zero-length one among them: lufs within TOL of loudness_ref, peak, blocks
    and gated equal to it; a second run and every track measured alone give the same bits."""
    tracks = crafted_tracks(ch)
    assert any(len(x) == 0 for x in tracks) and len({len(x) for x in tracks}) > 5
    rec = measured(pkg, ctx, tracks, ch)
    worst = 0.0
    for i, ((n, kind), x) in enumerate(zip(CASES[ch], tracks)):
        ref = loudness_ref(x, WEIGHTS[ch])
        assert ref.margin > 0.01, (n, kind)  # no block near a gate: equal counts are a fair demand
        got = rec[i]
        print(f"ch {ch} n {n} {kind}: lufs {got['lufs']:.6f} (ref {ref.lufs:.6f}), peak {got['peak']}, blocks {got['blocks']}, gated {got['gated']}")
        assert (int(got["blocks"]), int(got["gated"])) == (ref.blocks, ref.gated), (n, kind)
        assert float(got["peak"]) == ref.peak, (n, kind)
        if np.isfinite(ref.lufs):
            err = abs(float(got["lufs"]) - ref.lufs)
            worst = max(worst, err)
            assert err <= TOL and err <= 0.1, (n, kind, err, TOL)
        else:
            assert got["lufs"] == -np.inf, (n, kind)
    print(f"ch {ch}: worst |lufs - ref| {worst:.3g} LU (allowed {TOL:.3g}, float32 numpy recorded {YARDSTICK_LUFS:.3g})")
    again = measured(pkg, ctx, tracks, ch)
    assert np.array_equal(bits(again), bits(rec))
    for i in range(len(tracks)):  # alone, at another place in another buffer
        alone = measured(pkg, ctx, tracks[i:i + 1], ch, lead=8 * (i % 5))
        assert np.array_equal(bits(alone), bits(rec[i:i + 1])), CASES[ch][i]


def test_weights_and_silence(pkg, ctx):
    rng = np.random.default_rng(3)
    x = rng.integers(-9000, 9001, (30000, 6)).astype(np.int16)
    w = [0.5, 2, 0, 1, 1.41, 3]
    lfe = np.zeros((30000, 6), np.int16)
    lfe[:, 5] = x[:, 5]
    rec = measured(pkg, ctx, [x, lfe, np.zeros((30000, 6), np.int16), x[:0]], 6, w)
    assert abs(float(rec["lufs"][0]) - loudness_ref(x, w).lufs) <= TOL and abs(float(rec["lufs"][1]) - loudness_ref(lfe, w).lufs) <= TOL
    assert rec["lufs"][2] == -np.inf and rec["peak"][2] == 0 and (rec["blocks"][2], rec["gated"][2]) == (3, 0)
    assert rec["lufs"][3] == -np.inf and (rec["blocks"][3], rec["gated"][3], rec["peak"][3]) == (0, 0, 0)
    dflt = measured(pkg, ctx, [x, lfe], 6)
    assert np.array_equal(bits(dflt), bits(measured(pkg, ctx, [x, lfe], 6, pkg.loudness_weights(6))))
    assert dflt["lufs"][1] == -np.inf and dflt["gated"][1] == 0 and dflt["peak"][1] == np.abs(lfe.astype(np.int32)).max() / 32768


def test_kernel_refusals(pkg, ctx):
    """OPUSGPU_BAD_ARG before any device work, and `out` as it was."""
    lib = pkg.load_lib()
    buf = np.zeros((4800 * 5, 2), dtype=np.int16)
    d_in = ctx.dev_alloc(buf.nbytes)
    try:
        ctx.h2d(d_in, buf)
        ok = np.zeros(1, dtype=pkg.LOUDNESS_SPAN_DTYPE)
        ok[0] = (0, 24000)
        out = np.full(4, 0x5A5A5A5A, dtype=np.uint32)

        def call(spans, ptr, channels, weights):
            w = None if weights is None else np.asarray(weights, dtype=np.float32)
            return lib.opusgpu_tracks_loudness_device(ctx.h, len(spans), spans.ctypes.data, ptr, channels, None if w is None else w.ctypes.data,
                                                      out.ctypes.data, None)
        odd, neg = ok.copy(), ok.copy()
        odd[0], neg[0] = (4, 100), (0, -1)
        for spans, ptr, channels, weights in ((ok, d_in, 0, None), (ok, d_in, 9, None), (odd, d_in, 2, None), (neg, d_in, 2, None),
                                              (ok, d_in, 2, [1, -0.5]), (ok, d_in, 2, [np.nan, 1]), (ok, d_in, 2, [np.inf, 1]),
                                              (ok, d_in.value + 2, 2, None)):
            assert call(spans, ptr, channels, weights) == pkg.OPUSGPU_BAD_ARG
            assert (out == 0x5A5A5A5A).all()
        assert call(ok, d_in, 2, None) == 0 and out.view(pkg.LOUDNESS_DTYPE)[0]["blocks"] == 2
        req = np.zeros(1, dtype=pkg.LOUDNESS_REQ_DTYPE)
        for mode, target, limit, nw, w0 in ((3, -23, 1, 0, 0), (-1, -23, 1, 0, 0), (1, -23, 1, 9, 0), (1, -23, 1, 2, -1), (1, -23, 1, 1, np.nan),
                                            (2, np.inf, 1, 0, 0), (2, -23, np.nan, 0, 0)):
            req[0] = (mode, target, limit, nw, [w0] + [0] * 7)
            assert lib.opusgpu_set_loudness(ctx.h, req.ctypes.data) == pkg.OPUSGPU_BAD_ARG
        assert lib.opusgpu_last_loudness(ctx.h, 0, None, None) == 0
    finally:
        ctx.dev_free(d_in)


# ---- whole files --------------------------------------------------------------------------------------------
TARGET = -23.0


def gain_of(rec, target, limit):
    """TRACK LOUDNESS, GAIN, in double."""
    lufs, peak = float(rec["lufs"]), float(rec["peak"])
    if lufs == -np.inf:
        return 1.0
    g = 10.0 ** ((target - lufs) / 20.0)
    return limit / peak if limit > 0 and peak * g > limit else g


def scales_of(info, target, limit, base=None):
    g = np.array([gain_of(r, target, limit) for r in info], dtype=np.float64)
    base = np.full(len(info), 2.0 ** -15, dtype=np.float32) if base is None else np.asarray(base, dtype=np.float32)
    return (base.astype(np.float64) * g).astype(np.float32), g


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                                                                                 y.view(np.uint32) if y.dtype == np.float32 else y)
                                    for x, y in zip(a, b))


def alone_on(pkg, ctx, s16_tracks, ch, weights=None):
    """The kernels alone over the S16 tracks of the default path, at their final lengths."""
    return measured(pkg, ctx, [np.ascontiguousarray(t) for t in s16_tracks], ch, weights)


def check_outputs(pkg, ctx, dec, b, outs, s16_outs, ch):
    """dec: the decoder's decode_files.  For every output: loudness="measure" changes nothing and reports the standalone records;
    loudness=TARGET equals scale=s; then a bound peak limit on top of a caller's scale."""
    s16 = dec(None, batch=b)
    want = alone_on(pkg, ctx, s16[0], ch)
    assert (want["blocks"] > 0).sum() >= 3 and np.isfinite(want["lufs"]).sum() >= 3 and (want["lufs"] == -np.inf).any()
    n = b.n_files
    for kw in s16_outs + outs:
        plain = dec(None, batch=b, **kw)
        m = dec(None, batch=b, loudness="measure", **kw)
        assert same(m[0], plain[0]), kw
        for f in plain[1].dtype.names:
            assert np.array_equal(m[1][f], plain[1][f]), (kw, f)
        for mine, theirs in (("lufs", "lufs"), ("peak", "peak"), ("loudness_blocks", "blocks"), ("loudness_gated", "gated")):
            assert np.array_equal(bits(m[1][mine]), bits(want[theirs])), (kw, mine)
        assert (m[1]["gain"] == 1.0).all()
    for kw in outs:
        for target, limit, base in ((TARGET, 1.0, None), (-6.0, 0.25, np.linspace(0.5, 2.0, n) / 32768)):
            s, g = scales_of(want, target, limit, base)
            more = {} if base is None else {"scale": base}
            got = dec(None, batch=b, loudness=target, peak_limit=limit, **more, **kw)
            ref = dec(None, batch=b, scale=s, **kw)
            assert same(got[0], ref[0]), (kw, target)
            assert np.array_equal(got[1]["gain"], g) and np.array_equal(bits(got[1]["lufs"]), bits(want["lufs"])), (kw, target)
            assert (g[want["lufs"] == -np.inf] == 1.0).all()
            if limit < 1:  # the limit binds somewhere, and where it does the peak lands on it
                lufs = np.where(np.isfinite(want["lufs"]), want["lufs"], target).astype(np.float64)
                bound = np.isfinite(want["lufs"]) & (want["peak"].astype(np.float64) * 10.0 ** ((target - lufs) / 20) > limit)
                assert bound.any() and np.allclose(g[bound] * want["peak"][bound], limit, rtol=1e-12)
    for kw in s16_outs:  # an int16 result takes no gain
        with pytest.raises(ValueError):
            dec(None, batch=b, loudness=TARGET, **kw)
    return s16, want


def long_files(rng, channels, serial):
    """Three files long enough for blocks: 26, 40 and 31 CELT packets (520 - 800 ms), the second with a quiet middle."""
    celt = fu.TOCS20[channels][2]
    out = []
    for i, n in enumerate((26, 40, 31)):
        pk = [fu.packet(rng, celt, 120 if (i != 1 or j < 12 or j > 27) else 8) for j in range(n)]
        out.append(fu.opus_file([pk[j:j + 5] for j in range(0, n, 5)], channels, 312, serial=serial + i, end_trim=211 * i)[0])
    return out


@pytest.mark.parametrize("pipeline", [0, 1])
def test_stereo_files(pkg, ctx, pipeline):
    """The stereo corpus, the files whose frame fails on the device (measured at their final lengths), a header-only file (gain 1)
    and three longer ones; in order and pipelined."""
    files, bad = stereo_files(2)
    files = files + long_files(np.random.default_rng(77), 2, 900)
    ctx.streams_alloc(len(files), 2)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    outs = [dict(format="f32"), dict(format="f32_planar"), dict(rate=16000, mono=True, format="f32"), dict(resample=44100, format="f32"),
            dict(features="logmel", mono=True)]
    s16, want = check_outputs(pkg, ctx, ctx.decode_files, b, outs, [dict(), dict(rate=16000, mono=True)], 2)
    info = ctx.decode_files(None, batch=b, loudness="measure", rate=16000, mono=True)[1]
    assert any(x is not None for x in bad)
    for i, seq in enumerate(bad):
        if seq is not None:  # a failed track: its record is that of its final length
            final = b.packet_start(i, seq)
            assert info["track_samples"][i] == final < b.info["track_samples"][i] and info["loudness_blocks"][i] == max(0, final // 4800 - 3)
            assert info["peak"][i] == np.abs(s16[0][i].astype(np.int32)).max(initial=0) / 32768
    empty = [i for i in range(b.n_files) if s16[1]["track_samples"][i] == 0]
    assert empty and (want["lufs"][empty] == -np.inf).all() and (want["peak"][empty] == 0).all()
    # the header's float tracks are those of the identity mix: format= alone, with and without a request, lands on the same elements
    assert same(ctx.decode_files(None, batch=b, format="f32", loudness="measure")[0], ctx.decode_files(None, batch=b, format="f32")[0])
    ctx.set_pipeline(0)
    b.close()


def test_surround_files(pkg, ctx):
    """5.1 files through mix="stereo", all channels and the rate: the measurement is taken in front of the mix, on six channels with
    the layout's default weights; a caller's weights reach the kernels."""
    layout = LAYOUTS["5.1"]
    n = 7
    corpus = mf.corpus(pkg, np.random.default_rng(51), layout, n, 27, per_page=6)
    ms = pkg.MultistreamContext(0, n + 1, *layout)
    files = [c[0] for c in corpus] + [fu.opus_file([], head=mf.head(layout, 312))[0]]  # and a header-only file
    b = pkg.MsFileBatch(files, layout, threads=2)
    assert (b.info["status"][:n] == 0).all()
    outs = [dict(mix="stereo", format="f32"), dict(format="f32"), dict(rate=16000, format="f32_planar"), dict(features="logmel", mix="mono")]
    s16, want = check_outputs(pkg, ctx, ms.decode_files, b, outs, [dict(), dict(mix="stereo")], 6)
    w = [1, 1, 1, 0, 0, 1]
    info = ms.decode_files(None, batch=b, loudness="measure", channel_weights=w, mix="stereo")[1]
    mine = alone_on(pkg, ctx, s16[0], 6, w)
    assert np.array_equal(bits(info["lufs"]), bits(mine["lufs"])) and not np.array_equal(bits(mine["lufs"]), bits(want["lufs"]))
    b.close()
    ms.close()


def test_c_level_refusals_and_switching_off(pkg, ctx):
    lib = pkg.load_lib()
    files = stereo_files(2)[0]
    ctx.streams_alloc(len(files), 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    ctx.set_mode(b.rfc)
    n = b.n_files
    lengths, status = np.full(n, -7, dtype=np.int64), np.full((n, 2), -7, dtype=np.int32)
    req = np.zeros(1, dtype=pkg.LOUDNESS_REQ_DTYPE)
    d = ctx.dev_alloc(max(int(b.track_samples), 1) * 2 * 4)
    try:
        req[0] = (pkg.LOUDNESS_NORMALIZE, -23.0, 1.0, 0, [0] * 8)
        assert lib.opusgpu_set_loudness(ctx.h, req.ctypes.data) == 0
        assert lib.opusgpu_files_decode(ctx.h, b.h, d, lengths.ctypes.data, status.ctypes.data) == pkg.OPUSGPU_BAD_ARG  # int16 takes no gain
        assert lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, pkg.TRACKS_S16, None, d, None, None, lengths.ctypes.data,
                                                  status.ctypes.data) == pkg.OPUSGPU_BAD_ARG
        req[0] = (pkg.LOUDNESS_MEASURE, 0, 0, 0, [0] * 8)
        assert lib.opusgpu_set_loudness(ctx.h, req.ctypes.data) == 0
        for fmt in (pkg.TRACKS_F32, pkg.TRACKS_F32_PLANAR):  # never an int16 track: refused, and the message names the way round
            assert lib.opusgpu_files_decode_as(ctx.h, b.h, fmt, None, d, lengths.ctypes.data, status.ctypes.data) == pkg.OPUSGPU_BAD_ARG
            msg = lib.opusgpu_last_error(ctx.h).decode()
            assert "_mixed" in msg and "48000" in msg and "identity" in msg and "16384" in msg
        assert (lengths == -7).all() and (status == -7).all()
        req[0] = (pkg.LOUDNESS_MEASURE, 0, 0, 3, [1, 1, 1] + [0] * 5)  # three weights for two channels
        assert lib.opusgpu_set_loudness(ctx.h, req.ctypes.data) == 0
        assert lib.opusgpu_files_decode(ctx.h, b.h, d, lengths.ctypes.data, status.ctypes.data) == pkg.OPUSGPU_BAD_ARG
        req[0] = (pkg.LOUDNESS_MEASURE, 0, 0, 0, [0] * 8)
        assert lib.opusgpu_set_loudness(ctx.h, req.ctypes.data) == 0
        assert lib.opusgpu_files_decode(ctx.h, b.h, d, lengths.ctypes.data, status.ctypes.data) == 0
        rec, gains = np.zeros(n, dtype=pkg.LOUDNESS_DTYPE), np.zeros(n)
        assert lib.opusgpu_last_loudness(ctx.h, n, rec.ctypes.data, gains.ctypes.data) == n and (gains == 1).all()
        assert lib.opusgpu_set_loudness(ctx.h, None) == 0
    finally:
        ctx.dev_free(d)
    plain = ctx.decode_files(None, batch=b, format="f32")  # files_decode_as again: the request is off
    fresh = pkg.Context(0)
    want = fresh.decode_files(None, batch=b, format="f32")
    fresh.close()
    assert same(plain[0], want[0]) and np.array_equal(plain[1], want[1]) and "lufs" not in plain[1].dtype.names
    m = ctx.decode_files(None, batch=b, loudness="measure")
    assert np.array_equal(bits(m[1]["lufs"]), bits(rec["lufs"])) and np.array_equal(bits(m[1]["peak"]), bits(rec["peak"]))
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
from test_gpu_tracks_loudness import long_files
import torch
files = [c[1] for c in fu.corpus20(2, channel_switches=False)] + long_files(np.random.default_rng(77), 2, 900)
ctx = pkg.Context(0)
b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
FILL = 12345.5
for kw in (dict(format="f32"), dict(format="f32_planar"), dict(rate=16000, mono=True, format="f32")):
    want, winfo = ctx.decode_files(None, batch=b, loudness=-23.0, peak_limit=0.5, **kw)
    assert (winfo["gain"] != 1.0).sum() >= 3
    req = pkg.files_request(b, loudness=-23.0, **kw)
    out = torch.full((req.total * req.channels + 256,), FILL, dtype=torch.float32, device="cuda:0")
    tracks, info = ctx.decode_files(None, batch=b, loudness=-23.0, peak_limit=0.5, out=out, **kw)
    assert np.array_equal(info, winfo) and len(tracks) == len(files) and sum(w.size for w in want) > 100000
    for t, w in zip(tracks, want):
        assert t.is_cuda and tuple(t.shape) == w.shape
        assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
        assert np.array_equal(t.cpu().numpy().view(np.uint32), w.view(np.uint32))
    assert bool((out[-256:] == FILL).all())
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor(tmp_path):
    """decode_files(loudness=, out=tensor): the normalised tracks straight into a torch tensor, views of it equal to the numpy route
    -- the identity-mix route of format="f32" included.  In a process of its own: torch brings its HIP runtime."""
    script = tmp_path / "out_tensor_loudness.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
