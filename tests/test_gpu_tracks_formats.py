"""Float tracks of the whole-file path on the GPU (include/opusgpu.h TRACK FORMATS: opusgpu_files_decode_as, opusgpu_ms_files_decode_as,
the k_*_assemble_f32 kernels).  A float sample is (float)s * scale with s the int16 sample of the S16 path, one IEEE multiply, so
every check here is bit for bit: the kernels alone against a numpy scatter of `pcm.astype(np.float32) * np.float32(scale)` into a
buffer of guard bytes, whole files against the numpy conversion of the S16 tracks of the same planned batch -- which are
themselves held against the single-file reader / the oracle here, so that the chain is closed inside this file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
import ms_util
import ogg_util
from ms_util import LAYOUTS, OracleMs
from test_gpu_ms_files import KERNEL_LAYOUTS as MS_KERNEL_LAYOUTS

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
FORMATS = ["f32", "f32_planar"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ct():
    return fu.load_ct()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def as_float(track, scale, planar):
    """What a float track must be, from its S16 form [samples, channels]."""
    f = track.astype(np.float32) * np.float32(scale)
    return np.ascontiguousarray(f.T) if planar else f


# ---- the kernels alone ------------------------------------------------------------------------------------
def crafted(rng, pkg, n_rows, row, zero_counts, far_src):
    """The segment list of test_assembly_kernel_alone / test_fused_assembly_kernel_alone and a place for every track: track i is d
    samples of guard, the segment, guard up to its plane length -- a multiple of 64 beyond the segment's reach -- and 64 more
    behind its last plane.  -> combos, segs, places, total samples per channel."""
    combos = [(s, c, d) for s in range(8) for c in range(1, 9) for d in range(8)]
    combos += [(s, c, d) for c in ((0,) if zero_counts else ()) + (1, 7, 8, 9, 959, 960, 2880) for s in (0, 3, 8) + ((1913,) if far_src else ())
               for d in (0, 1, 5, 8, 63)]
    combos = [(s, c, d) for s, c, d in combos if s + c <= row]
    n = len(combos)
    segs = np.zeros(n, dtype=pkg.TRACK_SEG_DTYPE)
    places = np.zeros(n, dtype=pkg.TRACK_PLACE_DTYPE)
    at = 0
    for i, (s, c, d) in enumerate(combos):
        plane = (d + c + 63) // 64 * 64 + 64 * int(rng.integers(1, 3))
        segs[i] = (rng.integers(0, n_rows), s, c, i, at + d, i % 5, 0)
        places[i] = (at, plane, 0, 0)
        at += plane + 64
    scale = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    scale[0] = 2.0 ** -15
    assert np.isfinite(scale).all() and (scale < 0).sum() > 10 and (scale != 0).all()
    places["scale"] = scale
    return combos, segs, places, at


def scatter(want, C, planar, sg, pl, samples):
    """The kept samples [count, C] of a segment, converted, to their elements of the flat track buffer."""
    f = samples.astype(np.float32) * np.float32(pl["scale"])
    if planar:
        first = sg["dst_first"] - pl["track_offset"]
        for c in range(C):
            base = C * pl["track_offset"] + c * pl["plane_samples"] + first
            want[base:base + sg["count"]] = bits(f[:, c])
    else:
        want[C * sg["dst_first"]:C * (sg["dst_first"] + sg["count"])] = bits(f).ravel()


def expect(C, planar, segs, places, total, row_res, state, rows):
    want = np.full(total * C, GUARD, dtype=np.uint32)
    want_state = state.copy()
    written = 0
    for sg in segs:
        t, r = sg["track"], sg["slot"]
        if row_res[r] < 0:
            if sg["packet_seq"] < want_state["first_bad"][t]:
                want_state[t] = (sg["packet_seq"], row_res[r])
        elif sg["packet_seq"] < want_state["first_bad"][t]:
            scatter(want, C, planar, sg, places[t], rows[r][sg["src_first"]:sg["src_first"] + sg["count"]])
            written += C * int(sg["count"])
    assert written > 20000 and (want != GUARD).sum() == written
    return want, want_state


def closed_tracks(rng, pkg, n):
    state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
    state["first_bad"] = 2**31 - 1
    closed = rng.choice(n, 40, replace=False)  # tracks that an earlier step has ended at packet 2: segments of packets 2.. write nothing
    state["first_bad"][closed], state["code"][closed] = 2, -18
    return state


def check(got, want, got_state, want_state, combos, segs, C):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (len(bad), bad[:8], [hex(x) for x in got[bad[:4]]], [hex(x) for x in want[bad[:4]]],
                           [(c, int(sg["dst_first"])) for c, sg in zip(combos, segs) if C * (sg["dst_first"] - 64) <= bad[0]][-1:])
    assert np.array_equal(got_state, want_state)
    assert (want_state["first_bad"] != 2**31 - 1).sum() > 40  # failed rows have ended tracks


@pytest.mark.parametrize("format", FORMATS)
@pytest.mark.parametrize("channels", [1, 2])
def test_assembly_kernel_alone(pkg, ctx, channels, format):
    """k_tracks_assemble_f32 / _planar2 on the crafted segments of test_gpu_files.py::test_assembly_kernel_alone: every src_first /
    count / dst_first residue modulo 8 samples, counts of 1, 7, 8, 9, 959, 960 and 2,880, 37 rows of 2,880, failed rows and tracks
    closed before, a scale per track (negative ones, one of 2**-15); planes longer than the segments reach, so that a wrong stride
    lands in guard; every guard element between tracks, between planes and behind them intact; the state records; n_segs = 0."""
    rng = np.random.default_rng(channels)
    C, ROW, n_rows = channels, 2880, 37
    planar, fmt = format == "f32_planar", pkg.TRACK_FORMATS[format]
    ctx.streams_alloc(1, C)
    combos, segs, places, total = crafted(rng, pkg, n_rows, ROW, False, False)
    n = len(combos)
    pcm = rng.integers(-32768, 32768, (n_rows, ROW, C), dtype=np.int16)
    res = np.full(n_rows, 960, dtype=np.int32)
    res[[5, 21]] = -18
    state = closed_tracks(rng, pkg, n)
    want, want_state = expect(C, planar, segs, places, total, res, state, pcm)
    fill = np.full(total * C, GUARD, dtype=np.uint32)
    bufs = [ctx.dev_alloc(x) for x in (segs.nbytes, pcm.nbytes, res.nbytes, fill.nbytes, state.nbytes, places.nbytes)]
    d_segs, d_pcm, d_res, d_tracks, d_state, d_place = bufs
    try:
        for d, a in ((d_segs, segs), (d_pcm, pcm), (d_res, res), (d_tracks, fill), (d_state, state), (d_place, places)):
            ctx.h2d(d, a)
        ctx.tracks_assemble_device_as(0, d_segs, d_pcm, ROW, d_res, fmt, d_place, d_tracks, d_state)  # n_segs = 0: nothing
        ctx.synchronize()
        got = np.zeros(total * C, dtype=np.uint32)
        ctx.d2h(got, d_tracks)
        assert (got == GUARD).all()
        with pytest.raises(pkg.OpusGpuError):  # a float format without its place table, S16 with one
            ctx.tracks_assemble_device_as(n, d_segs, d_pcm, ROW, d_res, fmt, None, d_tracks, d_state)
        with pytest.raises(pkg.OpusGpuError):
            ctx.tracks_assemble_device_as(n, d_segs, d_pcm, ROW, d_res, pkg.TRACKS_S16, d_place, d_tracks, d_state)
        ctx.tracks_assemble_device_as(n, d_segs, d_pcm, ROW, d_res, fmt, d_place, d_tracks, d_state)
        ctx.synchronize()
        ctx.d2h(got, d_tracks)
        got_state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
        ctx.d2h(got_state, d_state)
    finally:
        for p in bufs:
            ctx.dev_free(p)
    check(got, want, got_state, want_state, combos, segs, C)


MS_LAYOUTS = dict(MS_KERNEL_LAYOUTS, **{k: LAYOUTS[k] for k in ("7.1", "all-coupled", "stereo")})


@pytest.mark.parametrize("format", FORMATS)
@pytest.mark.parametrize("name", list(MS_LAYOUTS))
def test_fused_assembly_kernel_alone(pkg, name, format):
    """k_ms_tracks_assemble_f32 over the layouts of test_gpu_ms_files.py::test_fused_assembly_kernel_alone (and 7.1, all-coupled,
    stereo) with its segments -- counts of 0 and a far src_first included -- and its failed rows, against a numpy scatter through
    ms_util.mapping_apply, with the guard discipline of the test above."""
    layout = MS_LAYOUTS[name]
    C, S, cp, mp = layout
    mono = S - cp
    planar, fmt = format == "f32_planar", pkg.TRACK_FORMATS[format]
    rng = np.random.default_rng(C + S)
    ROW, n_rows = 2880, 13
    combos, segs, places, total = crafted(rng, pkg, n_rows, ROW, True, True)
    n = len(combos)
    segs["slot"][(segs["slot"] == 11) & (segs["src_first"] + segs["count"] > 960)] = 0  # row 11 is a short one
    pc = rng.integers(-32768, 32768, (n_rows * cp, ROW, 2), dtype=np.int16)
    pm = rng.integers(-32768, 32768, (n_rows * mono, ROW), dtype=np.int16)
    codes = np.full((n_rows, S), ROW, dtype=np.int32)
    codes[5, S // 2] = -18          # a middle elementary stream
    if S >= 3:
        codes[9, 1], codes[9, S - 1] = -4, -18  # the first negative one in stream order is the row's
    else:
        codes[9, S - 1] = -4
    codes[11] = 960                 # a shorter row: a result, not an error
    rc = np.ascontiguousarray(codes[:, :cp]).reshape(-1)
    rm = np.ascontiguousarray(codes[:, cp:]).reshape(-1)
    row_res = np.array([next((v for v in codes[r] if v < 0), codes[r, 0]) for r in range(n_rows)])
    mapped = [ms_util.mapping_apply(layout, [pc[r * cp + s] if s < cp else pm[r * mono + s - cp][:, None] for s in range(S)], ROW)
              for r in range(n_rows)]
    state = closed_tracks(rng, pkg, n)
    want, want_state = expect(C, planar, segs, places, total, row_res, state, mapped)
    fill = np.full(total * C, GUARD, dtype=np.uint32)
    ms = pkg.MultistreamContext(0, 1, *layout)
    ctx = pkg.Context(0)
    bufs = [ctx.dev_alloc(max(x, 16)) for x in (segs.nbytes, pc.nbytes, pm.nbytes, rc.nbytes, rm.nbytes, fill.nbytes, state.nbytes, places.nbytes)]
    d_segs, d_pc, d_pm, d_rc, d_rm, d_tracks, d_state, d_place = bufs
    try:
        for d, a in ((d_segs, segs), (d_pc, pc), (d_pm, pm), (d_rc, rc), (d_rm, rm), (d_tracks, fill), (d_state, state), (d_place, places)):
            if a.nbytes:
                ctx.h2d(d, a)
        ms.tracks_assemble_device_as(0, d_segs, d_pc, d_pm, ROW, d_rc, d_rm, fmt, d_place, d_tracks, d_state)  # n_segs = 0: nothing
        ms.synchronize()
        got = np.zeros(total * C, dtype=np.uint32)
        ctx.d2h(got, d_tracks)
        assert (got == GUARD).all()
        ms.tracks_assemble_device_as(n, d_segs, d_pc, d_pm, ROW, d_rc, d_rm, fmt, d_place, d_tracks, d_state)
        ms.synchronize()
        ctx.d2h(got, d_tracks)
        got_state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
        ctx.d2h(got_state, d_state)
    finally:
        for p in bufs:
            ctx.dev_free(p)
        ctx.close()
        ms.close()
    check(got, want, got_state, want_state, combos, segs, C)


# ---- whole files --------------------------------------------------------------------------------------------
def same_outcome(s16, flt, scales, planar):
    (t0, i0), (t1, i1) = s16, flt
    assert np.array_equal(i0, i1)  # lengths, final_status, bad_packet and the plan's fields
    for i, (a, b) in enumerate(zip(t0, t1)):
        want = as_float(a, scales[i], planar)
        assert b.dtype == np.float32 and b.shape == want.shape, (i, b.shape, want.shape)
        assert np.array_equal(bits(b), bits(want)), i


@pytest.mark.parametrize("format", FORMATS)
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("channels", [2, 1])
def test_corpus_float_equals_converted_s16_equals_the_reader(pkg, ctx, ct, channels, pipeline, format):
    corpus = fu.corpus20(channels, channel_switches=False) + fu.refusal_files(channels)
    refused = {c[0]: c[2] for c in fu.refusal_files(channels)}
    ctx.streams_alloc(len(corpus), channels)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch([c[1] for c in corpus], channels=channels, flags=pkg.PAGES_GROUP_BY_MODE, threads=2)
    s16 = ctx.decode_files(None, batch=b)
    flt = ctx.decode_files(None, batch=b, format=format)
    same_outcome(s16, flt, [2.0 ** -15] * len(corpus), format == "f32_planar")
    tracks, info = s16
    kept = 0
    for i, c in enumerate(corpus):  # the S16 tracks against the reader, as test_gpu_files.py asks
        if c[0] in refused:
            assert info["final_status"][i] == refused[c[0]] and len(tracks[i]) == 0, c[0]
            continue
        code, want, _, final = fu.drain(ct, c[1])
        if code != 0:
            assert info["final_status"][i] == code and len(tracks[i]) == 0, c[0]
            continue
        assert info["final_status"][i] in (0, final) and info["bad_packet"][i] == -1, c[0]
        assert info["track_samples"][i] == len(tracks[i]) == len(want), c[0]
        assert np.array_equal(fu.as_stereo(tracks[i]), want), c[0]
        kept += len(want)
    assert kept > 100000
    b.close()


@pytest.mark.parametrize("format", FORMATS)
@pytest.mark.parametrize("rfc", [False, True])
@pytest.mark.parametrize("name", ["5.1", "muted"])
def test_surround_float_equals_converted_s16_equals_the_oracle(pkg, oracle, name, rfc, format):
    layout = LAYOUTS[name]
    n = 9
    rng = np.random.default_rng(sum(name.encode()) + rfc)
    corpus = mf.corpus(pkg, rng, layout, n, 7, rfc=rfc)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, rfc=rfc, threads=2)
    assert (b.info["status"] == 0).all()
    scales = (np.random.default_rng(3).standard_normal(n) / 4096).astype(np.float32)  # negative ones: a muted channel is then -0.0
    s16 = ms.decode_files(None, batch=b)
    flt = ms.decode_files(None, batch=b, format=format, scale=scales)
    same_outcome(s16, flt, scales, format == "f32_planar")
    orc = OracleMs(oracle, layout, n, rfc=rfc)
    tracks, info = s16
    for i, (_, els, ps, trim) in enumerate(corpus):
        want = mf.expected_track(orc, i, els, ps, trim)
        assert (info["final_status"][i], info["bad_packet"][i]) == (0, -1), i
        assert info["track_samples"][i] == b.info["track_samples"][i] == len(tracks[i]) == len(want) > 0, i
        assert np.array_equal(tracks[i], want), i
    b.close()
    ms.close()


@pytest.mark.parametrize("format", FORMATS)
def test_head_gain(pkg, ctx, format):
    """scale="head_gain": the OpusHead output gains +256 and -1541 (Q7.8 dB) as factors, the 1 / 32768 folded in."""
    rng = np.random.default_rng(8)
    gains = [256, -1541]
    files = [fu.opus_file([[fu.packet(rng, 0xFC, 120) for _ in range(3)] for _ in range(2)], 2, 312, serial=60 + i, end_trim=57,
                          head=ogg_util.opus_head(channels=2, pre_skip=312, gain=g))[0] for i, g in enumerate(gains)]
    ctx.streams_alloc(2, 2)
    b = pkg.FileBatch(files, channels=2)
    assert list(b.info["output_gain"]) == gains and (b.info["status"] == 0).all()
    s16 = ctx.decode_files(None, batch=b)
    flt = ctx.decode_files(None, batch=b, format=format, scale="head_gain")
    scales = [pkg.head_gain_scale(g) for g in gains]
    assert scales[0] > 2.0 ** -15 > scales[1] > 0
    assert all(len(t) == 6 * 960 - 312 - 57 and np.abs(t).max() > 1000 for t in s16[0])
    same_outcome(s16, flt, scales, format == "f32_planar")
    b.close()


@pytest.mark.parametrize("format", FORMATS)
@pytest.mark.parametrize("channels", [2, 1])
def test_failed_frames_in_float_tracks(pkg, ctx, channels, format):
    """fu.failing_files: lengths and codes are those of the S16 run, and what lies before the final length is its conversion."""
    files = fu.failing_files(channels)
    ctx.streams_alloc(len(files), channels)
    b = pkg.FileBatch([f[1] for f in files], channels=channels, flags=pkg.PAGES_GROUP_BY_MODE)
    s16 = ctx.decode_files(None, batch=b)
    flt = ctx.decode_files(None, batch=b, format=format)
    same_outcome(s16, flt, [2.0 ** -15] * len(files), format == "f32_planar")
    info = flt[1]
    assert any(bad is not None for _, _, bad in files)
    for i, (name, _, bad_seq) in enumerate(files):
        if bad_seq is None:
            assert (info["final_status"][i], info["bad_packet"][i]) == (0, -1) and info["track_samples"][i] == b.info["track_samples"][i], name
        else:
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, bad_seq), name
            assert info["track_samples"][i] == b.packet_start(i, bad_seq) < b.info["track_samples"][i], name
    b.close()


def test_c_calls_refuse_bad_formats_and_scales(pkg, ctx):
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:3]]
    ctx.streams_alloc(len(files), 2)
    ctx.set_mode(False)
    b = pkg.FileBatch(files, channels=2)
    d = ctx.dev_alloc(int(b.track_samples) * 8)
    one = np.ones(3, dtype=np.float32)
    try:
        for fmt, scale in ((3, None), (-1, None), (pkg.TRACKS_S16, one), (pkg.TRACKS_F32, np.array([1, np.nan, 1], dtype=np.float32)),
                           (pkg.TRACKS_F32_PLANAR, np.array([np.inf, 1, 1], dtype=np.float32))):
            rc = ctx.lib.opusgpu_files_decode_as(ctx.h, b.h, fmt, None if scale is None else scale.ctypes.data, d, None, None)
            assert rc == pkg.OPUSGPU_BAD_ARG, (fmt, scale)
        assert ctx.lib.opusgpu_files_decode_as(ctx.h, b.h, pkg.TRACKS_S16, None, d, None, None) == 0  # the existing call
    finally:
        ctx.dev_free(d)
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
ctx = pkg.Context(0)
ctx.streams_alloc(len(files), 2)
b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE)
want, winfo = ctx.decode_files(None, batch=b, format="f32_planar")
need = int(b.track_samples) * 2
FILL = 12345.5
out = torch.full((need + 256,), FILL, dtype=torch.float32, device="cuda:0")
tracks, info = ctx.decode_files(None, batch=b, format="f32_planar", out=out)
assert np.array_equal(info, winfo) and len(tracks) == len(files) and sum(len(w[0]) for w in want) > 50000
untouched = torch.ones(need + 256, dtype=torch.bool)
for t, w, o, planned in zip(tracks, want, b.info["track_offset"], b.info["track_samples"]):
    assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == w.shape
    assert t.numel() == 0 or t.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()  # a view of `out`
    assert np.array_equal(t.cpu().numpy().view(np.uint32), w.view(np.uint32))
    plane = (int(planned) + 63) // 64 * 64
    for c in range(2):
        untouched[2 * int(o) + c * plane:2 * int(o) + c * plane + w.shape[1]] = False
host = out.cpu()
assert untouched.sum() > 256 and bool((host[untouched] == FILL).all()) and not bool((host[~untouched] == FILL).any())
for bad in (out[1:], out.to(torch.float64), out[:need - 1], out[::2], out.cpu()):
    try:
        ctx.decode_files(None, batch=b, format="f32_planar", out=bad)
    except ValueError:
        continue
    raise AssertionError("accepted a tensor that does not fit")
b.close()
ctx.close()
print("out-tensor ok")
"""


def test_out_tensor_planar(tmp_path):
    """decode_files(out=tensor): straight into a torch tensor's memory, the tracks views of it equal to the numpy route, every
    element outside the tracks' planes as it was.  In a process of its own: torch brings its HIP runtime (see test_abi.py)."""
    script = tmp_path / "out_tensor.py"
    script.write_text(OUT_SCRIPT)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=120)  # torch's import is most of it
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "out-tensor ok" in r.stdout
