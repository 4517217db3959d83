"""Track loudness of the whole-file path (include/opusgpu.h, TRACK LOUDNESS), what needs no GPU: loudness_ref, the header's section
restated in float64 with scipy.signal.lfilter, which every check here and in tests/test_gpu_tracks_loudness.py compares against;
known answers from outside the project (EBU Tech 3341); the cases the definition pins; the host functions; the refusals decode_files
raises before any device work.  loudness_f32 restates the kernels' own arithmetic in numpy -- float32, one segment of warm-up,
transposed direct form II, nothing fused, the gate in float64 -- and yardstick() measures it against loudness_ref over the crafted
tracks of the GPU test, whose tolerance is 8 x that."""
import collections
import os
import re

import numpy as np
import pytest
from scipy.signal import lfilter

from test_kernel_budget import _kernel_metadata
from test_tracks_resample import batch, ms_batch  # noqa: F401 (fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_loudness_weights", "opusgpu_loudness_gain", "opusgpu_tracks_loudness_device", "opusgpu_set_loudness", "opusgpu_last_loudness",
       "opusgpu_ms_set_loudness", "opusgpu_ms_last_loudness"]
# BS.1770-4, the 48 kHz K-weighting
K1_B, K1_A = [1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585]
K2_B, K2_A = [1.0, -2.0, 1.0], [1.0, -1.99004745483398, 0.99007225036621]
SEG = 4800
WEIGHTS = {1: [1], 2: [1, 1], 3: [1, 1, 1], 4: [1, 1, 1.41, 1.41], 5: [1, 1, 1, 1.41, 1.41], 6: [1, 1, 1, 1.41, 1.41, 0],
           7: [1, 1, 1, 1.41, 1.41, 1, 0], 8: [1, 1, 1, 1.41, 1.41, 1, 1, 0]}

Loudness = collections.namedtuple("Loudness", "lufs peak blocks gated energies powers margin")


def gate(e, weights):
    """Segment energies [segments, channels] (float64) -> (lufs, blocks, gated, block powers, the smallest distance in LU of a
    block from either gate -- inf where there is none)."""
    w = np.asarray(weights, dtype=np.float64)
    blocks = max(0, len(e) - 3)
    if not blocks:
        return -np.inf, 0, 0, np.zeros(0), np.inf
    p = ((e[0:blocks] + e[1:blocks + 1] + e[2:blocks + 2] + e[3:blocks + 3]) @ w) / (4 * SEG)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10 * np.log10(p)
    a = l > -70
    margin = np.abs(l[np.isfinite(l)] + 70).min(initial=np.inf)
    if not a.any():
        return -np.inf, blocks, 0, p, margin
    rel = 0.1 * p[a].mean()
    g = a & (p > rel)
    margin = min(margin, np.abs(10 * np.log10(p[a] / rel)).min())
    return -0.691 + 10 * np.log10(p[g].mean()), blocks, int(g.sum()), p, margin


def loudness_ref(track, weights):
    """TRACK LOUDNESS to the letter, in float64: track int16 [n, channels], all of it signal (the FINAL length)."""
    track = np.asarray(track)
    n, ch = track.shape
    x = track.astype(np.float64) / 32768
    z = lfilter(K2_B, K2_A, lfilter(K1_B, K1_A, x, axis=0), axis=0) if n else x
    segs = n // SEG
    e = (z[:segs * SEG] ** 2).reshape(segs, SEG, ch).sum(axis=1)
    lufs, blocks, gated, p, margin = gate(e, weights)
    peak = np.abs(track.astype(np.int32)).max(initial=0) / 32768
    return Loudness(lufs, peak, blocks, gated, e, p, margin)


def loudness_f32(tracks, weights):
    """The kernels' arithmetic for a list of int16 tracks [n, channels] of one channel count: every whole segment filtered in
    float32 from zero state one segment earlier (segment 0: at the track's first sample -- a warm-up over zeros leaves the state
    zero), transposed direct form II, each product and sum rounded on its own, the energy summed sample by sample; blocks, gates
    and means in float64 from the float32 energies; lufs rounded to float32.  All segments of all tracks run side by side."""
    ch = tracks[0].shape[1]
    f = np.float32
    rows, owner = [], []
    for t, x in enumerate(tracks):
        pad = np.concatenate([np.zeros((SEG, ch), np.int16), x])
        for j in range(len(x) // SEG):
            rows.append(pad[j * SEG:(j + 2) * SEG])
            owner.append(t)
    e = np.zeros((len(rows), ch), dtype=f)
    if rows:
        X = np.stack(rows).astype(f) * f(1.0 / 32768)  # [segments, 2 * SEG, channels]
        (b10, b11, b12), (_, a11, a12) = [[f(v) for v in c] for c in (K1_B, K1_A)]
        (b20, b21, b22), (_, a21, a22) = [[f(v) for v in c] for c in (K2_B, K2_A)]
        s = np.zeros((4,) + e.shape, dtype=f)
        for n in range(2 * SEG):
            x = X[:, n]
            y = b10 * x + s[0]
            s[0] = (b11 * x - a11 * y) + s[1]
            s[1] = b12 * x - a12 * y
            z = b20 * y + s[2]
            s[2] = (b21 * y - a21 * z) + s[3]
            s[3] = b22 * y - a22 * z
            if n >= SEG:
                e = e + z * z
        assert e.dtype == f and s.dtype == f
    owner = np.array(owner, dtype=np.int64)
    out = []
    for t, x in enumerate(tracks):
        et = e[owner == t].astype(np.float64)
        lufs, blocks, gated, p, margin = gate(et, np.asarray(weights, dtype=f))
        out.append(Loudness(float(f(lufs)), np.abs(x.astype(np.int32)).max(initial=0) / 32768, blocks, gated, et, p, margin))
    return out


# ---- the crafted tracks of the GPU test -----------------------------------------------------------------------
TILE = 64  # segments of a tile of k_tracks_loudness_seg (LOUD_TILE): the long lengths lie around TILE * SEG
LONG = [TILE * SEG - 1, TILE * SEG, TILE * SEG + 1, 68 * SEG + 77]
CASES = {1: [(0, "noise"), (1, "noise"), (4799, "noise"), (4800, "noise"), (19199, "noise"), (19200, "noise"), (19201, "tone"), (23999, "quiet"),
             (24000, "zeros"), (24001, "noise"), (LONG[0], "stepped"), (LONG[1], "tone"), (LONG[2], "spotlight"), (LONG[3], "spotlight"),
             (LONG[3], "stepped"), (LONG[1], "quiet")],
         6: [(0, "noise"), (4799, "quiet"), (19200, "noise"), (24001, "tone"), (LONG[2], "spotlight"), (LONG[3], "stepped")]}
CASES[2], CASES[8] = CASES[1], CASES[6]
STEPS_DB = [0, -15, -30, -60, -80]
SEED = 1770


def crafted(rng, n, ch, kind):
    """int16 [n, ch].  noise: full-scale uniform; quiet: +-40; zeros; tone: 30 Hz riding on a DC offset (the worst case for float32:
    the filter removes nearly all of it); stepped: noise whose segments carry gains drawn from STEPS_DB, so that both gates have
    something to drop; spotlight: full scale in four consecutive segments that end or straddle a tile boundary, +-2 elsewhere."""
    if kind == "zeros":
        return np.zeros((n, ch), dtype=np.int16)
    if kind == "quiet":
        return rng.integers(-40, 41, (n, ch)).astype(np.int16)
    noise = rng.integers(-32768, 32768, (n, ch)).astype(np.int16)
    if kind == "noise":
        return noise
    if kind == "tone":
        t = np.arange(n)[:, None] / 48000.0
        return np.rint(12000 + 8000 * np.sin(2 * np.pi * 30 * t + np.arange(ch)[None, :])).astype(np.int16)
    if kind == "stepped":
        g = 10 ** (rng.choice(STEPS_DB, -(-n // SEG)) / 20.0)
        return np.rint(noise * np.repeat(g, SEG)[:n, None]).astype(np.int16)
    assert kind == "spotlight" and n >= TILE * SEG
    x = rng.integers(-2, 3, (n, ch)).astype(np.int16)
    first = TILE - 4 if n < (TILE + 2) * SEG else TILE - 2  # segments 60 .. 63, or 62 .. 65
    x[first * SEG:(first + 4) * SEG] = noise[first * SEG:(first + 4) * SEG]
    return x


def crafted_tracks(ch):
    rng = np.random.default_rng(SEED + ch)
    return [crafted(rng, n, ch, kind) for n, kind in CASES[ch]]


def yardstick():
    """-> (the largest |lufs_f32 - lufs_ref| in LU, the largest relative segment-energy error) of loudness_f32 against loudness_ref
    over the crafted tracks; segments whose energy is zero in both take no part in the second."""
    d_lufs = d_e = 0.0
    for ch in sorted(CASES):
        tracks = crafted_tracks(ch)
        for x, got in zip(tracks, loudness_f32(tracks, WEIGHTS[ch])):
            ref = loudness_ref(x, WEIGHTS[ch])
            assert (got.blocks, got.gated, got.peak) == (ref.blocks, ref.gated, ref.peak)
            if np.isfinite(ref.lufs):
                d_lufs = max(d_lufs, abs(got.lufs - ref.lufs))
            else:
                assert got.lufs == ref.lufs
            keep = ref.energies > 0
            if keep.any():
                d_e = max(d_e, float((np.abs(got.energies - ref.energies)[keep] / ref.energies[keep]).max()))
    return d_lufs, d_e


# ---- tests -------------------------------------------------------------------------------------------------
def sine(freq, dbfs, seconds, ch):
    t = np.arange(int(48000 * seconds)) / 48000.0
    return np.repeat(np.rint(32767 * 10 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * t)).astype(np.int16)[:, None], ch, axis=1)


def test_symbols_and_records(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "TRACK LOUDNESS" in hdr
    assert pkg.LOUDNESS_SPAN_DTYPE.itemsize == 16 and "opusgpu_loudness_span { /* 16 bytes" in hdr
    assert pkg.LOUDNESS_DTYPE.itemsize == 16 and "opusgpu_loudness { /* 16 bytes" in hdr
    assert pkg.LOUDNESS_REQ_DTYPE.itemsize == 48 and "opusgpu_loudness_req { /* 48 bytes" in hdr
    assert (pkg.LOUDNESS_OFF, pkg.LOUDNESS_MEASURE, pkg.LOUDNESS_NORMALIZE) == (0, 1, 2)
    for c in K1_B + K1_A[1:] + K2_A[1:]:
        assert repr(abs(c)) in hdr, c


@pytest.mark.parametrize("freq,dbfs,ch,want", [(1000, -23.0, 2, -23.0), (1000, -33.0, 2, -33.0), (997, 0.0, 1, -3.01)])
def test_known_answers_of_ebu_tech_3341(freq, dbfs, ch, want):
    got = loudness_ref(sine(freq, dbfs, 3, ch), WEIGHTS[ch])
    print(freq, dbfs, ch, got.lufs)
    assert abs(got.lufs - want) <= 0.1 and got.blocks == 27 == got.gated


def test_cases_the_definition_pins(pkg):
    rng = np.random.default_rng(5)
    silent = loudness_ref(np.zeros((48000, 2), np.int16), WEIGHTS[2])
    assert silent.lufs == -np.inf and silent.gated == 0 and silent.blocks == 7 and silent.peak == 0
    rec = np.zeros(1, dtype=pkg.LOUDNESS_DTYPE)
    rec[0] = (silent.lufs, silent.peak, silent.blocks, silent.gated)
    assert pkg.loudness_gain(rec[0], -23.0) == 1.0
    noise = rng.integers(-20000, 20001, (19200, 1)).astype(np.int16)
    assert loudness_ref(noise[:19199], [1]).blocks == 0 and loudness_ref(noise[:19199], [1]).lufs == -np.inf
    one = loudness_ref(noise, [1])
    assert one.blocks == 1 == one.gated and np.isfinite(one.lufs)
    assert loudness_ref(noise[:-1], [1]).peak == np.abs(noise[:-1].astype(np.int32)).max() / 32768
    # 5.1 (FL C FR RL RR LFE): the LFE alone is no loudness, and FL -> RL is 10 log10(1.41) more
    x = np.zeros((48000, 6), np.int16)
    x[:, 5] = sine(60, -6, 1, 1)[:, 0]
    lfe = loudness_ref(x, WEIGHTS[6])
    assert lfe.lufs == -np.inf and lfe.gated == 0 and lfe.peak > 0.5
    fl, rl = x.copy(), x.copy()
    tone = sine(500, -20, 1, 1)[:, 0]
    fl[:, 0], rl[:, 3] = tone, tone
    assert abs(loudness_ref(rl, WEIGHTS[6]).lufs - loudness_ref(fl, WEIGHTS[6]).lufs - 10 * np.log10(1.41)) < 1e-9


def test_gating_drops_the_quiet_blocks():
    """2 s at -36 dBFS, 6 s at -23 dBFS, 2 s at -36 dBFS: the quiet blocks fall to the relative gate, the six transition blocks
    stay in -- so the result is about -23.19, not -23.0, and the test holds the gate counts and the plain arithmetic."""
    x = np.concatenate([sine(1000, -36, 2, 2), sine(1000, -23, 6, 2), sine(1000, -36, 2, 2)])
    got = loudness_ref(x, WEIGHTS[2])
    print(got.lufs, got.blocks, got.gated, got.margin)
    assert (got.blocks, got.gated) == (97, 63) and got.margin > 0.01
    assert -23.3 < got.lufs < -23.1
    l = -0.691 + 10 * np.log10(got.powers)
    assert (l > -70).all()  # the absolute gate drops nothing here
    kept = np.sort(got.powers)[-63:]
    assert kept.min() > 0.1 * got.powers.mean() > np.sort(got.powers)[-64]
    assert abs(got.lufs - (-0.691 + 10 * np.log10(kept.mean()))) < 1e-12


def test_host_weights_and_gain(pkg):
    lib = pkg.load_lib()
    for ch in range(1, 9):
        assert np.array_equal(pkg.loudness_weights(ch), np.array(WEIGHTS[ch], dtype=np.float32)), ch
    for ch in (0, 9, -1):
        with pytest.raises(ValueError):
            pkg.loudness_weights(ch)
    rec = np.zeros(1, dtype=pkg.LOUDNESS_DTYPE)
    for lufs, peak, target, limit in ((-30.5, 0.25, -23.0, 1.0), (-30.5, 0.9, -23.0, 1.0), (-10.0, 1.0, -23.0, 1.0), (-40.0, 0.5, -16.0, 0.0),
                                      (-40.0, 0.5, -16.0, 0.89), (-np.inf, 0.3, -23.0, 1.0), (-23.0, 0.0, -23.0, 1.0)):
        rec[0] = (lufs, peak, 10, 5)
        lufs32, peak32 = float(np.float32(lufs)), float(np.float32(peak))
        want = 1.0
        if np.isfinite(lufs):
            want = 10 ** ((target - lufs32) / 20)
            if limit > 0 and peak32 * want > limit:
                want = limit / peak32
        got = pkg.loudness_gain(rec[0], target, limit)
        assert got == pytest.approx(want, rel=1e-14), (lufs, peak, target, limit)
        if limit > 0 and np.isfinite(lufs):
            assert peak32 * got <= limit * (1 + 1e-15)
    assert pkg.loudness_gain((-30.5, 0.9, 1, 1), -23.0) == pytest.approx(1 / float(np.float32(0.9)))  # the limit binds
    assert lib.opusgpu_loudness_gain(None, -23.0, 1.0) == 1.0
    # requests: what opusgpu_set_loudness refuses needs a context; its NULL checks do not
    assert lib.opusgpu_set_loudness(None, None) == pkg.OPUSGPU_BAD_ARG and lib.opusgpu_ms_set_loudness(None, None) == pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_last_loudness(None, 0, None, None) == pkg.OPUSGPU_BAD_ARG
    assert lib.opusgpu_tracks_loudness_device(None, 0, None, None, 2, None, None, None) == pkg.OPUSGPU_BAD_ARG


def test_the_request_of_decode_files(pkg, batch, ms_batch):
    """files_request with loudness=: the record, the call it means, and the refusals -- ValueError, no decoder anywhere."""
    assert pkg.files_request(batch).loudness is None and pkg.loudness_request(batch) is None
    m = pkg.files_request(batch, loudness="measure")
    assert (m.entry, m.kind, m.fmt) == ("files_decode", "tracks", pkg.TRACKS_S16)
    assert int(m.loudness["mode"][0]) == pkg.LOUDNESS_MEASURE and int(m.loudness["n_weights"][0]) == 0
    for b, multistream in ((batch, False), (ms_batch, True)):
        for fmt in ("f32", "f32_planar"):  # no int16 track in files_decode_as: the identity mix at 48 kHz, on the same grid
            plain = pkg.files_request(b, multistream, format=fmt)
            r = pkg.files_request(b, multistream, format=fmt, loudness=-23.0, peak_limit=0.5)
            assert plain.entry == "files_decode_as" and r.entry == "files_decode_mixed" and r.args[0] == 48000 and r.channels == b.channels
            assert np.array_equal(r.mix["m"][0, :b.channels, :b.channels], 16384 * np.eye(b.channels, dtype=np.int16))
            assert np.array_equal(r.offsets, plain.offsets) and np.array_equal(r.planes, plain.planes) and r.total == plain.total
            rec = r.loudness[0]
            assert (int(rec["mode"]), float(rec["target_lufs"]), float(rec["peak_limit"])) == (pkg.LOUDNESS_NORMALIZE, -23.0, 0.5)
            assert pkg.files_request(b, multistream, format=fmt, loudness="measure").entry == "files_decode_mixed"
    r = pkg.files_request(batch, rate=16000, mono=True, format="f32", loudness=-16, channel_weights=[1, 0.5])
    assert r.entry == "files_decode_resampled" and int(r.loudness["n_weights"][0]) == 2 and list(r.loudness["weights"][0, :3]) == [1, 0.5, 0]
    assert pkg.files_request(batch, features="logmel", mono=True, loudness=-23.0).entry == "files_decode_mel"
    assert pkg.files_request(ms_batch, True, mix="stereo", rate=16000, format="f32", loudness=-23.0).loudness is not None
    for kw in (dict(loudness=-23.0), dict(loudness=-23.0, format="s16"), dict(loudness=-23.0, rate=16000, mono=True),
               dict(loudness=-23.0, mix="mono"), dict(loudness=-23.0, resample=44100),            # an int16 result with a target
               dict(loudness="measure", channel_weights=[1, -1]), dict(loudness="measure", channel_weights=[1, np.nan]),
               dict(loudness="measure", channel_weights=[1, 1, 1]), dict(channel_weights=[1, 1]),  # a bad weight
               dict(loudness="loud"), dict(loudness=np.inf, format="f32"), dict(loudness=True, format="f32"),
               dict(loudness=-23.0, format="f32", peak_limit=np.nan)):
        with pytest.raises(ValueError):
            pkg.files_request(batch, **kw)


def test_kernels_hold_their_state_in_registers():
    """k_tracks_loudness_seg<C> for 1 - 8 channels: the 4 C words of a group, the 4 C state values and the C sums are indexed by
    literals only, so nothing lands in scratch, and a wave fits the 256 registers of one-wave workgroups at two waves per SIMD; the
    gate kernel's LDS is its two reduction arrays."""
    seen, gate_kernel = {}, None
    for mangled, v in _kernel_metadata().items():
        m = re.search(r"\d+k_tracks_loudness_segILi(\d+)E", mangled)
        if m:
            seen[int(m.group(1))] = v
        if re.search(r"\d+k_tracks_loudness_gate", mangled):
            gate_kernel = v
    print(seen, gate_kernel)
    assert sorted(seen) == list(range(1, 9))
    assert all(vgpr <= 256 and scratch == 0 and lds == 0 for vgpr, scratch, lds in seen.values()), seen
    assert gate_kernel is not None and gate_kernel[1] == 0 and gate_kernel[2] == 256 * 12


def test_crafted_tracks_keep_clear_of_the_gates():
    """What makes the GPU test's demand for equal gate counts fair: no block of a crafted track within 0.01 LU of either gate, and
    both gates drop blocks somewhere."""
    dropped_abs = dropped_rel = 0
    for ch in sorted(CASES):
        for (n, kind), x in zip(CASES[ch], crafted_tracks(ch)):
            ref = loudness_ref(x, WEIGHTS[ch])
            assert x.shape == (n, ch) and ref.margin > 0.01, (ch, n, kind, ref.margin)
            if ref.blocks:
                with np.errstate(divide="ignore"):
                    passed_abs = int((-0.691 + 10 * np.log10(ref.powers) > -70).sum())
                dropped_abs += ref.blocks - passed_abs
                dropped_rel += passed_abs - ref.gated
    assert dropped_abs > 50 and dropped_rel > 20


def test_the_yardstick_is_what_the_gpu_test_records():
    """loudness_f32 against loudness_ref over the crafted tracks: the constants of tests/test_gpu_tracks_loudness.py, and within
    what the standard allows by a wide margin."""
    import test_gpu_tracks_loudness as g
    d_lufs, d_e = yardstick()
    print(f"yardstick: lufs {d_lufs:.3g} LU, segment energy {d_e:.3g} relative")
    assert d_lufs == pytest.approx(g.YARDSTICK_LUFS, rel=0.02) and d_e == pytest.approx(g.YARDSTICK_ENERGY, rel=0.02)
    assert 8 * d_lufs < 0.1
