"""The directed corpus tests/golden/rare_paths.json ON THE GPU: packets written with a range encoder (tests/rc_craft.py) for the decode
branches random payloads never reach, decoded next to ordinary lcg_payloads streams of the same mode in batches of 256 streams --
four waves of the 64-frame parse kernels.  A corpus sequence may change its TOC from packet to packet (a SILK-only frame behind a
hybrid one runs the 2.5 ms CELT frame); entries are batched by their TOC sequence, and every step's ordinary streams carry that step's
TOC, the last one after a sequence has ended.

Lane placement: every corpus stream sits once at each of the stream indices = 0, 31, 32, 63 (mod 64) among ordinary neighbours (a
diverging lane at the half-wave seams), and in a second layout fills all 64 lanes of a wave (the branch wave-uniform; the waves
no entry of the batch fills hold ordinary streams, and a batch of four entries has none).
Routes: the device path step by step; the same steps as ONE pipelined window (set_pipeline(1)) with the step's mode mask declared,
so that the 64-frame parse kernels, k_silk_params and the tight synthesis twins carry them; the host path (decode_packets).
Compared with the oracle: every PCM sample and every return code on every route; the range decoder's final range after every
packet on all three routes (a queued run gives no state in between, so the device and the pipelined route run every prefix of
the steps as a run of its own).  Stage taps (opusgpu_debug_stage_taps) of every corpus stream against the oracle's, as
tests/test_gpu_stage_taps.py compares them, so that a difference names a kernel.  Every test first asserts that the oracle's
result for each corpus packet is the one recorded in the fixture.
"""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

from test_gpu_pipeline import run_queued

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = json.load(open(os.path.join(ROOT, "tests", "golden", "rare_paths.json")))
N, SEAMS, FILL_LEN = 256, (0, 31, 32, 63), 60


def _groups(corpus=CORPUS):
    """corpus entries by (TOC sequence, decoder channels), four at a time: one batch each.  (The helpers and the two test bodies take
    the corpus as a parameter: tests/test_gpu_saturation_paths.py runs them over its own.)"""
    by = {}
    for i, e in enumerate(corpus["entries"]):
        by.setdefault((tuple(int(p[:2], 16) for p in e["packets"]), e["channels"]), []).append(i)
    return [(tocs, ch, ids[k:k + 4]) for (tocs, ch), ids in sorted(by.items()) for k in range(0, len(ids), 4)]


GROUPS = _groups()
IDS = [f"toc{'_'.join('%02x' % t for t in tocs)}-ch{ch}-e{'_'.join(map(str, ids))}" for tocs, ch, ids in GROUPS]


def _batch(pkg, tocs, ids, layout, corpus=CORPUS):
    """-> packets[frame][stream] (bytes), owner[stream] = corpus entry or -1, the TOC of every step"""
    ents = [corpus["entries"][i] for i in ids]
    tocs = list(tocs) + [tocs[-1]]  # (+ 1 step: an ordinary packet on the state the corpus packets leave)
    frames = len(tocs)
    pay = pkg.lcg_payloads(N, frames, FILL_LEN, seed_base=0x4A2E + tocs[0])
    pk = [[bytes([tocs[f]]) + pay[f, s].tobytes() for s in range(N)] for f in range(frames)]
    owner = [-1] * N
    for j, e in enumerate(ents):
        if layout == "seams":
            where = [64 * ((j + k) % 4) + SEAMS[k] for k in range(4)]
        else:
            where = range(64 * j, 64 * j + 64)
        for s in where:
            assert owner[s] == -1
            owner[s] = ids[j]
            for f, hx in enumerate(e["packets"]):
                pk[f][s] = bytes.fromhex(hx)
    return pk, owner, tocs


def _oracle(oracle, channels, pk, owner, corpus=CORPUS):
    frames = len(pk)
    pcm = np.zeros((frames, N, 960 * channels), dtype=np.int16)
    rets = np.zeros((frames, N), dtype=np.int32)
    rngs = np.zeros((frames, N), dtype=np.uint32)
    d = oracle.decoder(channels)
    for s in range(N):
        d.init()
        for f in range(frames):
            ref, r = d.decode(pk[f][s])
            rets[f, s], rngs[f, s] = r, oracle.lib.oc_decoder_final_range(d.h)
            if r > 0:
                pcm[f, s] = ref[:960].reshape(-1)
            if owner[s] >= 0 and f < len(corpus["entries"][owner[s]]["packets"]):  # no comparison of nothing
                exp = corpus["entries"][owner[s]]["expect"][f]
                assert [r, int(rngs[f, s]), zlib.crc32(ref[:max(r, 0)].tobytes())] == exp, ("the oracle moved", owner[s], f)
    return pcm, rets, rngs


def _arena(pk):
    frames = len(pk)
    lens = np.array([[len(p) for p in row] for row in pk], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens.reshape(-1))[:-1]]).reshape(frames, N)
    arena = np.frombuffer(b"".join(p for row in pk for p in row) + bytes(16), dtype=np.uint8).copy()
    return arena, offs, lens


def _final_ranges(ctx):
    head = (C.c_int32 * 4)()
    out = np.zeros(N, dtype=np.uint32)
    for s in range(N):
        assert ctx.lib.opusgpu_stream_state_get(ctx.h, s, head, 16) == 0
        out[s] = head[3] & 0xFFFFFFFF
    return out


def _same(pcm, res, ref, rets, what):
    assert (res == rets).all(), (what, "return codes", np.argwhere(res != rets)[:4].tolist())
    ok = rets == 960
    assert ok.any()
    bad = (pcm != ref).any(axis=-1) & ok
    assert not bad.any(), (what, "PCM of (frame, stream)", np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("layout", ["seams", "wave"])
@pytest.mark.parametrize("toc_seq, channels, ids", GROUPS, ids=IDS)
def test_corpus_streams_on_three_routes(pkg, oracle, gpu_ctx, toc_seq, channels, ids, layout):
    streams_on_three_routes(CORPUS, pkg, oracle, gpu_ctx, toc_seq, channels, ids, layout)


def streams_on_three_routes(corpus, pkg, oracle, ctx, toc_seq, channels, ids, layout):
    pk, owner, step_toc = _batch(pkg, toc_seq, ids, layout, corpus)
    frames = len(pk)
    ref, rets, rngs = _oracle(oracle, channels, pk, owner, corpus)
    arena, offs, lens = _arena(pk)
    tocs = np.repeat(np.array(step_toc, dtype=np.uint8)[:, None], N, axis=1)
    masks = {pkg.toc_modes(t) for t in step_toc}
    modes = masks.pop() if len(masks) == 1 else 0  # declared where the window is single-mode
    # ---- the device path, step by step, the final range after every packet
    pcm, res = run_queued(pkg, ctx, channels, arena, offs, lens - 1, tocs, pipeline=False)
    _same(pcm, res, ref, rets, "device path")
    assert (_final_ranges(ctx) == rngs[-1]).all(), "device path: final range after the last packet"
    for f in range(frames - 1):  # ... and after every earlier packet: the first f + 1 steps alone (run_queued starts from fresh streams)
        run_queued(pkg, ctx, channels, arena, offs[:f + 1], lens[:f + 1] - 1, tocs[:f + 1], pipeline=False)
        assert (_final_ranges(ctx) == rngs[f]).all(), ("device path: final range after packet", f)
    # ---- one pipelined window with the mode mask declared
    pcm, res = run_queued(pkg, ctx, channels, arena, offs, lens - 1, tocs, pipeline=True, window=True, modes=modes)
    _same(pcm, res, ref, rets, "pipelined window")
    assert (_final_ranges(ctx) == rngs[-1]).all(), "pipelined window: final range after the last packet"
    for f in range(frames - 1):  # ... and after every earlier packet: the first f + 1 steps as a window of their own
        masks = {pkg.toc_modes(t) for t in step_toc[:f + 1]}
        run_queued(pkg, ctx, channels, arena, offs[:f + 1], lens[:f + 1] - 1, tocs[:f + 1], pipeline=True, window=True,
                   modes=masks.pop() if len(masks) == 1 else 0)
        assert (_final_ranges(ctx) == rngs[f]).all(), ("pipelined window: final range after packet", f)
    # ---- the host path
    ctx.streams_alloc(N, channels)
    for f in range(frames):
        p, r = ctx.decode_packets(np.arange(N), pk[f])
        _same(np.asarray(p).reshape(1, N, -1)[:, :, :960 * channels], np.asarray(r).reshape(1, N), ref[f:f + 1], rets[f:f + 1], ("host path", f))
        assert (_final_ranges(ctx) == rngs[f]).all(), ("host path: final range after packet", f)


def _otap(oracle, d, what, c, dtype, count):
    buf = np.zeros(count, dtype=dtype)
    oracle.lib.oc_taps_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert oracle.lib.oc_taps_copy(d.h, what, c, buf.ctypes.data) == buf.nbytes
    return buf


@pytest.mark.parametrize("toc_seq, channels, ids", GROUPS, ids=IDS)
def test_corpus_stage_taps(pkg, oracle, gpu_ctx, toc_seq, channels, ids):
    """CELT: record header, energies, pulses, tf_res, synthesis output after the comb filter, overlap tail.  SILK: gains, both LPC
    sets, LTP taps, the core output."""
    stage_taps(CORPUS, pkg, oracle, gpu_ctx, toc_seq, channels, ids)


def stage_taps(corpus, pkg, oracle, ctx, toc_seq, channels, ids):
    pk, owner, step_toc = _batch(pkg, toc_seq, ids, "seams", corpus)
    frames = len(pk)
    arena, offs, lens = _arena(pk)
    ctx.streams_alloc(N, channels)
    ctx.set_pipeline(False)
    mine = [s for s in range(N) if owner[s] >= 0]
    oracle.lib.oc_taps_enable.argtypes = [C.c_void_p]
    oracle.lib.oc_silk_taps_copy.argtypes = [C.c_int, C.c_int, C.c_void_p]
    oracle.lib.oc_silk_taps_enable.argtypes = [C.c_int]
    decs = {}
    for s in mine:
        decs[s] = oracle.decoder(channels)
        decs[s].init()
        assert oracle.lib.oc_taps_enable(decs[s].h)
    d_arena, d_desc = ctx.dev_alloc(arena.size), ctx.dev_alloc(16 * N)
    d_pcm, d_res = ctx.dev_alloc(N * 960 * channels * 2), ctx.dev_alloc(4 * N)
    ctx.h2d(d_arena, arena)
    descs = np.zeros(N, dtype=pkg.DESC_DTYPE)
    descs["stream"] = np.arange(N, dtype=np.int32)
    from test_gpu_pipeline import desc_flags
    oracle.lib.oc_silk_taps_enable(1)
    try:
        for f in range(frames):
            toc = step_toc[f]
            celt, silk, hybrid = bool(toc & 0x80), not (toc & 0x80), (toc & 0xE0) == 0x60
            descs["offset"] = (offs[f] + 1).astype(np.int32)
            descs["len"] = (lens[f] - 1).astype(np.int32)
            descs["flags"] = desc_flags(np.full(N, toc, dtype=np.uint8))[0]
            ctx.h2d(d_desc, descs)
            ctx.decode_step_device(N, d_desc, d_arena, d_pcm, d_res)
            ctx.synchronize()
            for s in mine:
                ref, r = decs[s].decode(pk[f][s])  # (the SILK taps are those of this call)
                if f < len(corpus["entries"][owner[s]]["packets"]):
                    exp = corpus["entries"][owner[s]]["expect"][f]
                    assert [r, oracle.lib.oc_decoder_final_range(decs[s].h), zlib.crc32(ref[:max(r, 0)].tobytes())] == exp
                if r != 960:
                    continue
                t = ctx.debug_stage_taps(s)
                where = (hex(toc), f, s, owner[s])
                if celt:
                    h = _otap(oracle, decs[s], 4, 0, np.int32, 75)
                    assert t.celt_valid and t.celt_ret == 960, where
                    got = (t.transient, t.silence, t.intensity, t.dual_stereo, t.spread, t.lm, t.pf_pitch, t.pf_gain, t.pf_tapset, t.anti_collapse_on)
                    assert got == tuple(int(h[k]) for k in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10)), ("parse record header", where)
                    assert t.celt_rng_final == np.uint32(h[11]), ("range coder state after the frame", where)
                    assert (np.array(t.pulses) == h[12:33]).all(), ("pulses", where)
                    assert (np.array(t.tf_res) == h[54:75]).all(), ("tf_res", where)
                    nE = 21 * (2 if toc & 4 else 1)
                    assert (np.array(t.bandE)[:nE] == _otap(oracle, decs[s], 1, 0, np.int16, 42)[:nE]).all(), ("band energies", where)
                    for c in range(channels):
                        assert (np.array(t.syn_post[c]) == _otap(oracle, decs[s], 3, c, np.int32, 960)).all(), ("synthesis after the comb filter", c, where)
                        assert (np.array(t.overlap_tail[c]) == _otap(oracle, decs[s], 2, c, np.int32, 1080)[960:1020]).all(), ("overlap tail", c, where)
                if hybrid:  # the CELT layer's record (bands 17..20): k_celt_parse
                    h = _otap(oracle, decs[s], 4, 0, np.int32, 75)
                    assert t.celt_valid and t.celt_ret == 960, where
                    assert (t.transient, t.silence, t.spread, t.lm) == (h[0], h[1], h[5], h[6]), ("hybrid: CELT header", where)
                    assert (np.array(t.pulses)[17:] == h[12 + 17:33]).all(), ("hybrid: pulses", where)
                    assert t.celt_rng_final == np.uint32(h[11]), ("hybrid: range coder state after the frame", where)
                if silk:
                    assert t.silk_valid and t.silk_ret == 0, where
                    for ch in range(2 if toc & 4 else 1):
                        def st(what, dtype, count):
                            b = np.zeros(count, dtype=dtype)
                            assert oracle.lib.oc_silk_taps_copy(what, ch, b.ctypes.data) >= 0
                            return b
                        sb = st(0, np.int32, 6)
                        if not sb[0]:
                            continue
                        flen, order, k = int(sb[3]), int(sb[4]), t.silk_ch[ch]
                        assert (k.signalType, k.quantOffsetType, k.LTP_scale_Q14) == (sb[1], sb[2], sb[5]), ("signal type / LTP scale", where)
                        b = st(1, np.int32, 8)
                        assert (np.array(k.pitchL) == b[:4]).all() and (np.array(k.Gains_Q16) == b[4:]).all(), ("pitch lags / gains", where)
                        b = st(2, np.int16, 32).reshape(2, 16)
                        assert (np.array(k.PredCoef_Q12).reshape(2, 16)[:, :order] == b[:, :order]).all(), ("LPC coefficients", where)
                        assert (np.array(k.LTPCoef_Q14) == st(3, np.int16, 20)).all(), ("LTP coefficients", where)
                        assert (np.array(t.silk_out[ch])[:flen] == st(4, np.int16, 320)[:flen]).all(), ("synthesis core output", where)
    finally:
        oracle.lib.oc_silk_taps_enable(0)
        for p in (d_arena, d_desc, d_pcm, d_res):
            ctx.dev_free(p)
