"""The directed corpus tests/golden/kernel_paths.json ON THE GPU: the frames that take the branch sides of the kernel source which nothing
else the suite decodes takes (tools/kernel_branches.py measures that in host emulation; tests/test_kernel_paths.py is the CPU half).

Reference-mode entries run through the machinery of tests/test_gpu_rare_paths.py: batches of 256 streams, every corpus stream at
stream indices 0, 31, 32 and 63 (mod 64) among lcg_payloads neighbours ("seams") and, in a second layout, filling a whole wave
("wave"); the device path step by step, one pipelined window with the mode mask declared, the host path; every PCM sample, every
return code and the final range after every packet against the oracle, and the stage taps so that a difference names a kernel.

RFC entries (an empty packet is a loss, "fec" lists the packets before which decode_fec is asked for) run in batches of 256 streams in
set_mode(True) through decode_packets / decode_packets_fec with frame_capacity = 6; every stream -- corpus streams and their
lcg_payloads neighbours, which carry the entry's TOC byte per step -- is checked against its own oracle decoder in RFC mode over
the domain rfc_common.same_pcm defines (rfc_common.oracle_step / same_step, any frame count and duration), with return codes, the
final range, and the recorded `expect` for corpus streams.  The corpus holds RFC entries only where a side needs RFC mode (none at
present), so the same body also runs over the RFC entries of tests/golden/saturation_paths.json, and once with decode_fec.

The frames that are NOT for the kernel of 20 ms frames: the census shows that a frame with leaves is always fast (the record limits
cannot be exceeded: tests/test_kernel_paths.py), so the only frames k_celt_recon takes in its role RECON_REST_ONLY are CELT
frames of at most one byte (celt_decode_frame's early CELT_BAD_ARG: a record without leaves).  They get a test of their own: in a
pipelined CELT window, at the seams of a wave and filling one, among fast neighbours, with the frames behind them.
"""
import json
import os
import zlib

import numpy as np
import pytest

import rfc_common as rc
import test_gpu_rare_paths as rp
from test_gpu_pipeline import run_queued

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_paths.json")))
REFERENCE = {"entries": [e for e in CORPUS["entries"] if not e.get("rfc")]}
LOSSY = [e for e in CORPUS["entries"] if e.get("rfc")]
N = rp.N


def _ids(groups):
    return [f"toc{'_'.join('%02x' % t for t in tocs)}-ch{ch}-e{'_'.join(map(str, ids))}" for tocs, ch, ids in groups]


GROUPS = rp._groups(REFERENCE)


def test_the_corpus_is_what_the_batches_hold():
    """(no GPU work) every entry is in exactly one batch; a batch is 256 streams x at most 8 corpus packets and one more step"""
    assert sorted(i for _, _, ids in GROUPS for i in ids) == list(range(len(REFERENCE["entries"])))
    assert sorted(i for _, _, ids in LOSSY_GROUPS for i in ids) == list(range(len(LOSSY)))
    assert all(1 <= len(tocs) <= 8 and len(ids) <= 4 for tocs, _, ids in GROUPS)
    assert len(REFERENCE["entries"]) + len(LOSSY) == len(CORPUS["entries"]) > 0


@pytest.mark.parametrize("layout", ["seams", "wave"])
@pytest.mark.parametrize("toc_seq, channels, ids", GROUPS, ids=_ids(GROUPS))
def test_kernel_path_streams_on_three_routes(pkg, oracle, gpu_ctx, toc_seq, channels, ids, layout):
    rp.streams_on_three_routes(REFERENCE, pkg, oracle, gpu_ctx, toc_seq, channels, ids, layout)


@pytest.mark.parametrize("toc_seq, channels, ids", GROUPS, ids=_ids(GROUPS))
def test_kernel_path_streams_stage_taps(pkg, oracle, gpu_ctx, toc_seq, channels, ids):
    rp.stage_taps(REFERENCE, pkg, oracle, gpu_ctx, toc_seq, channels, ids)


# ---- RFC mode ------------------------------------------------------------------------------------------------------------------------
def _lossy_groups(entries):
    """rfc entries by (decoder channels, first byte or loss per step, fec marks), four at a time"""
    by = {}
    for i, e in enumerate(entries):
        steps = tuple(int(p[:2], 16) if p else -1 for p in e["packets"])
        by.setdefault((e["channels"], steps, tuple(e.get("fec") or ())), []).append(i)
    return [(ch, steps, fec, ids[k:k + 4]) for (ch, steps, fec), ids in sorted(by.items()) for k in range(0, len(ids), 4)]


LOSSY_GROUPS = _lossy_groups(LOSSY)


def rfc_streams(entries, pkg, oracle, ctx, channels, steps, fec, ids, layout, recorded=True):
    """Every stream of the batch decodes the step's TOC byte (frame-count code 0 for the neighbours: one frame of the TOC's
    duration) or loses the step's packet; before the steps listed in `fec` every stream recovers the packet before from the
    step's packet.  recorded: the entries' `expect` is this run's (no decode_fec was added)."""
    ents = [entries[i] for i in ids]
    frames = len(steps)
    pay = pkg.lcg_payloads(N, frames, rp.FILL_LEN, seed_base=0x6B1 + (steps[0] & 0xFF))
    pk = [[(bytes([steps[f] & 0xFC]) + pay[f, s].tobytes()) if steps[f] >= 0 else b"" for s in range(N)] for f in range(frames)]
    owner = [-1] * N
    for j, e in enumerate(ents):
        where = [64 * ((j + k) % 4) + rp.SEAMS[k] for k in range(4)] if layout == "seams" else range(64 * j, 64 * j + 64)
        for s in where:
            assert owner[s] == -1
            owner[s] = j
            for f, hx in enumerate(e["packets"]):
                pk[f][s] = bytes.fromhex(hx)
    decs, last = [], [None] * N
    for s in range(N):
        d = oracle.decoder(channels)
        d.init()
        d.set_rfc(True)
        decs.append(d)
    ctx.set_mode(True)
    try:
        ctx.streams_alloc(N, channels)
        for f in range(frames):
            who = [s for s in range(N) if f in fec and pk[f][s] and rc.frame_payloads(oracle, pk[f][s]) is not None]
            if who:
                pcm, res = ctx.decode_packets_fec(np.array(who), [pk[f][s] for s in who], frame_capacity=6)
                for j, s in enumerate(who):
                    ref, r, spans, before = rc.oracle_fec_step(oracle, decs[s], pk[f][s], last[s], channels)
                    bad = rc.same_fec_step(pcm[j], res[j], ref, r, spans, before, channels)
                    assert bad is None, (f, s, hex(pk[f][s][0]), bad)
            pcm, res = ctx.decode_packets(np.arange(N), pk[f], frame_capacity=6)
            rng = rp._final_ranges(ctx)
            for s in range(N):
                ref, r, domain, last[s] = rc.oracle_step(oracle, decs[s], pk[f][s], last[s], channels)
                want_rng = oracle.lib.oc_decoder_final_range(decs[s].h)
                where = (f, s, "lost" if not pk[f][s] else hex(pk[f][s][0]), "corpus entry %d" % ids[owner[s]] if owner[s] >= 0 else "neighbour")
                if owner[s] >= 0 and recorded:
                    exp = ents[owner[s]]["expect"][f]
                    assert [r, want_rng, zlib.crc32(ref[:max(r, 0)].tobytes())] == exp, ("the oracle moved", where)
                bad = rc.same_step(pcm[s], res[s], ref, r, domain, channels)
                assert bad is None, (where, bad)
                assert int(rng[s]) == want_rng, ("final range", where)
    finally:
        ctx.set_mode(False)


SATURATION_LOSSY = [e for e in json.load(open(os.path.join(ROOT, "tests", "golden", "saturation_paths.json")))["entries"] if e["rfc"]]
# (where, entries, group, is `expect` the sequence's own?): the corpus's RFC entries -- it holds some only where a side needs RFC mode --
# and, so that the comparison always runs, those of the saturation corpus: as recorded, and the first group once more with
# decode_fec asked for before its first packet behind the first (the oracle then moves off the recorded results)
RFC_RUNS = [("kernel", LOSSY, g, True) for g in LOSSY_GROUPS] + [("saturation", SATURATION_LOSSY, g, True) for g in _lossy_groups(SATURATION_LOSSY)]
_g = RFC_RUNS[-len(_lossy_groups(SATURATION_LOSSY))][2]
RFC_RUNS.append(("saturation-fec", SATURATION_LOSSY, (_g[0], _g[1], (next(k for k in range(1, len(_g[1])) if _g[1][k] >= 0),), _g[3]), False))


@pytest.mark.parametrize("layout", ["seams", "wave"])
@pytest.mark.parametrize("where, entries, group, recorded", RFC_RUNS,
                         ids=[f"{w}-ch{g[0]}-{'_'.join('lost' if t < 0 else '%02x' % t for t in g[1])}-e{'_'.join(map(str, g[3]))}"
                              for w, _, g, _ in RFC_RUNS])
def test_kernel_path_streams_in_rfc_mode(pkg, oracle, gpu_ctx, where, entries, group, recorded, layout):
    rfc_streams(entries, pkg, oracle, gpu_ctx, *group, layout, recorded=recorded)


# ---- the frames the general reconstruction kernel takes in a pipelined CELT window ---------------------------------------------------------
TOC, L, FRAMES = 0xFC, 160, 4


@pytest.mark.parametrize("route", ["in_order", "window"])
def test_frames_that_are_not_fast_among_fast_neighbours(pkg, oracle, gpu_ctx, route):
    """CELT frames of 0 and 1 payload bytes: recon_fast_eligible is false for them (RF_BAD_CELT), so in a pipelined CELT window
    k_celt_recon_fb leaves them (RECON_NOT_MINE) and k_celt_recon takes them in its role RECON_REST_ONLY.  Wave 0 has them at
    stream indices 0, 31, 32 and 63 in steps 1 and 2, wave 1 is full of them in step 1, wave 2 has one in every step but the last at its
    stream 7, wave 3 has none.  Every return code, the PCM of every frame that decodes -- the frames behind a refused one among them: it
    must have left the stream's CELT state alone -- and the final range after the window, against the oracle."""
    pay = pkg.lcg_payloads(N, FRAMES, L, seed_base=0x7E57F000)
    pk = [[bytes([TOC]) + pay[f, s].tobytes() for s in range(N)] for f in range(FRAMES)]
    short = {(1, s): 1 for s in rp.SEAMS}
    short.update({(2, s): 0 for s in rp.SEAMS})
    short.update({(1, s): (s & 1) for s in range(64, 128)})
    short.update({(f, 128 + 7): (f & 1) for f in range(FRAMES - 1)})
    for (f, s), n in short.items():
        pk[f][s] = pk[f][s][:1 + n]
    ref = np.zeros((FRAMES, N, 960 * 2), dtype=np.int16)
    rets = np.zeros((FRAMES, N), dtype=np.int32)
    rngs = np.zeros(N, dtype=np.uint32)
    d = oracle.decoder(2)
    for s in range(N):
        d.init()
        for f in range(FRAMES):
            out, r = d.decode(pk[f][s])
            rets[f, s] = r
            if r > 0:
                ref[f, s] = out[:960].reshape(-1)
        rngs[s] = oracle.lib.oc_decoder_final_range(d.h)
    assert all(rets[f, s] < 0 for f, s in short) and (rets < 0).sum() == len(short)  # (the oracle refuses exactly these)
    arena, offs, lens = rp._arena(pk)
    tocs = np.full((FRAMES, N), TOC, dtype=np.uint8)
    how = dict(pipeline=False) if route == "in_order" else dict(pipeline=True, window=True, modes=pkg.toc_modes(TOC))
    pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens - 1, tocs, **how)
    assert (res == rets).all(), (route, "return codes of (frame, stream)", np.argwhere(res != rets)[:4].tolist())
    bad = (pcm != ref).any(axis=-1) & (rets == 960)
    assert not bad.any(), (route, "PCM of (frame, stream)", np.argwhere(bad)[:8].tolist())
    assert (rp._final_ranges(gpu_ctx) == rngs).all(), (route, "final range after the last step")
