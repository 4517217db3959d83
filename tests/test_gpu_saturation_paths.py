"""The directed corpus tests/golden/saturation_paths.json ON THE GPU: frames whose LPC synthesis update -- add_sat32(residual,
lshift_sat32(prediction, 4)) -- saturates hundreds of times on either side, on every sample index mod 4 of the row form's trip,
in the first and the last subframe and on the first sample behind a saturated history (tests/test_saturation_paths.py checks
that from the oracle's census), and the frames that clamp the other rarely clamped helpers.  The machinery is that of
tests/test_gpu_rare_paths.py, run over this corpus: batches of 256 streams, every corpus stream at stream indices 0, 31, 32
and 63 (mod 64) among ordinary lcg_payloads neighbours and, in a second layout, filling a whole wave; the device path step by
step, one pipelined window with the mode mask declared, the host path; every PCM sample, every return code and the final
range after every packet against the oracle; SILK stage taps so that a difference names a kernel (taken, as there, on the
step-by-step route: a difference in the pipelined route's kernels alone shows as PCM).

Which kernel a saturating frame runs through (the entry's "class" names its frame):
  * k_silk_synth (og_silk_synth.hip), the row form of the recurrence: the MB, WB and hybrid classes on the pipelined route;
  * its narrowband twin (og_silk_nb.hip): the NB classes on the pipelined route;
  * the hybrid step: the hybrid classes, whose CELT layer is decoded off the noise behind the SILK layer;
  * k_decode_step's single-kernel code: every class on the step-by-step and the host route, the "-in-stereo-decoder" entries
    (a mono packet in a stereo decoder) among them.  On the GPU that code, too, takes decoded frames through the row form; the
    one-lane core (silk_decode_core_lane) runs there only for a decoded channel beside a concealed one (forward error
    correction with one channel's copy missing), which the frame writer cannot produce -- that core is compared on the
    corpus in host emulation (tests/test_saturation_paths.py);
  * k_decode_rfc with the lost packets behind the frames (the concealment's synthesis update and its output, the comfort
    noise's, CELT's pitch-based concealment, the mix of the concealed layers): the entries marked rfc, through set_mode(True)
    and decode_packets against the oracle's RFC mode and its concealment.
"""
import json
import os
import zlib

import numpy as np
import pytest

import rfc_common as rc
import test_gpu_rare_paths as rp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = json.load(open(os.path.join(ROOT, "tests", "golden", "saturation_paths.json")))
REFERENCE = {"entries": [e for e in CORPUS["entries"] if not e["rfc"]]}  # what the reference-mode machinery reads of a corpus
LOSSY = [e for e in CORPUS["entries"] if e["rfc"]]
N = rp.N


def _ids(groups):
    return [f"toc{'_'.join('%02x' % t for t in tocs)}-ch{ch}-e{'_'.join(map(str, ids))}" for tocs, ch, ids in groups]


def _half(tocs, ch):
    """a mono SILK-only packet in a stereo decoder defines only the first 960 entries of its 1920"""
    return ch == 2 and all(not (t & 0x84) and (t & 0x60) != 0x60 for t in tocs)


GROUPS = rp._groups(REFERENCE)
FULL_GROUPS = [g for g in GROUPS if not _half(g[0], g[1])]
HALF_GROUPS = [g for g in GROUPS if _half(g[0], g[1])]


def test_the_batches_hold_a_saturating_frame_for_every_kernel():
    """(no GPU work: the parametrisation below covers what the module's docstring lists)"""
    classes = {REFERENCE["entries"][i].get("class"): (tocs, ch) for tocs, ch, ids in GROUPS for i in ids}
    for band, toc in (("nb", 0x08), ("mb", 0x28), ("wb", 0x48), ("hybrid", 0x78)):
        for voicing in ("unvoiced", "voiced"):
            assert classes[f"{band}-{voicing}-mono"] == ((toc,) * 3, 1) and classes[f"{band}-{voicing}-stereo"] == ((toc | 4,) * 3, 2)
    assert classes["nb-voiced-mono-in-stereo-decoder"] == ((0x08,) * 3, 2) and classes["wb-unvoiced-mono-in-stereo-decoder"] == ((0x48,) * 3, 2)
    assert len([e for e in LOSSY if e.get("class", "").endswith("-lossy")]) == 16


@pytest.mark.parametrize("layout", ["seams", "wave"])
@pytest.mark.parametrize("toc_seq, channels, ids", FULL_GROUPS, ids=_ids(FULL_GROUPS))
def test_saturating_streams_on_three_routes(pkg, oracle, gpu_ctx, toc_seq, channels, ids, layout):
    rp.streams_on_three_routes(REFERENCE, pkg, oracle, gpu_ctx, toc_seq, channels, ids, layout)


@pytest.mark.parametrize("layout", ["seams", "wave"])
@pytest.mark.parametrize("toc_seq, channels, ids", HALF_GROUPS, ids=_ids(HALF_GROUPS))
def test_saturating_mono_packets_in_a_stereo_decoder_on_three_routes(pkg, oracle, gpu_ctx, toc_seq, channels, ids, layout):
    """the same three routes over the entries whose packets define half of their output: the defined 960 entries, every return code,
    the final range after the last packet"""
    ctx = gpu_ctx
    pk, owner, step_toc = rp._batch(pkg, toc_seq, ids, layout, REFERENCE)
    ref, rets, rngs = rp._oracle(oracle, channels, pk, owner, REFERENCE)
    arena, offs, lens = rp._arena(pk)
    tocs = np.repeat(np.array(step_toc, dtype=np.uint8)[:, None], N, axis=1)
    masks = {pkg.toc_modes(t) for t in step_toc}
    assert len(masks) == 1
    for what, how in (("device path", dict(pipeline=False)), ("pipelined window", dict(pipeline=True, window=True, modes=masks.pop()))):
        pcm, res = rp.run_queued(pkg, ctx, channels, arena, offs, lens - 1, tocs, **how)
        rp._same(pcm[:, :, :960], res, ref[:, :, :960], rets, what)
        assert (rp._final_ranges(ctx) == rngs[-1]).all(), (what, "final range after the last packet")
    ctx.streams_alloc(N, channels)
    for f in range(len(pk)):
        p, r = ctx.decode_packets(np.arange(N), pk[f])
        rp._same(np.asarray(p).reshape(1, N, -1)[:, :, :960], np.asarray(r).reshape(1, N), ref[f:f + 1, :, :960], rets[f:f + 1], ("host path", f))
        assert (rp._final_ranges(ctx) == rngs[f]).all(), ("host path: final range after packet", f)


@pytest.mark.parametrize("toc_seq, channels, ids", GROUPS, ids=_ids(GROUPS))
def test_saturating_streams_stage_taps(pkg, oracle, gpu_ctx, toc_seq, channels, ids):
    rp.stage_taps(REFERENCE, pkg, oracle, gpu_ctx, toc_seq, channels, ids)


# ---- RFC mode: the frames with the lost packets behind them ---------------------------------------------------------------------------
def _lossy_groups():
    """rfc entries by (decoder channels, TOC or loss per step), four at a time"""
    by = {}
    for i, e in enumerate(LOSSY):
        by.setdefault((e["channels"], tuple(int(p[:2], 16) if p else -1 for p in e["packets"])), []).append(i)
    return [(ch, steps, ids[k:k + 4]) for (ch, steps), ids in sorted(by.items()) for k in range(0, len(ids), 4)]


LOSSY_GROUPS = _lossy_groups()
LOSSY_IDS = [f"ch{ch}-{'_'.join('lost' if t < 0 else '%02x' % t for t in steps)}-e{'_'.join(map(str, ids))}" for ch, steps, ids in LOSSY_GROUPS]


@pytest.mark.parametrize("layout", ["seams", "wave"])
@pytest.mark.parametrize("channels, steps, ids", LOSSY_GROUPS, ids=LOSSY_IDS)
def test_saturating_streams_and_their_losses_in_rfc_mode(pkg, oracle, gpu_ctx, channels, steps, ids, layout):
    """k_decode_rfc: every stream of the batch decodes the step's TOC (20 ms, one frame) or loses the step's packet; the corpus
    streams sit among lcg_payloads neighbours as in the reference-mode batches"""
    ctx = gpu_ctx
    ents = [LOSSY[i] for i in ids]
    frames = len(steps)
    assert all(t < 0 or (t & 3) == 0 for t in steps)
    pay = pkg.lcg_payloads(N, frames, rp.FILL_LEN, seed_base=0x5A7 + (steps[0] & 0xFF))
    pk = [[(bytes([steps[f]]) + pay[f, s].tobytes()) if steps[f] >= 0 else b"" for s in range(N)] for f in range(frames)]
    owner = [-1] * N
    for j, e in enumerate(ents):
        where = [64 * ((j + k) % 4) + rp.SEAMS[k] for k in range(4)] if layout == "seams" else range(64 * j, 64 * j + 64)
        for s in where:
            assert owner[s] == -1
            owner[s] = j
            for f, hx in enumerate(e["packets"]):
                pk[f][s] = bytes.fromhex(hx)
    decs = []
    for s in range(N):
        d = oracle.decoder(channels)
        d.init()
        d.set_rfc(True)
        decs.append(d)
    last = [None] * N  # (rfc_common.oracle_step: what a stream's lost packet is concealed like)
    ctx.set_mode(True)
    try:
        ctx.streams_alloc(N, channels)
        for f in range(frames):
            pcm, res = ctx.decode_packets(np.arange(N), pk[f], frame_capacity=6)
            rng = rp._final_ranges(ctx)
            for s in range(N):
                ref, r, domain, last[s] = rc.oracle_step(oracle, decs[s], pk[f][s], last[s], channels)
                want_rng = oracle.lib.oc_decoder_final_range(decs[s].h)
                if owner[s] >= 0:
                    exp = ents[owner[s]]["expect"][f]
                    assert [r, want_rng, zlib.crc32(ref[:max(r, 0)].tobytes())] == exp, ("the oracle moved", ids[owner[s]], f)
                where = (f, s, "lost" if not pk[f][s] else hex(pk[f][s][0]), "corpus entry %d" % ids[owner[s]] if owner[s] >= 0 else "neighbour")
                assert res[s] == r == 960, ("return code", where, int(res[s]), r)
                assert int(rng[s]) == want_rng, ("final range", where)
                assert rc.same_step(pcm[s], res[s], ref, r, domain, channels) is None, ("over the entries the packet defines", where)
                got, want = np.asarray(pcm[s])[:960].reshape(-1), ref[:960].reshape(-1)
                bad = np.argwhere(got != want)
                assert not len(bad), ("PCM", where, "first differing entries", bad[:4].reshape(-1).tolist())
    finally:
        ctx.set_mode(False)
