"""k_celt_post (og_api.hip) against the oracle, sample by sample: the de-emphasis kernel's fast path keeps ONE LDS buffer -- a row's
int16 outputs go over the row's own consumed int32 inputs, and what a lane needs of other rows (ring, position, SILK length) comes from
their lanes' registers -- and everything that is not a full wave of aligned stereo rows takes the row-per-lane path (celt_post_lane).

  * 33 and 64 stereo CELT fullband frames per step: one full wave of 64 rows and a wave of two (fast path, and celt_post_lane for the
    ragged wave), and two full waves.  160-byte LCG payloads, which clamp in sig2word16 in most frames, 20-byte ones, and a stream
    that goes silent for two steps (peak 0, then a frame that starts from -28 dB): loud and quiet rows side by side in one wave.  In
    order and as one pipelined window.
  * the same 64 streams behind a hybrid frame and a SILK-only one: the SILK-only frame behind a hybrid one decodes a 2.5 ms CELT frame
    (Q4), so the ring head stands at 960 + 120 and no position is a multiple of 32 again -- every wave takes celt_post_lane.
  * 32 hybrid fullband streams, one full wave: mono and stereo packets in a stereo decoder (960 and 1,920 SILK samples to add, the
    kind changing from step to step and from stream to stream), LCG payloads and the directed frames of tests/golden/saturation_paths.json
    whose SILK half saturates (the packed add clamps).  In order and as one pipelined window.
Every sample of every step is compared.  The bar is equality."""
import functools
import json
import os

import numpy as np
import pytest

from test_gpu_pipeline import run_queued

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 4
CELT, SILK_WB, HYB_ST, HYB_MONO = 0xFC, 0x4C, 0x7C, 0x78


def _pkg():
    from conftest import load_pkg
    return load_pkg()


def _oracle_run(pk):
    """packets [step][stream] through one oracle decoder per stream -> PCM int16 [steps, n, 1920] (read-only)"""
    import oracle_py
    oracle = oracle_py.load()
    steps, n = len(pk), len(pk[0])
    ref = np.zeros((steps, n, 960 * 2), dtype=np.int16)
    d = oracle.decoder(2)
    for s in range(n):
        d.init()
        for f in range(steps):
            out, r = d.decode(pk[f][s])
            assert r == 960, (f, s, r)
            ref[f, s] = out[:960].reshape(-1)
    ref.setflags(write=False)
    return ref


def _celt_packets(n):
    pkg = _pkg()
    big, small = pkg.lcg_payloads(n, FRAMES, 160, seed_base=0x9057A000 + n), pkg.lcg_payloads(n, FRAMES, 20, seed_base=0x9057B000 + n)
    pk = [[bytes([CELT]) + (small if s % 4 == 3 else big)[f, s].tobytes() for s in range(n)] for f in range(FRAMES)]
    for f in (1, 2):  # the silence flag: four 0xFF bytes in front (tests/parse_alloc_batches.py)
        pk[f][n - 2] = bytes([CELT]) + b"\xff" * 4 + pk[f][n - 2][5:]
    return pk


@functools.lru_cache(maxsize=None)
def celt_batch(n):
    pk = _celt_packets(n)
    return pk, _oracle_run(pk)


@functools.lru_cache(maxsize=None)
def unaligned_batch():
    """64 streams: hybrid, SILK-only wideband (+ the 2.5 ms CELT frame of the transition), then the CELT steps of celt_batch(64)"""
    pkg = _pkg()
    n = 64
    hyb, silk = pkg.lcg_payloads(n, 1, 120, seed_base=0x9057C000), pkg.lcg_payloads(n, 1, 60, seed_base=0x9057D000)
    pk = [[bytes([HYB_ST]) + hyb[0, s].tobytes() for s in range(n)], [bytes([SILK_WB]) + silk[0, s].tobytes() for s in range(n)]]
    pk += _celt_packets(n)
    return pk, _oracle_run(pk)


@functools.lru_cache(maxsize=None)
def hybrid_batch():
    pkg = _pkg()
    n = 32
    pay = pkg.lcg_payloads(n, FRAMES, 120, seed_base=0x9057E000)
    # stream s sends mono packets in the steps where (f + s) % 3 == 0: 960 SILK samples to add, else 1,920
    pk = [[bytes([HYB_MONO if (f + s) % 3 == 0 else HYB_ST]) + pay[f, s].tobytes() for s in range(n)] for f in range(FRAMES)]
    corpus = json.load(open(os.path.join(ROOT, "tests", "golden", "saturation_paths.json")))["entries"]
    loud = [e for e in corpus if not e["rfc"] and e["channels"] == 2 and e["packets"][0][:2] == "7c" and len(e["packets"]) <= FRAMES]
    assert len(loud) >= 2
    for j, e in enumerate(loud):  # at both ends of the wave's rows and in the middle, among LCG neighbours
        for s in (j, 15 - j, 31 - j):
            for f, hx in enumerate(e["packets"]):
                pk[f][s] = bytes.fromhex(hx)
    return pk, _oracle_run(pk)


def test_the_batches_hold_loud_and_quiet_frames():
    """(no GPU work) clamped samples and near-silent frames in the CELT batches' full waves; both SILK lengths in every hybrid step; the
    directed hybrid frames reach full scale"""
    for n in (33, 64):
        _, ref = celt_batch(n)
        peak = np.abs(ref[:, :32].astype(np.int32)).max(axis=-1) if n == 33 else np.abs(ref.astype(np.int32)).max(axis=-1)
        assert (peak >= 32767).sum() >= 8 and (peak < 256).sum() >= 1 + (n == 64), (n, peak.tolist())
    _, ref = celt_batch(64)
    assert (np.abs(ref[:, 62].astype(np.int32)).max(axis=-1) < 256).sum() >= 2
    pk, ref = hybrid_batch()
    for f in range(FRAMES):
        kinds = {p[0] for p in pk[f]}
        assert kinds == {HYB_MONO, HYB_ST}, (f, kinds)
    assert (np.abs(ref[:, :2].astype(np.int32)).max(axis=-1) >= 32767).any()


def _run(pkg, ctx, pk, route):
    steps, n = len(pk), len(pk[0])
    lens = np.array([[len(p) for p in row] for row in pk], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens.reshape(-1))[:-1]]).reshape(steps, n)
    arena = np.frombuffer(b"".join(p for row in pk for p in row) + bytes(16), dtype=np.uint8).copy()
    tocs = np.array([[p[0] for p in row] for row in pk], dtype=np.uint8)
    modes = {pkg.toc_modes(int(t)) for t in tocs.reshape(-1)}
    if route == "in_order":
        how = dict(pipeline=False)
    else:
        assert len(modes) == 1  # (a window is declared with one mode mask)
        how = dict(pipeline=True, window=True, modes=modes.pop())
    return run_queued(pkg, ctx, 2, arena, offs, lens - 1, tocs, **how)


def _same(pcm, res, ref, what):
    assert (res == 960).all(), (what, "result codes of (step, stream)", np.argwhere(res != 960)[:8].tolist())
    bad = pcm != ref
    assert not bad.any(), (what, "first samples that differ (step, stream, index)", np.argwhere(bad)[:8].tolist(), "frames that differ per step",
                           bad.any(axis=-1).sum(axis=1).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
@pytest.mark.parametrize("n", [33, 64])
def test_celt_rows_loud_and_quiet(pkg, gpu_ctx, n, route):
    pk, ref = celt_batch(n)
    pcm, res = _run(pkg, gpu_ctx, pk, route)
    _same(pcm, res, ref, (n, route))


@pytest.mark.gpu
def test_rows_whose_ring_head_is_no_multiple_of_32(pkg, gpu_ctx):
    pk, ref = unaligned_batch()
    pcm, res = _run(pkg, gpu_ctx, pk, "in_order")
    _same(pcm, res, ref, "behind a 2.5 ms frame")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
def test_hybrid_rows_add_960_and_1920_silk_samples(pkg, gpu_ctx, route):
    pk, ref = hybrid_batch()
    pcm, res = _run(pkg, gpu_ctx, pk, route)
    _same(pcm, res, ref, ("hybrid", route))
