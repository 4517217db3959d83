"""The frames k_celt_recon_fb does not reconstruct, on the three routes of a CELT-only batch.

In a CELT-only step the frames recon_fast_eligible leaves out are CELT frames of at most one payload byte (celt_decode_frame's early
CELT_BAD_ARG, RF_BAD_CELT: a record without leaves; a record cannot overflow, tests/test_kernel_paths.py).  In order they go to
k_celt_recon in its role RECON_REST_ONLY, launched behind k_celt_recon_fb; in a pipelined CELT-only step k_celt_recon_fb finishes
them itself (`empties`, og_recon.hip) and nothing is launched behind it (launch_celt_recon, og_api.hip).  Either way such a frame
reports the reference's code, leaves the stream's CELT state alone -- the frames behind it decode as the oracle's do -- and moves the
stream's header words (final range, prev_mode).

165 stereo CELT fullband streams (the odd size of tests/test_gpu_parse_layout.py: a ragged last workgroup in every kernel that takes
64 or 128 frames) x 8 steps.  Every fifth stream, and the last one, carries in one step of three a packet whose CELT payload is 0 or
1 byte; in steps 0, 3 and 6 that holds for frame 0 and for frame 164, the first and the last workgroup of the step.  The batch runs
in order (pipeline off: the leftover launch serves those frames), as single pipelined steps and as ONE queued window; every step's
result codes, the PCM of every frame that decodes and the final range after the last step (of the streams whose last frame decodes)
are compared with the oracle, and the three runs with each other.  The bar is equality."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_pipeline import run_queued

STREAMS, FRAMES, TOC, L = 165, 8, 0xFC, 160
ROUTES = ("in_order", "single_steps", "window")


def short_len(f, s):
    """the payload bytes of (step, stream) when it is one of the short frames, else None"""
    if s % 5 and s != STREAMS - 1:
        return None
    phase = 0 if s == STREAMS - 1 else s // 5
    return (f + s) & 1 if (f + phase) % 3 == 0 else None


@functools.lru_cache(maxsize=None)
def batch():
    """packets [step][stream], and the oracle's PCM, return codes and final ranges (computed once, read-only)"""
    import oracle_py
    from conftest import load_pkg
    oracle, pkg = oracle_py.load(), load_pkg()
    pay = pkg.lcg_payloads(STREAMS, FRAMES, L, seed_base=0x1EF70000)
    pk = [[bytes([TOC]) + pay[f, s].tobytes() for s in range(STREAMS)] for f in range(FRAMES)]
    for f in range(FRAMES):
        for s in range(STREAMS):
            n = short_len(f, s)
            if n is not None:
                pk[f][s] = pk[f][s][:1 + n]
    ref = np.zeros((FRAMES, STREAMS, 960 * 2), dtype=np.int16)
    rets = np.zeros((FRAMES, STREAMS), dtype=np.int32)
    rngs = np.zeros(STREAMS, dtype=np.uint32)
    d = oracle.decoder(2)
    for s in range(STREAMS):
        d.init()
        for f in range(FRAMES):
            out, r = d.decode(pk[f][s])
            rets[f, s] = r
            if r > 0:
                ref[f, s] = out[:960].reshape(-1)
        rngs[s] = oracle.lib.oc_decoder_final_range(d.h)
    for a in (ref, rets, rngs):
        a.setflags(write=False)
    return pk, ref, rets, rngs


def test_the_batch_holds_the_frames_it_claims():
    """(no GPU work) short frames in at least four steps, of both lengths, in the first and in the last workgroup of one step; the
    oracle refuses exactly these"""
    pk, _, rets, _ = batch()
    short = {(f, s): short_len(f, s) for f in range(FRAMES) for s in range(STREAMS) if short_len(f, s) is not None}
    assert all(len(pk[f][s]) == 1 + n for (f, s), n in short.items()) and set(short.values()) == {0, 1}
    steps = sorted({f for f, _ in short})
    assert len(steps) >= 4, steps
    both_ends = [f for f in range(FRAMES) if (f, 0) in short and (f, STREAMS - 1) in short]
    assert len(both_ends) >= 2, both_ends
    assert all(f + 1 < FRAMES and (f + 1, 0) not in short for f in both_ends[:-1])  # (a fast frame follows a refused one)
    refused = rets < 0
    assert refused.sum() == len(short) and all(refused[f, s] for f, s in short)
    assert (rets[~refused] == 960).all()


def _final_ranges(ctx, n):
    head = (C.c_int32 * 4)()
    out = np.zeros(n, dtype=np.uint32)
    for s in range(n):
        assert ctx.lib.opusgpu_stream_state_get(ctx.h, s, head, 16) == 0
        out[s] = head[3] & 0xFFFFFFFF
    return out


@pytest.fixture(scope="module")
def runs(pkg, gpu_ctx):
    """the batch on the three routes: {route: (pcm, result codes, final ranges)}"""
    pk, _, _, _ = batch()
    lens = np.array([[len(p) for p in row] for row in pk], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens.reshape(-1))[:-1]]).reshape(FRAMES, STREAMS)
    arena = np.frombuffer(b"".join(p for row in pk for p in row) + bytes(16), dtype=np.uint8).copy()
    tocs = np.full((FRAMES, STREAMS), TOC, dtype=np.uint8)
    how = {"in_order": dict(pipeline=False), "single_steps": dict(pipeline=True, modes=pkg.toc_modes(TOC)),
           "window": dict(pipeline=True, window=True, modes=pkg.toc_modes(TOC))}
    out = {}
    for route in ROUTES:
        pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens - 1, tocs, **how[route])
        out[route] = (pcm, res, _final_ranges(gpu_ctx, STREAMS))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_every_step_matches_the_oracle(runs, route):
    _, ref, rets, rngs = batch()
    pcm, res, rng = runs[route]
    assert (res == rets).all(), (route, "return codes of (step, stream)", np.argwhere(res != rets)[:8].tolist())
    bad = (pcm != ref).any(axis=-1) & (rets == 960)
    assert not bad.any(), (route, "PCM of (step, stream)", np.argwhere(bad)[:8].tolist(), "frames that differ per step", bad.sum(axis=1).tolist())
    # (the final range of a stream whose LAST frame was refused is not compared with the oracle's: the library keeps the range
    # coder's word of the refused frame there, on every route, the oracle the one of the frame before; the routes must agree on it)
    last_ok = rets[-1] == 960
    assert last_ok.sum() >= STREAMS - len(range(0, STREAMS, 5)) - 1
    assert (rng[last_ok] == rngs[last_ok]).all(), (route, "final range after the last step, streams", np.flatnonzero((rng != rngs) & last_ok)[:8].tolist())


@pytest.mark.gpu
def test_the_three_routes_agree(runs):
    _, _, rets, _ = batch()
    ok = rets == 960
    pcm0, res0, rng0 = runs[ROUTES[0]]
    for route in ROUTES[1:]:
        pcm, res, rng = runs[route]
        assert (res == res0).all() and (rng == rng0).all(), route
        assert (pcm[ok] == pcm0[ok]).all(), route
