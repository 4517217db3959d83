"""The GPU's CELT synthesis against the float64 model of tests/celt_model.py, on three routes (tests/test_celt_model.py holds the
oracle to the same model on the CPU; plans, tolerances and what is left out are that file's, unchanged):

  * RFC mode through k_decode_rfc (set_mode(True), decode_packets): the three CELT-only plans, mono and stereo decoders, frames of
    2.5 / 5 / 10 / 20 ms, every ordered pair of durations, packets of several frames.  The hybrid plan is checked for PCM equality
    with the oracle only; its CELT layer is held to the model on the CPU.
  * reference mode through the split path (k_celt_parse64 / k_celt_recon_fb / k_celt_post): 20 ms CELT-only, step by step with
    opusgpu_debug_stage_taps' syn_post against the model at TOL_SYN, and as pipelined steps (set_pipeline(1)).
  * reference mode through the single kernel k_decode_step: by default that kernel decodes only the parked Q4 frames, so the switch
    plan (hybrid -> SILK-only -> hybrid -> SILK-only -> CELT-only -> hybrid) and the 20 ms CELT-only plan run in a child process with
    OPUSGPU_SPLIT=0 (tests/celt_model_worker.py), where every frame goes through it: PCM equality with the oracle everywhere, the
    model where the frame is CELT-only.

The switch plan also runs on the default routes (hybrid halves on k_silk_* / k_celt_*, CELT-only frames on the split path, Q4's frame
on k_decode_step's second pass): an equality check with the oracle, whose CELT-only frames are the split path's once more.

The oracle decodes the same packets on the host and supplies the model's inputs (X, E, the header) through its tap log.  The GPU's PCM
must EQUAL the oracle's; against the model it is held to TOL_PCM like the oracle itself.
"""
import numpy as np
import pytest

import celt_model_plans as P
from celt_model_worker import groups as _groups, through_decode_packets as _through_decode_packets
from test_celt_model import run, tol_pcm, tol_syn, worst

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["rfc_runs", "rfc_pairs", "rfc_codes"])
def test_rfc_mode_against_the_model(oracle, gpu_ctx, name):
    plan, dec, mod, _, _ = run(oracle, name)
    got = _through_decode_packets(gpu_ctx, plan, dec, True)
    res = P.compare(plan, dec, mod, pcm_of=got)
    w = worst(res["pcm"], tol_pcm)
    print(name, "k_decode_rfc PCM: worst error / TOL_PCM", w, "over", len(res["pcm"]), "frames")
    assert len(res["pcm"]) == len(res["syn"]) >= 90 and w <= 1.0, (name, w)


def test_rfc_hybrid_equals_the_oracle(oracle, gpu_ctx):
    plan, dec, _, _, _ = run(oracle, "rfc_hybrid")
    _through_decode_packets(gpu_ctx, plan, dec, True)


def test_reference_switches_on_the_default_routes_equal_the_oracle(oracle, gpu_ctx):
    """what a caller gets: every packet's PCM equal to the oracle's (asserted in _through_decode_packets).  The CELT-only frames run on
    the split path here, behind the reference's partial reset; they are held to the model as well, k_decode_step's are in the test below"""
    plan, dec, mod, _, _ = run(oracle, "ref_switch")
    got = _through_decode_packets(gpu_ctx, plan, dec, False)
    res = P.compare(plan, dec, mod, pcm_of=got)
    w = worst(res["pcm"], tol_pcm)
    print("ref_switch, default routes, CELT-only PCM: worst error / TOL_PCM", w, "over", len(res["pcm"]), "frames")
    assert len(res["pcm"]) >= 16 and w <= 1.0, w


def test_reference_mode_through_the_single_kernel():
    """k_decode_step for every frame (OPUSGPU_SPLIT=0, read once per process: a child): ref_switch and ref_celt, tests/celt_model_worker.py"""
    import os
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "celt_model_worker.py")
    out = subprocess.run([sys.executable, worker], env=dict(os.environ, OPUSGPU_SPLIT="0"), capture_output=True, text=True, timeout=120)
    print(out.stdout[-600:])
    assert out.returncode == 0 and "celt model worker ok" in out.stdout, (out.stdout[-600:], out.stderr[-1200:])


# ---- the split path, step by step on device-resident tables ---------------------------------------------------------------------------
def _step_tables(pkg, plan, ids, f):
    """arena and descriptors of step f for the streams `ids` (code-0 CELT-only fullband packets; a descriptor points behind the TOC)"""
    pk = [plan["streams"][i]["packets"][f] for i in ids]
    descs = np.zeros(len(ids), dtype=pkg.DESC_DTYPE)
    at, parts = 0, []
    for k, p in enumerate(pk):
        assert p[0] & 0xFB == 0xF8
        descs[k] = (k, at + 1, len(p) - 1, 2 | (4 << 2) | (32 if p[0] & 4 else 0))
        parts.append(np.frombuffer(p, dtype=np.uint8))
        at += len(p)
    return np.concatenate(parts + [np.zeros(16, dtype=np.uint8)]), descs


@pytest.mark.parametrize("pipeline", [False, True])
def test_reference_celt_through_the_split_path(pkg, oracle, gpu_ctx, pipeline):
    ctx = gpu_ctx
    plan, dec, mod, _, _ = run(oracle, "ref_celt")
    got = [[None] * len(st["packets"]) for st in plan["streams"]]
    syn_err = []
    for channels, ids in sorted(_groups(plan).items()):
        n, steps = len(ids), len(plan["streams"][ids[0]]["packets"])
        tables = [_step_tables(pkg, plan, ids, f) for f in range(steps)]
        ctx.streams_alloc(n, channels)
        d_arena = [ctx.dev_alloc(a.size) for a, _ in tables]
        d_desc = [ctx.dev_alloc(16 * n) for _ in tables]
        d_pcm = [ctx.dev_alloc(n * 960 * channels * 2) for _ in tables]
        d_res = [ctx.dev_alloc(4 * n) for _ in tables]
        try:
            for f, (arena, descs) in enumerate(tables):   # (complete in device memory before any step is queued)
                ctx.h2d(d_arena[f], arena)
                ctx.h2d(d_desc[f], descs)
            ctx.set_pipeline(pipeline)
            for f in range(steps):
                ctx.decode_step_device(n, d_desc[f], d_arena[f], d_pcm[f], d_res[f], modes=pkg.HAS_CELT)
                if pipeline:
                    continue
                ctx.synchronize()
                for k, i in enumerate(ids):   # the reconstruction's output, before de-emphasis, against the model and the oracle's tap
                    rec, mr = dec[i][f]["frames"][0], mod[i][f][0]
                    t = ctx.debug_stage_taps(k)
                    post = np.array([np.array(t.syn_post[c]) for c in range(channels)])
                    assert (post == rec["syn_post"]).all(), ("syn_post differs from the oracle's tap", i, f)
                    if not (mr["dead"] or P.frame_clamps(rec)):
                        syn_err.append((np.abs(post / 4096.0 - mr["syn"]).max(), mr["peak"]))
            ctx.synchronize()
            for f in range(steps):
                pcm = np.zeros((n, 960, channels), dtype=np.int16)
                res = np.zeros(n, dtype=np.int32)
                ctx.d2h(pcm, d_pcm[f])
                ctx.d2h(res, d_res[f])
                for k, i in enumerate(ids):
                    assert res[k] == 960 == dec[i][f]["ret"], (i, f, int(res[k]))
                    assert (pcm[k] == dec[i][f]["pcm"]).all(), ("PCM differs from the oracle", i, f, pipeline)
                    got[i][f] = pcm[k].copy()
        finally:
            ctx.synchronize()
            ctx.set_pipeline(False)
            for p in d_arena + d_desc + d_pcm + d_res:
                ctx.dev_free(p)
    res = P.compare(plan, dec, mod, pcm_of=got)
    w = worst(res["pcm"], tol_pcm)
    print("split path, pipeline", pipeline, "PCM: worst error / TOL_PCM", w, "over", len(res["pcm"]), "frames")
    assert len(res["pcm"]) >= 90 and w <= 1.0, w
    if not pipeline:
        ws = worst(syn_err, tol_syn)
        print("split path syn_post: worst error / TOL_SYN", ws, "over", len(syn_err), "frames")
        assert len(syn_err) == len(res["syn"]) and ws <= 1.0, ws
