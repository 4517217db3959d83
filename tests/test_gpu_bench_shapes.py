"""Every stream of every step of the single-mode workloads bench.py times, against the oracle.

bench.py checks the last step of a timed window on ~320 streams -- the one step no later kernel can overwrite.  Here each workload
of bench.WORKLOADS with a single TOC (CELT-FB 65,536, SILK-NB 65,536, hybrid-FB 262,144 streams) is queued the way run_workload
queues it: the same TOC and payload length, SILK-only / hybrid step tables in the order of the frames' LBRR flags
(build_step(order_by_header=True): slot j is stream descs["stream"][j]), the mode mask toc_modes(toc), pipelining on, all steps in
ONE window.  Every step has its own PCM buffer and every (stream, step) block of it is compared with the oracle; then once more
with one output buffer shared by all steps, as the bench does, and its final step checked in full.

Host memory stays bounded: the oracle runs over chunks of streams and keeps a 64-bit fingerprint of each 20 ms stereo block (the
block's 480 64-bit words times odd random constants, summed mod 2^64: a change of any one sample changes it), and each step's
device buffer comes back in chunks of slots by pointer offset.  (Mixed pages at 262,144 streams are checked every step by
test_gpu_pages.py.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 8  # W + K of a short bench run
CHUNK = 16384  # streams per oracle call / slots per copy
BLOCK = 960 * 2  # int16 samples of one stereo frame
_K = np.random.default_rng(0xB10C).integers(0, 2**63, BLOCK // 4, dtype=np.uint64) | np.uint64(1)


def fingerprint(blocks):
    """int16 [m, 1920] -> uint64 [m]."""
    return np.ascontiguousarray(blocks).view(np.uint64) @ _K


def oracle_fingerprints(oracle, toc, pay):
    """pay uint8 [steps, n, L] -> fingerprints uint64 [n, steps] of the oracle's PCM."""
    steps, n, _ = pay.shape
    out = np.zeros((n, steps), dtype=np.uint64)
    for s0 in range(0, n, CHUNK):
        s1 = min(n, s0 + CHUNK)
        pcm, ok = oracle.batch_decode_threads(2, toc, np.ascontiguousarray(pay[:, s0:s1]))
        assert ok == (s1 - s0) * steps
        out[s0:s1] = fingerprint(pcm.reshape(-1, BLOCK)).reshape(s1 - s0, steps)
    return out


def differing_slots(ctx, d_pcm, d_res, stream_of, want):
    """Slots of one step's device PCM / results whose block differs from want[stream] or whose return code is not 960."""
    n = len(stream_of)
    res = np.zeros(n, dtype=np.int32)
    ctx.d2h(res, d_res)
    bad = res != 960
    buf = np.zeros((CHUNK, BLOCK), dtype=np.int16)
    base = d_pcm.value
    for j0 in range(0, n, CHUNK):
        j1 = min(n, j0 + CHUNK)
        ctx.d2h(buf[:j1 - j0], C.c_void_p(base + j0 * BLOCK * 2))
        bad[j0:j1] |= fingerprint(buf[:j1 - j0]) != want[stream_of[j0:j1]]
    return np.nonzero(bad)[0]


@pytest.mark.parametrize("name", ["celt_fb_stereo_64k", "silk_nb_stereo_64k", "hybrid_fb_stereo_256k"])
def test_every_step_of_a_bench_window(pkg, oracle, gpu_ctx, name):
    import bench
    toc, L, _, n = bench.WORKLOADS[name]
    modes = pkg.toc_modes(toc)
    by_header = not (toc & 0x80)
    pay = pkg.lcg_payloads(n, STEPS, L, seed_base=0xBE4C0000 + toc)
    want = oracle_fingerprints(oracle, toc, pay)
    ctx = gpu_ctx
    tabs, streams, frees = [], [], []
    for f in range(STEPS):
        arena, descs = pkg.build_step(toc, pay[f], order_by_header=by_header)
        a, d = ctx.dev_alloc(arena.nbytes + 16), ctx.dev_alloc(descs.nbytes)
        ctx.h2d(a, arena)
        ctx.h2d(d, descs)
        tabs.append((d, a))
        streams.append(descs["stream"].astype(np.int64))
        frees += [a, d]
    del pay
    try:
        for shared in (False, True):
            ctx.streams_alloc(n, 2)
            ctx.set_pipeline(True)
            outs = [(ctx.dev_alloc(n * BLOCK * 2), ctx.dev_alloc(4 * n)) for _ in range(1 if shared else STEPS)]
            if shared:
                outs = outs * STEPS
            ctx.decode_steps_device([n] * STEPS, [t[0] for t in tabs], [t[1] for t in tabs], [o[0] for o in outs], [o[1] for o in outs],
                                    modes=modes)
            ctx.synchronize()
            ctx.set_pipeline(False)
            for f in range(STEPS - 1 if shared else 0, STEPS):
                bad = differing_slots(ctx, outs[f][0], outs[f][1], streams[f], want[:, f])
                assert len(bad) == 0, (f"{name}, {'one shared output buffer' if shared else 'a buffer per step'}: step {f}: {len(bad)} of "
                                       f"{n} streams differ from the oracle (streams {streams[f][bad][:8].tolist()})")
            for p in {o[0].value: o[0] for o in outs}.values():
                ctx.dev_free(p)
            for p in {o[1].value: o[1] for o in outs}.values():
                ctx.dev_free(p)
    finally:
        ctx.set_pipeline(False)
        for p in frees:
            ctx.dev_free(p)
