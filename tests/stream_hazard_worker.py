"""Child process of tests/test_gpu_stream_hazards.py: with the OPUSGPU_STALL_STREAM / OPUSGPU_STALL_US setting the parent put into
the environment (og_debug.hpp: one of the library's streams falls behind the others by whole steps), queue 8 steps of every
pipelined flow back to back -- no synchronisation in between, every step its own PCM and result buffers -- and compare every
sample and every return code with the oracle.  Prints one line per run ("ok" / "FAIL") with its time per step; exits 1 if a run
differs.  (GPU box.)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest
import oracle_py
from test_gpu_pipeline import CONFIGS, desc_flags, make_walk

pkg = conftest.load_pkg()
oracle = oracle_py.load()
FRAMES, N, N_HALVES = 8, 2048, 8192  # (N_HALVES: 2 x OG_HALVES_MIN, the smallest in-order step cut into two halves)
CH = 2


def constant_tables(rng, n, tocs, L):
    """Every frame of stream s carries TOC tocs[s] and L[s] payload bytes; -> arena, offs [frames, n] (TOC byte), plen, toc."""
    toc = np.broadcast_to(np.asarray(tocs, dtype=np.uint8), (FRAMES, n)).copy()
    plen = np.broadcast_to(np.asarray(L, dtype=np.int64) + 1, (FRAMES, n)).copy()
    offs = np.concatenate([[0], np.cumsum(plen.reshape(-1))[:-1]]).reshape(FRAMES, n)
    arena = rng.integers(0, 256, int(plen.sum()) + 16, dtype=np.uint8)
    arena[offs.reshape(-1)] = toc.reshape(-1)
    return arena, offs, plen, toc


def step_tables(arena, offs, plen, toc, by_header=False, group_by_mode=False):
    """One descriptor table per step.  by_header: in the order of the frames' LBRR flags (pkg.silk_header_key, as bench.py orders
    SILK-only / hybrid steps): slot j is then stream descs["stream"][j].  group_by_mode: SILK-only, hybrid, CELT-only frames in that
    order (decode_step_by_kind); -> list of (descs, (n_silk, n_hybrid, n_celt))."""
    frames, n = offs.shape
    flags, mode = desc_flags(toc)
    out = []
    for f in range(frames):
        d = np.zeros(n, dtype=pkg.DESC_DTYPE)
        d["stream"] = np.arange(n, dtype=np.int32)
        d["offset"] = (offs[f] + 1).astype(np.int32)
        d["len"] = (plen[f] - 1).astype(np.int32)
        d["flags"] = flags[f]
        if by_header:  # (any order of a step's table is a valid one: this is the bench's)
            d = d[np.argsort(pkg.silk_header_key(arena[offs[f] + 1], True), kind="stable")]
        if group_by_mode:
            d = d[np.argsort(mode[f], kind="stable")]
        out.append((d, tuple(int((mode[f] == m).sum()) for m in range(3))))
    return out


def run(ctx, n, arena, tables, modes, pipeline=True, window=False, by_kind=False):
    """Every step queued with nothing in between; -> per step (pcm [n, 960 * CH], res [n]) by slot, and ms per step."""
    ctx.streams_alloc(n, CH)
    ctx.set_pipeline(pipeline)
    d_arena = ctx.dev_alloc(arena.size)
    ctx.h2d(d_arena, arena)
    d_desc, d_pcm, d_res = [], [], []
    for d, _ in tables:
        d_desc.append(ctx.dev_alloc(d.nbytes))
        ctx.h2d(d_desc[-1], d)
        d_pcm.append(ctx.dev_alloc(n * 960 * CH * 2))
        d_res.append(ctx.dev_alloc(4 * n))
    ctx.synchronize()
    t0 = time.perf_counter()
    if window:
        ctx.decode_steps_device([n] * len(tables), d_desc, [d_arena] * len(tables), d_pcm, d_res, modes=modes)
    else:
        for f, (_, counts) in enumerate(tables):
            if by_kind:
                ctx.decode_step_by_kind(*counts, d_desc[f], d_arena, d_pcm[f], d_res[f], keeps_kind=True)
            else:
                ctx.decode_step_device(n, d_desc[f], d_arena, d_pcm[f], d_res[f], modes=modes)
    ctx.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / len(tables)
    got = []
    for f in range(len(tables)):
        pcm, res = np.zeros((n, 960 * CH), dtype=np.int16), np.zeros(n, dtype=np.int32)
        ctx.d2h(pcm, d_pcm[f])
        ctx.d2h(res, d_res[f])
        got.append((pcm, res))
    for p in [d_arena] + d_desc + d_pcm + d_res:
        ctx.dev_free(p)
    ctx.set_pipeline(False)
    return got, ms


def differ(got, tables, toc, ref, rets):
    """-> [(step, streams whose PCM differs, streams whose return code differs)] of the steps that differ."""
    _, mode = desc_flags(toc)
    bad = []
    for f, ((pcm, res), (d, _)) in enumerate(zip(got, tables)):
        s = d["stream"].astype(np.int64)
        want, wret = ref[s, f].reshape(len(s), -1), rets[s, f]
        ok = wret == 960
        half = ok & (mode[f, s] == 0) & ((toc[f, s] & 4) == 0)  # (Q3: a mono SILK packet in a stereo decoder defines 960 entries)
        full = ok & ~half
        pcm_bad = (pcm[full] != want[full]).any(axis=1).sum() + (pcm[half][:, :960] != want[half][:, :960]).any(axis=1).sum()
        res_bad = (res != wret).sum()
        if pcm_bad or res_bad:
            bad.append((f, int(pcm_bad), int(res_bad)))
    return bad


def main():
    rng = np.random.default_rng(0x57A11)
    ctx = pkg.Context(0)
    flows = []  # (name, n, (arena, offs, plen, toc), [(label, tables, modes, pipeline, window, by_kind)])
    # CELT-only steps declared with modes 4 (the early parse on parse_stream, the reconstruction on recon_stream)
    t = constant_tables(rng, N, [pkg.TOC_CELT_FB_STEREO] * N, [160] * N)
    st = step_tables(*t)
    flows.append(("celt-only (4)", N, t, [("one call per step", st, 4, True, False, False), ("window", st, 4, True, True, False)]))
    # declared SILK-only (1), hybrid-only (2) and SILK + hybrid (3) steps: the bench's TOCs; for 3, walks between SILK-only and
    # hybrid configurations (hybrid -> SILK-only transition frames, Q4, among them).  Half of the runs header-ordered.
    t = constant_tables(rng, N, [pkg.TOC_SILK_NB_STEREO] * N, [40] * N)
    flows.append(("silk-only (1)", N, t, [("one call per step, header-ordered", step_tables(*t, by_header=True), 1, True, False, False),
                                          ("window", step_tables(*t), 1, True, True, False)]))
    t = constant_tables(rng, N, [pkg.TOC_HYBRID_FB_STEREO] * N, [120] * N)
    flows.append(("hybrid-only (2)", N, t, [("one call per step", step_tables(*t), 2, True, False, False),
                                            ("window, header-ordered", step_tables(*t, by_header=True), 2, True, True, False)]))
    arena, offs, plen, lens, toc = make_walk(rng, N, FRAMES, CH, configs=np.array([1, 5, 9, 13, 15]), p_home=0.7)
    t = (arena, offs, plen, toc)
    flows.append(("silk + hybrid (3)", N, t, [("one call per step, header-ordered", step_tables(*t, by_header=True), 3, True, False, False),
                                              ("window", step_tables(*t), 3, True, True, False)]))
    # OPUSGPU_STEP_KEEPS_MODE: stream s is SILK-NB, hybrid FB or CELT FB by s % 3 -- whole steps (7 | 8) and three declared sub-steps
    t = constant_tables(rng, N, np.array([pkg.TOC_SILK_NB_STEREO, pkg.TOC_HYBRID_FB_STEREO, pkg.TOC_CELT_FB_STEREO])[np.arange(N) % 3],
                        np.array([40, 120, 160])[np.arange(N) % 3])
    flows.append(("keeps mode (7|8)", N, t, [("one call per step", step_tables(*t), 7 | pkg.STEP_KEEPS_MODE, True, False, False),
                                             ("sub-steps by kind", step_tables(*t, group_by_mode=True), 0, True, False, True)]))
    # undeclared steps of random mode walks (modes 0) with pipelining on
    arena, offs, plen, lens, toc = make_walk(rng, N, FRAMES, CH, configs=CONFIGS)
    t = (arena, offs, plen, toc)
    st = step_tables(*t)
    flows.append(("undeclared walks (0)", N, t, [("one call per step", st, 0, True, False, False), ("window", st, 0, True, True, False)]))
    # in-order steps cut into two halves: the second half on side_stream (a context that has never pipelined) or on recon_stream
    arena, offs, plen, lens, toc = make_walk(rng, N_HALVES, FRAMES, CH, configs=CONFIGS)
    t = (arena, offs, plen, toc)
    st = step_tables(*t)
    flows.append(("in-order halves (0)", N_HALVES, t, [("pipelining off", st, 0, False, False, False), ("pipelining on", st, 0, True, False, False)]))

    failed = 0
    for name, n, (arena, offs, plen, toc), runs in flows:
        ref, rets = oracle.batch_decode_var(CH, arena, offs, plen.astype(np.int32))
        for label, tables, modes, pipeline, window, by_kind in runs:
            c = ctx if pipeline else pkg.Context(0)  # (a context with a reconstruction stream runs second halves there)
            got, ms = run(c, n, arena, tables, modes, pipeline, window, by_kind)
            if c is not ctx:
                c.close()
            bad = differ(got, tables, toc, ref, rets)
            failed += bool(bad)
            what = "; ".join(f"step {f}: {p} of {n} streams' PCM differ, {r} return codes" for f, p, r in bad)
            print(f"{'FAIL' if bad else 'ok  '} {name}, {label}: {ms:.2f} ms per step{' -- ' + what if bad else ''}", flush=True)
    ctx.close()
    print(f"stall {os.environ.get('OPUSGPU_STALL_STREAM', '-')} {os.environ.get('OPUSGPU_STALL_US', '0')} us: {failed} runs differ")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
