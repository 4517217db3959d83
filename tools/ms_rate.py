#!/usr/bin/env python3
"""Multistream step rate (include/opusgpu.h, MULTISTREAM): 5.1 (6 channels, 4 streams, 2 coupled) at N decoders, CELT-FB 20 ms
frames of 160 bytes on every elementary stream, device-resident.  Reports the ms step (wall time per step of K steps queued back
to back on the object's stream) and, for comparison, the same elementary frames decoded by two plain contexts (the stereo
step, then the mono step) with no mapping.
k_ms_map's own time comes from a kernel trace: run this script under `rocprofv3 --kernel-trace --stats -d DIR -o ms --` and
then `python3 tools/ms_rate.py --stats DIR` reads DIR's kernel_stats.csv and reports the kernel's time and effective bandwidth
(bytes read + bytes written per step: N * (2 * 960 * 2 * 2 + 2 * 960 * 2) + N * 960 * 6 * 2).
usage (GPU box): python3 tools/ms_rate.py [--n N] [--steps K] | python3 tools/ms_rate.py --stats DIR [--n N]"""
import argparse
import glob
import importlib.util
import json
import os
import time

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--stats", default=None)
args = ap.parse_args()
n = args.n
MAP_BYTES = n * (2 * 960 * 2 * 2 + 2 * 960 * 2) + n * 960 * 6 * 2

if args.stats:
    import csv
    rows = []
    for f in glob.glob(os.path.join(args.stats, "**", "*kernel_stats.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "k_ms_map" in r["Name"]]
    assert rows, "no k_ms_map in the kernel statistics"
    r = rows[0]
    avg_ms = float(r["AverageNs"]) / 1e6
    print(json.dumps({"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_ms": round(avg_ms, 4),
                      "min_ms": round(float(r["MinNs"]) / 1e6, 4), "bytes_per_step": MAP_BYTES,
                      "tb_per_s": round(MAP_BYTES / (avg_ms / 1e3) / 1e12, 2)}))
    raise SystemExit(0)

spec = importlib.util.spec_from_file_location("opusgpu_pkg", os.path.join(here, "..", "esp32-opus-player_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pkg)

S, CP, CH, L = 4, 2, 6, 160
rng = np.random.default_rng(1)
toc_st, toc_mo = 0xFC, 0xF8  # CELT FB 20 ms, stereo / mono
flags = {t: pkg.packet_to_frames(bytes([t, 0, 0]))[0][2] for t in (toc_st, toc_mo)}
arena = rng.integers(0, 256, n * S * L + 16, dtype=np.uint8)
rows = np.zeros(n * S, dtype=pkg.DESC_DTYPE)
rows["stream"] = np.repeat(np.arange(n), S)
rows["offset"] = np.arange(n * S) * L
rows["len"] = L
rows["flags"] = np.tile([flags[toc_st]] * CP + [flags[toc_mo]] * (S - CP), n)
# the same frames for the two plain contexts
st = rows.reshape(n, S)[:, :CP].reshape(-1).copy()
st["stream"] = np.arange(n * CP)
mo = rows.reshape(n, S)[:, CP:].reshape(-1).copy()
mo["stream"] = np.arange(n * (S - CP))

ctx = pkg.Context(0)
d_rows, d_arena = ctx.dev_alloc(rows.nbytes), ctx.dev_alloc(arena.nbytes)
d_pcm, d_res = ctx.dev_alloc(n * 960 * CH * 2), ctx.dev_alloc(4 * n)
ctx.h2d(d_rows, rows)
ctx.h2d(d_arena, arena)
ms = pkg.MultistreamContext(0, n, CH, S, CP, [0, 4, 1, 2, 3, 5])


def timed(step, sync, k):
    step()
    sync()
    t0 = time.perf_counter()
    for _ in range(k):
        step()
    sync()
    return (time.perf_counter() - t0) / k * 1e3


ms_ms = timed(lambda: ms.decode_step_device(n, d_rows, d_arena, d_pcm, d_res), ms.synchronize, args.steps)
res = np.zeros(n, np.int32)
ctx.d2h(res, d_res)
assert (res == 960).all(), np.unique(res)[:8]

cs, cm = pkg.Context(0), pkg.Context(0)
cs.streams_alloc(n * CP, 2)
cm.streams_alloc(n * (S - CP), 1)
d_st, d_mo = ctx.dev_alloc(st.nbytes), ctx.dev_alloc(mo.nbytes)
ctx.h2d(d_st, st)
ctx.h2d(d_mo, mo)
d_pst, d_pmo = ctx.dev_alloc(n * CP * 960 * 4), ctx.dev_alloc(n * (S - CP) * 960 * 2)
d_rst, d_rmo = ctx.dev_alloc(4 * n * CP), ctx.dev_alloc(4 * n * (S - CP))


def plain():
    cs.decode_step_device(n * CP, d_st, d_arena, d_pst, d_rst)
    cs.synchronize()
    cm.decode_step_device(n * (S - CP), d_mo, d_arena, d_pmo, d_rmo)


st_ms = timed(lambda: cs.decode_step_device(n * CP, d_st, d_arena, d_pst, d_rst), cs.synchronize, args.steps)
mo_ms = timed(lambda: cm.decode_step_device(n * (S - CP), d_mo, d_arena, d_pmo, d_rmo), cm.synchronize, args.steps)
seq_ms = timed(plain, cm.synchronize, args.steps)
print(json.dumps({"layout": "5.1", "decoders": n, "ms_step_ms": round(ms_ms, 3), "stereo_step_ms": round(st_ms, 3),
                  "mono_step_ms": round(mo_ms, 3), "stereo_then_mono_ms": round(seq_ms, 3), "map_bytes_per_step": MAP_BYTES}))
ms.close()
cs.close()
cm.close()
ctx.close()
