#!/usr/bin/env python3
"""Which code regions ("sites") of the PVQ index walk (og_celt_recon.hpp, pvq_leaf_lane) a WAVE passes per trip of its loop on the
headline payloads, and what candidate schedules of the walk would cost (CPU, host emulation for the leaves).  A wave
holds the leaves of one frame, one per lane, and runs every region that has at least one taker, loops to their deepest lane.
The walk is restated here per lane with the kernel's own schedule (tools/pvq_zero_run.py has the arithmetic); the cost of a region
is its static vector + LDS instruction count read off the ISA (tools/isa_by_line.py), so the sums are estimates of wave-instructions.
usage: python3 tools/pvq_walk_sites.py [streams [frames]]"""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pvq_zero_run as Z  # noqa: E402

U, V = Z.U, Z.V

# static vector + LDS instructions per region (parent ISA, profiles/r07/a_static_by_line.txt)
COST = dict(sparse_setup=25, zr_pre=10, zr_closed=18, zr_loop_setup=7, zr_probe=15, zr_apply=8, dense_setup=14, sign=4, cand7=36,
            ps_setup=3, ps_probe=17, pd_setup=3, pd_probe=13, store=13, loop=4,
            one_setup=9, one_probe=16, cand3=12)  # (the one-loop search as built, from the new ISA)


def bisect_up(lo, hi, ok):  # smallest t in [lo, hi] with ok(t) (ok(hi) assumed); returns (t, probes)
    p = 0
    while lo < hi:
        mid = (lo + hi) >> 1
        p += 1
        if ok(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo, p


def bisect_down(lo, hi, ok):  # largest t in [lo, hi] with ok(t) (ok(lo) assumed)
    p = 0
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        p += 1
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo, p


def lane_trips(n, k, i):
    """Per trip of the kernel's loop: {site: probes (1 for straight-line regions)}."""
    trips = []
    while n > 2 and k > 0:
        t = {}
        sparse = n > k
        if sparse:
            t["sparse_setup"] = 1
            if k <= 13 and n > k and n > 3:
                t["zr_pre"] = 1
                Vn = V(n, k)
                m = 2 * i - Vn
                m = m + 1 if m >= 0 else -m
                lo0 = max(k + 1, 2)
                if k <= 2:
                    t["zr_closed"] = 1
                    a = lo0
                    while a < n and V(a, k) < m:
                        a += 1
                else:
                    a, p = bisect_up(lo0, n, lambda x: V(x, k) >= m)
                    t["zr_bisect"] = p
                if a < n:
                    t["zr_apply"] = 1
                    i -= (Vn - V(a, k)) // 2
                    n = a
                    if n <= 2:
                        trips.append(t)
                        break
        else:
            t["dense_setup"] = 1
        t["sign"] = 1
        p1 = U(n, k + 1)
        s = i >= p1
        if s:
            i -= p1
        p0 = U(n, k)
        if p0 <= i and not s:
            i -= p0
        else:
            kk, p = bisect_down(0, k - 1, lambda r: U(n, r) <= i)
            # the one-loop search (what is built): n > k lanes bisect the table rows 4 .. k - 1 only, rows 1 .. 3 at once after it
            if sparse:
                lo, t["one_depth"] = bisect_down(min(3, k - 1), k - 1, lambda r: r <= 3 or U(n, r) <= i)
                if lo <= 3:
                    t["cand3"] = 1
            else:
                t["one_depth"] = p
            if sparse and k <= 8:
                t["cand7"] = 1
                t["pulse_depth"] = p
            elif sparse:
                t["ps_bisect"] = p
            else:
                t["pd_bisect"] = p
            t["store"] = 1
            i -= U(n, kk)
            k = kk
        n -= 1
        trips.append(t)
    return trips


def wave_cost(frames_trips):
    """Sum over trips of the wave's cost under the schedules compared; also how often each site has a taker."""
    tot = dict(old=0.0, merged_pulse=0.0, one_pulse_loop=0.0, all_loops=0.0, built=0.0)
    depth = dict(zr_bisect=0, ps_bisect=0, pd_bisect=0, one_depth=0)
    takers = {}
    ntrips = 0
    for lanes in frames_trips:
        for tr in range(max(len(x) for x in lanes)):
            ts = [x[tr] for x in lanes if tr < len(x)]
            ntrips += 1
            has = lambda s: any(s in t for t in ts)
            dep = lambda s: max((t.get(s, 0) for t in ts), default=0)
            for s in ("sparse_setup", "dense_setup", "zr_closed", "zr_bisect", "zr_apply", "cand7", "ps_bisect", "pd_bisect", "store"):
                if has(s):
                    takers[s] = takers.get(s, 0) + 1
            c = COST
            for s in depth:
                depth[s] += dep(s)
            base = c["loop"] + has("sparse_setup") * c["sparse_setup"] + has("zr_pre") * c["zr_pre"] + has("zr_apply") * c["zr_apply"] \
                + has("dense_setup") * c["dense_setup"] + has("sign") * c["sign"] + has("store") * c["store"]
            zr_old = has("zr_closed") * c["zr_closed"] + has("zr_bisect") * (c["zr_loop_setup"] + dep("zr_bisect") * c["zr_probe"])
            ps = has("ps_bisect") * (c["ps_setup"] + dep("ps_bisect") * c["ps_probe"])
            pd = has("pd_bisect") * (c["pd_setup"] + dep("pd_bisect") * c["pd_probe"])
            tot["old"] += base + zr_old + has("cand7") * c["cand7"] + ps + pd
            # the two pulse bisections as one loop (a probe that serves both kinds: the dearer one plus two selects), cand7 kept
            d2 = max(dep("ps_bisect"), dep("pd_bisect"))
            merged = (d2 > 0 or has("ps_bisect") or has("pd_bisect")) * (c["ps_setup"] + 2 + d2 * (c["ps_probe"] + 2))
            tot["merged_pulse"] += base + zr_old + has("cand7") * c["cand7"] + merged
            # ... and the k <= 8 lanes in that loop too (no seven-candidate form)
            d3 = max(d2, dep("pulse_depth"))
            any_pulse = has("cand7") or has("ps_bisect") or has("pd_bisect")
            one = any_pulse * (c["ps_setup"] + 2 + d3 * (c["ps_probe"] + 2))
            tot["one_pulse_loop"] += base + zr_old + one
            tot["built"] += base + zr_old + any_pulse * (c["one_setup"] + dep("one_depth") * c["one_probe"]) + has("cand3") * c["cand3"]
            # ... and the k <= 2 zero runs in the zero-run loop (depth as a bisection over lo0 .. n would take)
            dz = dep("zr_bisect")
            if has("zr_closed"):
                dz = max(dz, 8)  # (n up to 176: its bisection is up to eight probes, nearly always the wave's deepest)
            tot["all_loops"] += base + (dz > 0) * (c["zr_loop_setup"] + dz * (c["zr_probe"] + 3)) + one
    return tot, takers, ntrips, depth


def main():
    spec = importlib.util.spec_from_file_location("opusgpu_pkg", os.path.join(ROOT, "esp32-opus-player_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkg)
    lib = C.CDLL(os.path.join(ROOT, "tests", "emul", "libog_emul.so"))
    lib.emu_state_size.restype = C.c_int
    lib.emu_decode_frame.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
    lib.emu_last_leaf_geom.argtypes = [C.c_void_p, C.c_int]
    lib.emu_last_leaf_idx.argtypes = [C.c_void_p, C.c_int]
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    F = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    pay = pkg.lcg_payloads(S, F, 160)
    out = np.zeros((960, 2), dtype=np.int16)
    geom, idx = np.zeros(512, dtype=np.uint32), np.zeros(512, dtype=np.uint32)
    frames = []
    nB = 0
    for s in range(S):
        st = C.create_string_buffer(lib.emu_state_size())
        lib.emu_stream_init(st, 2)
        for f in range(F):
            assert lib.emu_decode_frame(st, pay[f, s].tobytes(), 160, 1002, 1105, 2, out.ctypes.data) == 960
            nl = lib.emu_last_leaf_geom(geom.ctypes.data, 512)
            lib.emu_last_leaf_idx(idx.ctypes.data, 512)
            for r0 in range(0, nl, 64):  # rounds of 64 leaves
                lanes = [lane_trips(int((g >> 11) & 255), int((g >> 19) & 255), int(ix)) for g, ix in zip(geom[r0:min(nl, r0 + 64)], idx[r0:min(nl, r0 + 64)])]
                frames.append([x for x in lanes if x] or [[]])
    tot, takers, ntrips, depth = wave_cost(frames)
    nf = S * F
    print(f"{nf} frames, {len(frames)} rounds: trips of the wave's loop per frame {ntrips / nf:.1f}")
    print("share of the wave's trips in which a region has at least one taker:")
    for s, v in sorted(takers.items(), key=lambda kv: -kv[1]):
        print(f"  {s:14s} {100.0 * v / ntrips:5.1f} %")
    print("probes per trip, the wave's deepest lane, mean over all trips:", {s: round(v / ntrips, 2) for s, v in depth.items()})
    print("estimated wave-instructions of the walk's loop per frame (static costs x takers x depth):")
    for s, v in tot.items():
        print(f"  {s:16s} {v / nf:7.0f}   ({100.0 * (v - tot['old']) / tot['old']:+.1f} %)")


if __name__ == "__main__":
    main()
