#!/usr/bin/env python3
"""usage: tools/comb_step_census.py [streams frames [payload-bytes]]   (default 64 x 12 x 160: 768 stereo frames of the bench's payloads)
The comb filter's steps in k_celt_recon_fb on the bench's payloads, by class (tests/emul/og_comb_census_main.cpp, built here into a
temporary directory: the kernel source in host emulation, the device's step rule replayed for every call), and static x trips: the
vector instructions a step of each class executes -- read from `hipcc -S` of og_recon.hip through tools/isa_blocks.py for the tree
before og_comb_step.hpp (PARENT) and with it (NEW), DESIGN.md 6n -- times the steps per frame.  CPU only."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg  # noqa: E402

CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
KINDS = ("fade_both", "fade_off_to_on", "fade_on_to_off", "past_fade")
WINS = ("buffer", "ring", "across")
# vector instructions of one step: what every step of the kind executes with its window(s) left out, one window by class, and what
# a cross-fade step with lanes behind the cross-fade adds
PARENT = {"base": {"fade_both": 57, "fade_off_to_on": 57, "fade_on_to_off": 57, "past_fade": 26},
          "window": {"buffer": 4, "ring": 1, "across": 31}, "behind": {"fade_both": 11, "fade_off_to_on": 11, "fade_on_to_off": 11},
          "call": 23}
NEW = {"base": {"fade_both": 44, "fade_off_to_on": 42, "fade_on_to_off": 34, "past_fade": 13},
       "window": {"buffer": 1, "ring": 1, "across": 26}, "behind": {"fade_both": 10, "fade_off_to_on": 10, "fade_on_to_off": 2},
       "call": 22}


def census(n=64, frames=12, L=160):
    pkg = load_pkg()
    pay = pkg.lcg_payloads(n, frames, L)
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin = os.path.join(tmp, "og_comb_census_main"), os.path.join(tmp, "in.bin")
        flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fwrapv", "-Wno-pedantic", "-Wno-attributes", *flags, "-I", CSRC,
                               "-I", os.path.join(ROOT, "tests", "emul"), os.path.join(ROOT, "tests", "emul", "og_comb_census_main.cpp"), "-o", exe])
        with open(fin, "wb") as f:
            f.write(np.array([n, frames, L, 2, 2], dtype=np.int32).tobytes())
            f.write(pay.tobytes())
        out = subprocess.run([exe, fin], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def per_frame(c, t):
    """vector instructions per frame of the comb filter's calls under table t, by kind of step"""
    out = {}
    for k in KINDS:
        v = sum(c["steps_%s_%s" % (k, w)] * (t["base"][k] + t["window"][w]) for w in WINS)
        if k == "fade_both":
            v += sum(c["old_windows_fade_both_%s" % w] * t["window"][w] for w in WINS)
        if k != "past_fade":
            v += c["steps_%s_with_lanes_behind_the_fade" % k] * t["behind"][k]
        out[k] = v / c["frames"]
    out["calls"] = c["calls_that_filter"] * t["call"] / c["frames"]
    return out


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    c = census(*args)
    fr = c["frames"]
    print("%-52s %10s %12s" % ("counter", "total", "per frame"))
    for k, v in c.items():
        print("%-52s %10d %12.3f" % (k, v, v / fr))
    for k in KINDS:
        s = sum(c["steps_%s_%s" % (k, w)] for w in WINS)
        if s:
            print("%-52s %23.1f" % ("live lanes per step, " + k, c["live_lanes_" + k] / s))
    a, b = per_frame(c, PARENT), per_frame(c, NEW)
    print("\n%-28s %10s %10s %10s" % ("vector instructions / frame", "parent", "new", "drop"))
    for k in list(KINDS) + ["calls"]:
        print("%-28s %10.1f %10.1f %10.1f" % (k, a[k], b[k], a[k] - b[k]))
    print("%-28s %10.1f %10.1f %10.1f" % ("comb filter, total", sum(a.values()), sum(b.values()), sum(a.values()) - sum(b.values())))
