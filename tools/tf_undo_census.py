#!/usr/bin/env python3
"""usage: tools/tf_undo_census.py [streams frames [payload-bytes]]   (default 64 x 12 x 160: 768 stereo frames of the bench's payloads)
How much work the phase-major band loop's parallel passes (pm_tf_undo), the stereo merge and the ring writes of k_celt_recon_fb
have on the bench's payloads, per frame and per class of job: the kernel source in host emulation with its event counters on
(tests/emul/og_tf_census_main.cpp, built here into a temporary directory).  CPU only.  DESIGN.md 6l puts the static instruction
counts of tools/isa_by_line.py beside these."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg  # noqa: E402

CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")


def census(n=64, frames=12, L=160):
    pkg = load_pkg()
    pay = pkg.lcg_payloads(n, frames, L)
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin = os.path.join(tmp, "og_tf_census_main"), os.path.join(tmp, "in.bin")
        flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fwrapv", "-Wno-pedantic", "-Wno-attributes", *flags, "-I", CSRC,
                               "-I", os.path.join(ROOT, "tests", "emul"), os.path.join(ROOT, "tests", "emul", "og_tf_census_main.cpp"), "-o", exe])
        with open(fin, "wb") as f:
            f.write(np.array([n, frames, L, 2, 2], dtype=np.int32).tobytes())
            f.write(pay.tobytes())
        out = subprocess.run([exe, fin], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:]]
    c = census(*args)
    fr = c["frames"]
    print("%-44s %10s %12s" % ("counter", "total", "per frame"))
    for k, v in c.items():
        print("%-44s %10d %12.3f" % (k, v, v / fr))
