"""The spreading rotation of the PVQ leaves as it ships (rotate1_lane / rotate_chain, og_celt_recon.hpp: a chain at a time, four
steps at a time on packed pairs, the backward sweep started where the forward one counted to) in host emulation against
exp_rotation1 (celt.cpp:684) as its two plain sweeps -- driver tests/emul/og_rotation_chain_test.cpp, built here with g++ under
ASan + UBSan; no GPU:

* every block length 1 .. 176 x every stride 1 .. length: chains without a pair, with one pair, with exactly a multiple of four
  steps (what separates the unrolled loops from their tails) all occur, and the driver counts them;
* c, s and the coefficients: random i16 values and the corners -32768, -1, 0, 32767 (all sixteen corner pairs of (c, s));
* every vector has exactly `length` elements, so an access past the block's end is a sanitizer report.

The bar is equality, bit for bit."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")


def test_shipped_rotation_equals_the_two_plain_sweeps(tmp_path):
    exe = str(tmp_path / "og_rotation_chain_test")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(EMUL_DIR, "og_rotation_chain_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    m = re.search(r"cases (\d+) no_pair (\d+) one_pair (\d+) fours (\d+)", r.stdout)
    assert m, r.stdout
    cases, no_pair, one_pair, fours = map(int, m.groups())
    assert cases == 8 * 176 * 177 // 2  # eight draws for every (length, stride)
    assert no_pair > 0 and one_pair > 0 and fours > 0
