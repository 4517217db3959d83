"""The comb filter's steps as the device runs them (og_comb_step.hpp: comb_call, comb_steps over a memory policy; the device's
policy and instruction forms are CombDev and mul16x32_q15_u there) on the host with 64 lanes, against comb_filter's host loop
(og_celt.hpp, OG_HOST_EMUL) -- driver tests/emul/og_comb_step_test.cpp, built here with g++ under ASan + UBSan and run as a
program; no GPU:

* both calls of celt_synthesis (off 0 / N 120, off 120 / N 840), every lag 15 .. 1022 as the old filter's against three lags of
  {15, 16, 17, 33, 65, 66, 67, 118, 120, 122, 300, 512, 700, 959, 1021, 1022, the lag itself} in rotation, and the same with the
  roles swapped; the nine pairs of tapsets; gains zero and non-zero on either side, equal and unequal; every ring head that is a
  multiple of 8; signals over the whole range of the clamp with one sample in eight at +-SIG_SAT, so that the clamp fires;
* every buffer word after the call equal to the host loop's;
* every read of every lane -- dead lanes included, which compute with what they read and store nothing -- inside the synthesis
  buffer, the ring and the window table; every store inside the frame's 960 samples, at most 64 per step;
* the scalar-operand product (operand sign-extended beforehand) equal to mul16x32_q15 for all 65,536 gains against the extremes of
  32 bits, of the clamp and of the tap sums and against sampled words.

The counts of cases and classes are asserted, so a loop that silently skips shows.  The bar is equality."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")


def test_device_steps_equal_the_host_loop(tmp_path):
    exe = str(tmp_path / "og_comb_step_test")
    flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wno-attributes", *flags, "-I", CSRC,
                           os.path.join(EMUL_DIR, "og_comb_step_test.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    c = dict(re.findall(r"(\w+) (\d+)", r.stdout))
    c = {k: int(v) for k, v in c.items()}
    lags = 1022 - 15 + 1
    assert c["fails"] == 0
    assert c["cases"] == lags * 3 * 2 * 2                      # every lag x three of the spread x two calls x roles swapped
    assert c["fade_cases"] + c["plain_cases"] == c["cases"] and c["plain_cases"] > 0
    assert c["off_to_on"] > 0 and c["on_to_off"] > 0           # cross-fades with one filter without a gain
    assert c["samples"] == c["cases"] // 2 * (120 + 840)
    assert c["clamped"] > 0                                    # the clamp fired
    assert min(c["buf_windows"], c["ring_windows"], c["mixed_windows"], c["mixed_fade_steps"], c["short_steps"]) > 0
    assert c["dead_lane_slots"] > 0
    assert c["products"] == 65536 * 96
