"""The CELT parse kernel's rewritten decode helpers against the code they replace, in host emulation, over their WHOLE input sets
(tests/emul/og_parse_kat.cpp, built here with g++; no GPU):

* isqrt24 (a float root and two corrections) against isqrt32 (celt.cpp:3086) for every argument below 2^24 -- the triangular
  angle model passes at most 8 * 129^2 + 1.
* the lane flavour of ec_dec_uint (one decode / update for both sizes of the total) against the template it overloads: every
  total from 2 to 65,537 (past the point where the raw bits start, 257, and every count of raw bits up to eight) and every
  PVQ codebook size of the pulse cache (rom_pulse_v: the totals the leaves really pass, up to 2^32 - 1), each from 24 decoder
  states.  Compared: the value and every field of the coder state afterwards (the error flag among them).
  Each total is also decoded from two constructed states that yield its top range-coded value, one followed by raw bits that
  are all ones: the error return (raw bits that carry the value past the total) and its clamp must be reached -- asserted.
* split_theta_lane against compute_theta as the partition walk used to call it, two ways.  (a) Every band x every LM a split
  can leave (-1 .. 2) x every budget b the band loop can hand down (0 .. 16383, its clamp) x both angle models, the decoder state
  changing from call to call: this walks everything in front of the decode (the resolution qn, the budget arithmetic) but only
  SAMPLES the decoded value.  (b) For every resolution qn that compute_qn returns anywhere in that domain (the even values the
  exp2 table yields, 2 .. 256: the test prints and checks the set) x both models x EVERY value fm in 0 .. ft - 1 the decoder can
  return against the model's total, from 3 decoder states each whose `val` is placed inside fm's interval: this walks the mapping
  fm -> (itheta, fl, fs) -- the low / high select, isqrt24, the fl / fs algebra, the raw bit and its error clamp at qn = 256 --
  completely.  Compared in both: all six fields of the split, the budget left and the coder state.  (compute_theta's uniform
  branch calls ec_dec_uint, i.e. the new overload; (b) also runs the template's body from the same states.)

Every bar is equality: the integer path is bit-exact by construction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")


@pytest.fixture(scope="module")
def kat(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("kat") / "libog_parse_kat.so")
    flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-shared", "-fwrapv", *flags, "-I", CSRC,
                           os.path.join(EMUL_DIR, "og_parse_kat.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.kat_isqrt.restype = C.c_long
    lib.kat_uint.restype = C.c_long
    lib.kat_theta.restype = C.c_long
    lib.kat_theta_values.restype = C.c_long
    return lib


def _packet(seed, n=160):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def test_isqrt24_is_isqrt32_below_2_24(kat):
    where = C.c_uint(0)
    bad = kat.kat_isqrt(C.byref(where))
    assert bad == 0, f"{bad} arguments differ, the first {where.value}"


@pytest.mark.parametrize("seed", [1, 2])
def test_lane_uint_is_the_template(kat, seed):
    sizes = (C.c_uint * 1024)()
    n = kat.kat_pulse_v(sizes, 1024)
    assert 0 < n <= 1024
    pkt = _packet(seed)
    where = C.c_uint(0)
    errors = C.c_long(0)
    bad = kat.kat_uint(pkt.ctypes.data_as(C.c_void_p), len(pkt), 2, 65537, sizes, n, 24, C.byref(where), C.byref(errors))
    print(f"error returns among the compared calls: {errors.value}")
    assert bad == 0, f"{bad} (total, state) pairs differ, the first at total {where.value}"
    assert errors.value > 0, "no state took ec_dec_uint's error return: that path is not covered"


@pytest.mark.parametrize("seed", [3, 4])
def test_split_theta_lane_is_compute_theta(kat, seed):
    pkt = _packet(seed)
    where = (C.c_uint * 2)()
    bad = kat.kat_theta(pkt.ctypes.data_as(C.c_void_p), len(pkt), 16383, 16, where)
    assert bad == 0, (f"{bad} calls differ, the first at band {where[0] & 255}, LM {((where[0] >> 8) & 15) - 1}, "
                      f"B0 {where[0] >> 12}, b {where[1]}")


@pytest.mark.parametrize("seed", [5, 6])
def test_split_theta_lane_maps_every_decoded_value_like_compute_theta(kat, seed):
    pkt = _packet(seed)
    where = (C.c_uint * 2)()
    cases, n_qn = C.c_long(0), C.c_int(0)
    qns = (C.c_int * 260)()
    bad = kat.kat_theta_values(pkt.ctypes.data_as(C.c_void_p), len(pkt), 3, where, C.byref(cases), qns, C.byref(n_qn))
    found = [qns[i] for i in range(n_qn.value)]
    print(f"{cases.value} calls compared over qn = {found}")
    assert bad >= 0, "the test could not construct its decoder states" if bad == -2 else "compute_qn left 0 .. 259"
    # compute_qn (celt.cpp:1215) rounds exp2_table8[qb & 7] >> (14 - (qb >> 3)) up to even for qb = 4 .. 64 (below 4 it returns 1: no
    # decode): the search over the walk's domain must have found every one of those, 256 -- the one with a raw bit -- among them
    exp2_table8 = [16384, 17866, 19483, 21247, 23170, 25267, 27554, 30048]
    formula = sorted({((exp2_table8[qb & 7] >> (14 - (qb >> 3))) + 1) >> 1 << 1 for qb in range(4, 65)})
    assert formula[0] == 2 and formula[-1] == 256
    assert found == formula, (found, formula)
    # every fm of every total, both models, three states: sum over qn of 3 x ((qn / 2 + 1)^2 + the uniform total)
    want = sum(3 * ((q // 2 + 1) ** 2 + (q >> (1 if q >= 256 else 0)) + 1) for q in found)
    assert cases.value == want, (cases.value, want)
    assert bad == 0, f"{bad} calls differ, the first at qn {where[0] & 4095}, B0 {where[0] >> 12}, fm {where[1]}"
