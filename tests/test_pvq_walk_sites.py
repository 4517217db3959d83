"""The reconstruction kernel's PVQ index walk (pvq_leaf_lane, og_celt_recon.hpp: one bisection per pulse for all lanes, the
collapse mask gathered from the pulses as they are stored) in host emulation, in the LDS layout of k_celt_recon_fb, against the
oracle's step-by-step cwrsi (oracle/oc_celt_math.c) -- driver tests/emul/og_pvq_walk_kat.cpp, built here with g++; no GPU:

* every (N, K) the pulse cache of the 48 kHz mode can produce (every band at every LM, N >= 2; each has a 32-bit codebook: asserted,
  nothing is skipped) x index 0, the last index, the indices around every U(N, k') for k' = 1 .. K + 1 -- where the first decoded
  value changes its sign or size -- and around U(N - 1, k'), and 200 indices from a seeded generator, x every block count B in
  {1, 2, 4, 8} that divides N.  Compared: the pulse vector and its energy yy as the walk leaves them (before the scaling), the
  scaled coefficients, and the collapse mask.  Every bar is equality.
* the block-of-position arithmetic of the mask, (j * M) >> 16 == j / blen, for every j < 176, every blen <= 176 (so every N <= 176
  with every B <= 8) and both multipliers the GPU's reciprocal can yield.
* the bench's payloads (CELT-only fullband stereo, 160-byte LCG payloads) through the emulated kernels in k_celt_recon_fb's own
  layout: every PCM sample equals the oracle's."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
ORACLE_DIR = os.path.join(ROOT, "oracle")


@pytest.fixture(scope="module")
def kat(tmp_path_factory, oracle):  # (the oracle fixture builds liboc_oracle.so)
    out = str(tmp_path_factory.mktemp("kat") / "libog_pvq_walk_kat.so")
    flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-shared", "-fwrapv", "-Wno-pedantic", *flags, "-I", CSRC,
                           os.path.join(EMUL_DIR, "og_pvq_walk_kat.cpp"), "-L", ORACLE_DIR, "-loc_oracle", "-Wl,-rpath," + ORACLE_DIR,
                           "-o", out])
    lib = C.CDLL(out)
    lib.kat_walk.restype = C.c_long
    lib.kat_walk.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.kat_block_of.restype = C.c_long
    return lib


def _tables():
    spec = importlib.util.spec_from_file_location("gen_rom", os.path.join(ROOT, "tools", "gen_rom_tables.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _reachable_nk():
    """(N, K) of the pulse cache (compute_pulse_cache layout: index[(LM + 1) * nbEBands + band], LM = -1 .. 3), N >= 2."""
    t = _tables()
    nb = 21
    out = set()
    for lm in range(-1, 4):
        for band in range(nb):
            width = t.EBAND[band + 1] - t.EBAND[band]
            n = width << lm if lm >= 0 else width >> 1
            if n < 2 or (lm < 0 and width & 1):
                continue
            at = t.PULSE_IDX[(lm + 1) * nb + band]
            if at < 0:
                continue
            for q in range(1, t.PULSE_BITS[at] + 1):
                out.add((n, q if q < 8 else (8 + (q & 7)) << ((q >> 3) - 1)))
    return sorted(out)


def _u_table(nmax, kmax):
    """U(n, k) in exact integers, rows 0 .. nmax, columns 0 .. kmax (U(n, 0) = 0 for n > 0, as cwrsi takes it)."""
    u = [[0] * (kmax + 1) for _ in range(nmax + 1)]
    for n in range(1, nmax + 1):
        for k in range(1, kmax + 1):
            u[n][k] = 1 if (n == 1 or k == 1) else min(u[n - 1][k] + u[n][k - 1] + u[n - 1][k - 1], 1 << 80)
    return u


def test_walk_equals_cwrsi_over_every_reachable_codebook(kat):
    pairs = _reachable_nk()
    assert len(pairs) > 300 and max(n for n, _ in pairs) == 176 and min(n for n, _ in pairs) == 2
    u = _u_table(176, max(k for _, k in pairs) + 2)
    rng = np.random.default_rng(56)
    where = (C.c_uint * 2)()
    cases = C.c_long(0)
    dense = sparse = multi = 0
    for n, k in pairs:
        v = u[n][k] + u[n][k + 1]
        assert 0 < v <= 0xFFFFFFFF, (n, k, v)  # a legal (N, K) has a 32-bit codebook: the reference walk covers all that is run
        if v <= 4096:
            idxs = set(range(v))  # a small codebook: all of it
        else:
            draws = set()
            while len(draws) < 200:  # 200 different ones
                draws |= {int(x) for x in rng.integers(0, v, 200 - len(draws))}
            idxs = {0, 1, v - 1, v - 2} | draws
        for j in range(1, k + 2):
            for d in (-1, 0, 1):
                idxs.add(u[n][j] + d)
                idxs.add(u[n][k + 1] + u[n][j] + d)  # ... the same boundaries in the negative half
                idxs.add(u[n - 1][j] + d)
        arr = np.array(sorted(x for x in idxs if 0 <= x < v), dtype=np.uint32)
        assert len(arr) >= min(v, 200)
        bad = kat.kat_walk(n, k, arr.ctypes.data, len(arr), C.byref(where), C.byref(cases))
        assert bad == 0, (f"N {n} K {k}: {bad} cases differ, the first at index {where[0]} with B {where[1] >> 8}: "
                          f"{ {1: 'pulses', 2: 'yy', 3: 'collapse mask', 4: 'scaled coefficients'}[where[1] & 255]}")
        dense += n <= k
        sparse += n > k
        multi += n % 2 == 0
    print(f"{len(pairs)} codebooks ({sparse} with N > K, {dense} with N <= K, {multi} with more than one block count), {cases.value} leaves compared")
    assert dense > 50 and sparse > 50 and multi > 100 and cases.value > 150000


def test_block_of_position_is_exact(kat):
    cases = C.c_long(0)
    bad = kat.kat_block_of(C.byref(cases))
    assert bad == 0 and cases.value == 176 * 176 * 2


def test_bench_payloads_in_the_fast_kernels_layout_match_oracle(pkg, oracle):
    subprocess.check_call(["make", "-C", EMUL_DIR, "-s", "libog_emul_tight.so"])
    emu = C.CDLL(os.path.join(EMUL_DIR, "libog_emul_tight.so"))
    emu.emu_state_size.restype = C.c_int
    emu.emu_stream_init.argtypes = [C.c_void_p, C.c_int]
    emu.emu_decode_frame.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    toc, n, frames, L = pkg.TOC_CELT_FB_STEREO, 512, 6, 160
    pay = pkg.lcg_payloads(n, frames, L)
    ref, ok = oracle.batch_decode_threads(2, toc, pay)
    assert ok == n * frames
    st = C.create_string_buffer(emu.emu_state_size())
    out = np.zeros((960, 2), dtype=np.int16)
    for s in range(n):
        emu.emu_stream_init(st, 2)
        for f in range(frames):
            out[:] = 0
            r = emu.emu_decode_frame(st, pay[f, s].tobytes(), L, 1002, 1105, 2, out.ctypes.data)
            assert r == 960, (s, f, r)  # (no frame of these payloads is left to the general kernel)
            assert np.array_equal(out, ref[s, f]), f"stream {s}, frame {f}: emulated PCM differs from the oracle"
