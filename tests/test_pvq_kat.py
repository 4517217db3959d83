"""Unit known-answer test ("cwrsi over all (N,K) reachable"): the kernels' PVQ leaf decode -- codeword index ->
pulses -> scaled to the leaf gain -> spreading rotation undone -> collapse mask -- in host emulation against the oracle's
alg_unquant, for every (N, K) the pulse cache of the 48 kHz mode can produce, over several indices (first, last, random),
block counts, spread settings and gains.  CPU only."""
import ctypes as C
import importlib.util
import os

import numpy as np

from pvq_cases import leaf_cases, sparse_leaf_cases  # (shared with tests/test_gpu_device_forms.py: the same cases on the GPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pvq_leaf_over_all_reachable_n_k(oracle):
    emu = C.CDLL(os.path.join(ROOT, "tests", "emul", "libog_emul.so"))
    emu.emu_pvq_leaf.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]
    emu.emu_pvq_leaf.restype = C.c_uint
    oracle.lib.oc_test_pvq_leaf.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]
    oracle.lib.oc_test_pvq_leaf.restype = C.c_uint
    a, b = np.zeros(176, dtype=np.int16), np.zeros(176, dtype=np.int16)
    checked = 0
    for n, k, index, B, gain, spread in leaf_cases():
        ma = emu.emu_pvq_leaf(n, k, index, B, gain, spread, a.ctypes.data)
        mb = oracle.lib.oc_test_pvq_leaf(n, k, index, spread, B, gain, b.ctypes.data)
        assert ma == mb, ("mask", n, k, index, B, spread, gain, ma, mb)
        assert (a[:n] == b[:n]).all(), ("X", n, k, index, B, spread, gain)
        checked += 1
    assert checked > 20000


def test_pvq_sparse_leaves_many_indices(oracle):
    """The leaf walk skips runs of zeros in sparse leaves by bisection (og_celt_recon.hpp, pvq_leaf_lane): every reachable
    (N, K) with more than one dimension per pulse, many indices each -- random ones, the first and last, and the ones around
    every U(N, j) boundary, where a run ends or a sign flips."""
    emu = C.CDLL(os.path.join(ROOT, "tests", "emul", "libog_emul.so"))
    emu.emu_pvq_leaf.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]
    emu.emu_pvq_leaf.restype = C.c_uint
    oracle.lib.oc_test_pvq_leaf.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]
    oracle.lib.oc_test_pvq_leaf.restype = C.c_uint
    a, b = np.zeros(176, dtype=np.int16), np.zeros(176, dtype=np.int16)
    checked = 0
    for n, k, index, B, gain, spread in sparse_leaf_cases():
        ma = emu.emu_pvq_leaf(n, k, index, B, gain, spread, a.ctypes.data)
        mb = oracle.lib.oc_test_pvq_leaf(n, k, index, spread, B, gain, b.ctypes.data)
        assert ma == mb and np.array_equal(a[:n], b[:n]), (n, k, index)
        checked += 1
    assert checked > 10000


def test_zero_run_identity_in_exact_integers():
    """What the kernel's zero-run skip rests on (tools/pvq_zero_run.py): with V(a) = U(a, k) + U(a, k + 1) the dimensions n .. a+1
    of a codeword all decode to zero exactly when V(n) - V(a) <= 2 i < V(n) + V(a), and skipping them subtracts (V(n) - V(a)) / 2
    -- checked against the step-by-step walk (cwrsi, src/celt.cpp:2545) in Python's exact integers."""
    import random
    spec = importlib.util.spec_from_file_location("pvq_zero_run", os.path.join(ROOT, "tools", "pvq_zero_run.py"))
    z = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(z)
    random.seed(5)
    n_cases = 0
    for n in (3, 4, 6, 8, 11, 16, 22, 24, 36, 48, 72, 96, 144, 176):
        for k in (1, 2, 3, 4, 5, 7, 10, 13, 14, 20, 40):
            v = z.V(n, k)
            if v >= 2 ** 32:
                continue
            picks = [0, v - 1, z.U(n, k), z.U(n, k) - 1, z.U(n, k + 1), z.U(n, k + 1) - 1] + [random.randrange(v) for _ in range(12)]
            for i in picks:
                if not 0 <= i < v:
                    continue
                ref = z.cwrsi_ref(n, k, i)
                assert sum(abs(x) for x in ref) == k and len(ref) == n
                for ratio in (1, 2):
                    assert z.cwrsi_skip2(n, k, i, ratio) == ref, (n, k, i, ratio)
                n_cases += 1
    assert n_cases > 1500
