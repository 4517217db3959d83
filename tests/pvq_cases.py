"""The PVQ leaf cases of the known-answer tests, as generators: tests/test_pvq_kat.py runs them through the host emulation,
tests/test_gpu_device_forms.py through the kernels' own code on the GPU.  Both see the same cases in the same order (fixed
seeds); the reference of either is the oracle's oc_test_pvq_leaf."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables():
    spec = importlib.util.spec_from_file_location("gen_rom", os.path.join(ROOT, "tools", "gen_rom_tables.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _get_pulses(q):
    return q if q < 8 else (8 + (q & 7)) << ((q >> 3) - 1)


def reachable_nk():
    """(N, K) pairs of the pulse cache (compute_pulse_cache layout: index[(LM + 1) * nbEBands + band], LM = -1 .. 3)."""
    t = _tables()
    nb = 21
    out = set()
    for lm in range(-1, 4):
        for i in range(nb):
            width = t.EBAND[i + 1] - t.EBAND[i]
            n = width << lm if lm >= 0 else width >> 1
            if n < 1 or (lm < 0 and width & 1):
                continue
            idx = t.PULSE_IDX[(lm + 1) * nb + i]
            if idx < 0:
                continue
            for q in range(1, t.PULSE_BITS[idx] + 1):
                out.add((n, _get_pulses(q)))
    return sorted(out)


def _v(n, k, memo={}):  # V(n, k) = number of PVQ codewords = U(n, k) + U(n, k + 1)
    def u(a, b):
        if (a, b) in memo:
            return memo[(a, b)]
        if a == 0 or b == 0:
            r = 1 if (a == 0 and b == 0) else 0
        else:
            r = u(a - 1, b) + u(a, b - 1) + u(a - 1, b - 1)
        memo[(a, b)] = r
        return r
    sys.setrecursionlimit(10000)
    return u(n, k) + u(n, k + 1)


def leaf_cases():
    """(n, k, index, B, gain, spread): every reachable (N >= 2, K), the first, last, middle and four random indices, every block
    count in {1, 2, 4, 8, 16} that divides N, spread 0 .. 3, a gain drawn per case."""
    rng = np.random.default_rng(8)
    pairs = [(n, k) for n, k in reachable_nk() if n >= 2]  # N = 1 bands carry a sign bit, not a PVQ codeword
    assert len(pairs) > 300 and max(n for n, _ in pairs) == 176
    for n, k in pairs:
        v = _v(n, k)
        assert 0 < v <= 0xFFFFFFFF, (n, k, v)  # a legal (N, K) has a 32-bit codebook
        idxs = {0, v - 1, v // 2} | {int(x) for x in rng.integers(0, v, 4)}
        blocks = [bb for bb in (1, 2, 4, 8, 16) if n % bb == 0 and n // bb >= 1]
        for index in idxs:
            for B in blocks:
                for spread in (0, 1, 2, 3):
                    gain = int(rng.choice([32767, 16384, 23170, 1, 12345]))
                    yield n, k, index, B, gain, spread


def sparse_leaf_cases():
    """(n, k, index, 1, 32767, 0): every reachable (N, K) with more than one dimension per pulse, many indices each -- random ones,
    the first and last, and the ones around every U(N, j) and U(N - 1, j) boundary, where a run of zeros ends or a sign flips."""
    rng = np.random.default_rng(18)
    memo = {}
    _v(2, 2, memo)

    def u(x, y):
        _v(x, y, memo)
        return memo[(x, y)]
    for n, k in [(n, k) for n, k in reachable_nk() if n >= 4 and n > k]:
        v = _v(n, k, memo)
        idxs = {0, 1, v - 1, v - 2} | {int(x) for x in rng.integers(0, v, 60)}
        for j in range(1, k + 2):
            for d in (-1, 0, 1):
                idxs.add(u(n, j) + d)
                idxs.add(u(n - 1, j) + d)
        for index in sorted(x for x in idxs if 0 <= x < v):
            yield n, k, index, 1, 32767, 0
