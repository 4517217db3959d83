"""Cases, exact references and comparators of the device known-answer tests (tests/test_gpu_device_forms.py runs them on the GPU,
tests/test_device_form_cases.py checks on the CPU that they are what they claim to be and that the comparators see a difference).
The references are Python integers, numpy int64 or the oracle's plain C -- never the host emulation."""
import ctypes as C
import itertools
import math
import os

import numpy as np

import pvq_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT_LIB = os.path.join(ROOT, "tests", "gpu_kat", "libog_gpu_kat.so")
M32 = 0xFFFFFFFF


def load_kat():
    """The device known-answer library (tests/gpu_kat), built by build() -- never here, never on the GPU box."""
    assert os.path.exists(KAT_LIB), "tests/gpu_kat/libog_gpu_kat.so is missing: run build() (__graft_entry__.py)"
    lib = C.CDLL(KAT_LIB)
    vp = C.c_void_p
    for name in ("gk_pvq_u3", "gk_pvq_isqrt_near", "gk_pvq_block_mul", "gk_pvq_block_of", "gk_mul16x32_q15", "gk_smulwb", "gk_rot_dot2",
                 "gk_add3", "gk_pk_sub_i16", "gk_rs_dot2", "gk_wave_sum", "gk_wave_or", "gk_wave_scan_add", "gk_wave_scan_max", "gk_pvq_tab"):
        getattr(lib, name).argtypes = [vp, vp, C.c_int]
    lib.gk_rc_icdf.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_uint]
    lib.gk_rc_lane_bytes.argtypes = [vp, C.c_int, vp]
    lib.gk_leaf_layout.argtypes = [vp]
    lib.gk_leaf_layout.restype = None
    lib.gk_pvq_leaves_check.argtypes = [vp, C.c_int]
    lib.gk_pvq_leaves.argtypes = [vp, vp, vp, C.c_int]
    return lib


def s16(x):
    return ((x & 0xFFFF) ^ 0x8000) - 0x8000


def s32(x):
    return ((x & M32) ^ 0x80000000) - 0x80000000


# ---- (a) lane primitives -------------------------------------------------------------------------------------------------------
PRIM_IN, PRIM_OUT = 5, 2
# 0, +-1, +-2^15, 2^15 - 1, +-(2^31 - 1), INT32_MIN, and 16-bit operands with garbage in the upper half
EDGE32 = [0, 1, -1, 1 << 15, -(1 << 15), (1 << 15) - 1, (1 << 31) - 1, -((1 << 31) - 1), -(1 << 31),
          0x12340000, 0x12340001, 0x1234FFFF, 0x00018000, 0xABCD8000, 0x00017FFF, 0xFFFE7FFF, 0xFFFF0000]
EDGE16 = [0, 1, -1, 32767, -32768, 0x12348000, 0xFFFF0001, 0x00017FFF]  # what reaches a 16-bit operand's register
N_RANDOM = 4096


def _rows(tuples):
    a = np.zeros((len(tuples), PRIM_IN), dtype=np.uint32)
    for c in range(len(tuples[0])):
        a[:, c] = np.array([t[c] & M32 for t in tuples], dtype=np.uint64).astype(np.uint32)
    return a


def _random_words(seed, n, cols):
    return [tuple(int(x) for x in row) for row in np.random.default_rng(seed).integers(0, 1 << 32, (n, cols), dtype=np.uint64)]


def prim_cases():
    """name -> (entry point, input rows [n, 5] uint32, expected first output word as a list of Python ints, or None where the test
    states a contract instead)."""
    out = {}
    hs = [(h,) for h in range(1, 2048)]
    out["pvq_u3"] = ("gk_pvq_u3", _rows(hs), [(2 * h * (h - 1) + 1) & M32 for (h,) in hs])
    out["pvq_isqrt_near"] = ("gk_pvq_isqrt_near", _rows([(t,) for t in range(176 * 176 + 1)]), None)
    out["pvq_block_mul"] = ("gk_pvq_block_mul", _rows([(b,) for b in range(1, 177)]), None)
    jb = [(j, b) for b in range(1, 177) for j in range(176)]
    out["pvq_block_of"] = ("gk_pvq_block_of", _rows(jb), [j // b for j, b in jb])
    pairs = list(itertools.product(EDGE32, EDGE32)) + _random_words(101, N_RANDOM, 2)
    out["mul16x32_q15"] = ("gk_mul16x32_q15", _rows(pairs), [((s16(a) * s32(b)) >> 15) & M32 for a, b in pairs])
    out["smulwb"] = ("gk_smulwb", _rows(pairs), [((s32(a) * s16(b)) >> 16) & M32 for a, b in pairs])
    # rot_dot2 on rot_pack'ed pairs: (x1 c1 + x2 c2 + half) in WRAPPING 32-bit arithmetic, then >> 15
    halves = [16384, 0, -1, (1 << 31) - 1, -(1 << 31)]
    quads = [q + (h,) for q in itertools.product(EDGE16, repeat=4) for h in halves] + _random_words(102, N_RANDOM, 5)
    quads.append((-32768, -32768, -32768, -32768, 16384))  # (-32768 x -32768) x 2 + half: past 2^31
    out["rot_dot2"] = ("gk_rot_dot2", _rows(quads), [(s32(s16(a) * s16(c) + s16(b) * s16(d) + s32(e)) >> 15) & M32 for a, b, c, d, e in quads])
    out["rot_pack"] = ("gk_rot_dot2", _rows(quads), [(a & 0xFFFF) | (b & 0xFFFF) << 16 for a, b, c, d, e in quads])  # second word
    triples = list(itertools.product(EDGE32, repeat=3)) + _random_words(103, N_RANDOM, 3)
    out["og_add3"] = ("gk_add3", _rows(triples), [(a + b + c) & M32 for a, b, c in triples])
    h16 = [0, 1, 0xFFFF, 0x7FFF, 0x8000]
    packed = [lo | hi << 16 for lo in h16 for hi in h16]
    pk = list(itertools.product(packed, packed)) + _random_words(104, N_RANDOM, 2)
    # per half, no saturation: 0x8000 - 1 = 0x7FFF, 0x7FFF - 0xFFFF = 0x8000
    out["og_pk_sub_i16"] = ("gk_pk_sub_i16", _rows(pk), [((a - b) & 0xFFFF) | (((a >> 16) - (b >> 16)) & 0xFFFF) << 16 for a, b in pk])
    accs = [0, 16384, -1, (1 << 31) - 1, -(1 << 31)]
    rs = [(x, t, a) for x in packed for t in packed for a in accs] + _random_words(105, N_RANDOM, 3)
    out["rs_dot2"] = ("gk_rs_dot2", _rows(rs), [(s32(c) + s16(a) * s16(b) + s16(a >> 16) * s16(b >> 16)) & M32 for a, b, c in rs])
    return out


def isqrt_violations(tq, r):
    """Where r is neither floor(sqrt(tq)) nor, at a perfect square only, one less: the contract of pvq_isqrt_near's caller.
    Returns (violating tq, tq where r is the floor minus one)."""
    tq, r = np.asarray(tq, dtype=np.int64), np.asarray(r, dtype=np.int64)
    fl = np.array([math.isqrt(int(t)) for t in tq], dtype=np.int64)
    low = (r == fl - 1)
    bad = ~((r == fl) | (low & (fl * fl == tq)))
    return [int(t) for t in tq[bad]], [int(t) for t in tq[low]]


def block_mul_violations(blen, m):
    """Where M is neither floor(65536 / blen) + 1 nor that plus one.  Returns (violating blen, blen with the larger M)."""
    blen, m = np.asarray(blen, dtype=np.int64), np.asarray(m, dtype=np.int64)
    base = 65536 // blen + 1
    return [int(b) for b in blen[(m != base) & (m != base + 1)]], [int(b) for b in blen[m == base + 1]]


def mismatches(got, want):
    """Flat indices at which two word arrays differ."""
    got, want = np.asarray(got).astype(np.int64) & M32, np.asarray(want, dtype=np.int64) & M32
    assert got.shape == want.shape, (got.shape, want.shape)
    return [int(i) for i in np.flatnonzero(got.ravel() != want.ravel())]


# ---- (b) wave helpers ----------------------------------------------------------------------------------------------------------
SEAMS = (0, 63, 15, 16, 31, 32, 47, 48)


def wave_vectors():
    """(vectors for sum / or / prefix sum [n, 64] int32, vectors for the prefix maximum: the same kinds, values >= 0)."""
    rng = np.random.default_rng(7)
    any_v, pos_v = [], []
    for lane in range(64):  # the unit vectors
        for val in (lane + 1, 0x7FFFFFFF):
            v = np.zeros(64, dtype=np.int64)
            v[lane] = val
            any_v.append(v)
            pos_v.append(v)
        v = np.zeros(64, dtype=np.int64)
        v[lane] = -(1 << 31)
        any_v.append(v)
    for v in (np.ones(64, dtype=np.int64), np.arange(64, dtype=np.int64), np.arange(64, dtype=np.int64)[::-1].copy(), np.arange(1, 65, dtype=np.int64) * 1000003):
        any_v.append(v)
        pos_v.append(v)
    # marker rows as pvq_rotate_wave makes them: zeros, and a leaf's number (its lane + 1, or the largest byte) where its items start
    groups = [(0,), (63,), (15,), (16,), (31,), (32,), (47,), (48,), (15, 16), (31, 32), (47, 48), (0, 63), SEAMS]
    for g in groups:
        for top in (False, True):
            v = np.zeros(64, dtype=np.int64)
            for lane in g:
                v[lane] = 255 if top else lane + 1
            any_v.append(v)
            pos_v.append(v)
    for _ in range(256):
        any_v.append(rng.integers(-(1 << 31), 1 << 31, 64))  # (sums that wrap 32 bits)
        pos_v.append(rng.integers(0, 1 << 31, 64) >> int(rng.integers(0, 31)))
    any_v.append(np.full(64, 0x7FFFFFFF, dtype=np.int64))  # a sum that wraps for certain
    any_v.append(np.full(64, -(1 << 31), dtype=np.int64))
    return np.array(any_v, dtype=np.int64).astype(np.int32), np.array(pos_v, dtype=np.int64).astype(np.int32)


def wave_reference(op, v):
    """Every lane's result, in int64 wrapped to 32 bits."""
    v = np.asarray(v).astype(np.int64)
    if op == "sum":
        r = np.repeat(v.sum(axis=1, keepdims=True), 64, axis=1)
    elif op == "or":
        r = np.repeat(np.bitwise_or.reduce(v & M32, axis=1, keepdims=True), 64, axis=1)
    elif op == "scan_add":
        r = np.cumsum(v, axis=1)
    else:
        r = np.maximum.accumulate(v, axis=1)
    return r & M32


# ---- (c) PVQ leaves: lists, waves, reference, comparator -----------------------------------------------------------------------
LEAF_WORDS = 8
_lists = {}


def leaf_lists():
    """The two case lists of tests/test_pvq_kat.py, joined: (cases, length of the first list)."""
    if "c" not in _lists:
        a = list(pvq_cases.leaf_cases())
        b = list(pvq_cases.sparse_leaf_cases())
        _lists["c"] = (a + b, len(a))
    return _lists["c"]


def leaf_reference(oracle):
    """oc_test_pvq_leaf of every case, once: (coefficients [cases, 176] int16, masks [cases] uint32).  Read-only."""
    if "r" not in _lists:
        cases, _ = leaf_lists()
        f = oracle.lib.oc_test_pvq_leaf
        f.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_void_p]
        f.restype = C.c_uint
        coef = np.zeros((len(cases), 176), dtype=np.int16)
        mask = np.zeros(len(cases), dtype=np.uint32)
        for ci, (n, k, index, B, gain, spread) in enumerate(cases):
            mask[ci] = f(n, k, index, spread, B, gain, coef[ci].ctypes.data)
        coef.setflags(write=False)
        mask.setflags(write=False)
        _lists["r"] = (coef, mask)
    return _lists["r"]


def rot_items(case):
    """(items of the wide-stride pass, items of the stride-1 pass) a leaf hands to pvq_rotate_wave: RotJob's rule, chains << logB
    (og_celt_recon.hpp); (0, 0) for a leaf without a rotation."""
    n, k, _, B, _, spread = case
    if not (2 * k < n and spread != 0):
        return 0, 0
    blen, log_b = n // B, B.bit_length() - 1
    stride2 = 0
    if n >= 8 * B:
        stride2 = 1
        while (stride2 * stride2 + stride2) * B + (B >> 2) < n:
            stride2 += 1
    wide = max(0, min(stride2, blen - stride2)) if stride2 else 0
    return wide << log_b, int(blen >= 2) << log_b


def pack_waves(order, cases, layout, per_wave=64):
    """Leaves at consecutive positions inside the two ranges layout = (lo0, hi0, lo1, hi1, row), one leaf per lane, a new wave when
    the lanes or the room run out.  Returns (leaves [waves, 64, 8] uint32, placements [(wave, lane, pos, case index)])."""
    lo0, hi0, lo1, hi1 = layout[:4]
    waves, place = [], []
    cur, lane, pos, ch = None, 0, lo0, 0
    for ci in order:
        n = cases[ci][0]
        while True:
            if cur is None:
                cur = np.zeros((64, LEAF_WORDS), dtype=np.uint32)
                waves.append(cur)
                lane, pos, ch = 0, lo0, 0
            if lane < per_wave:
                if ch == 0 and pos + n > hi0:
                    pos, ch = lo1, 1
                if pos + n <= (hi0 if ch == 0 else hi1):
                    break
            cur = None
        nn, k, index, B, gain, spread = cases[ci]
        cur[lane] = (nn, k, index, pos, B, gain, spread, 1)
        place.append((len(waves) - 1, lane, pos, ci))
        lane += 1
        pos += n
    return (np.array(waves, dtype=np.uint32).reshape(-1, 64, LEAF_WORDS), place)


N_DIRECTED = 16  # waves of each directed kind


def leaf_compositions(layout):
    """name -> (leaves, placements): how the cases are dealt into waves (part of what pvq_rotate_wave is tested on)."""
    cases, n_first = leaf_lists()
    rot = [rot_items(c) for c in cases]
    comp = {}
    comp["order_all_nk"] = pack_waves(range(n_first), cases, layout)
    comp["order_sparse"] = pack_waves(range(n_first, len(cases)), cases, layout)
    shuffled = np.random.default_rng(2024).permutation(len(cases))  # rotated and unrotated leaves of all sizes share waves
    comp["shuffled"] = pack_waves([int(x) for x in shuffled], cases, layout)
    # directed waves, made of cases of the first list
    still = [ci for ci in range(n_first) if rot[ci] == (0, 0) and cases[ci][0] <= 12]
    turning = [ci for ci in range(n_first) if rot[ci][1] > 0]
    turning = turning[::max(1, len(turning) // (2 * N_DIRECTED))][:2 * N_DIRECTED]  # (spread over the sizes)
    assert len(still) >= 64 * 2 * N_DIRECTED and len(turning) == 2 * N_DIRECTED
    order0, order63, none = [], [], []
    for w in range(N_DIRECTED):
        order0 += [turning[w]] + still[63 * w:63 * w + 63]
        order63 += still[63 * (N_DIRECTED + w):63 * (N_DIRECTED + w) + 63] + [turning[N_DIRECTED + w]]
        none += still[64 * w:64 * w + 64]
    comp["rot_lane0_only"] = pack_waves(order0, cases, layout)
    comp["rot_lane63_only"] = pack_waves(order63, cases, layout)
    comp["no_rotation"] = pack_waves(none, cases, layout)
    # eight large leaves of 16 blocks with both sweeps: far more than 64 items in either pass
    big = [ci for ci in range(n_first) if cases[ci][0] >= 128 and cases[ci][3] == 16 and rot[ci][0] > 0 and rot[ci][1] > 0]
    big = big[::max(1, len(big) // (8 * N_DIRECTED))][:8 * N_DIRECTED]
    assert len(big) == 8 * N_DIRECTED
    comp["many_items"] = pack_waves(big, cases, layout, per_wave=8)
    return comp


def wave_item_totals(leaves_place, n_waves):
    """Per wave: (rotating leaves, items of the wide pass, items of the stride-1 pass, lanes of the rotating leaves)."""
    cases, _ = leaf_lists()
    tot = [[0, 0, 0, []] for _ in range(n_waves)]
    for w, lane, _, ci in leaves_place:
        a, b = rot_items(cases[ci])
        if a or b:
            tot[w][0] += 1
            tot[w][1] += a
            tot[w][2] += b
            tot[w][3].append(lane)
    return tot


def expected_rows(place, n_waves, row, ref_coef, ref_mask):
    """What the driver must return for a composition: every coefficient of every wave's row (zero where no leaf lies), every
    lane's mask (zero for a lane without a leaf), and which case owns a coefficient (-1: none)."""
    cases, _ = leaf_lists()
    exp = np.zeros((n_waves, row), dtype=np.int16)
    exp_mask = np.zeros((n_waves, 64), dtype=np.uint32)
    owner = np.full((n_waves, row), -1, dtype=np.int64)
    for w, lane, pos, ci in place:
        n = cases[ci][0]
        exp[w, pos:pos + n] = ref_coef[ci, :n]
        owner[w, pos:pos + n] = ci
        exp_mask[w, lane] = ref_mask[ci]
    return exp, exp_mask, owner


def compare_leaves(coef, mask, exp, exp_mask, owner, place):
    """Every difference: ("coef", wave, position, owning case or -1) and ("mask", wave, lane, case or -1)."""
    out = [("coef", int(w), int(p), int(owner[w, p])) for w, p in np.argwhere(coef != exp)]
    by_lane = {(w, lane): ci for w, lane, _, ci in place}
    out += [("mask", int(w), int(l), by_lane.get((int(w), int(l)), -1)) for w, l in np.argwhere(mask != exp_mask)]
    return out


# ---- (d) the U table in registers ------------------------------------------------------------------------------------------------
def u192_table():
    t = pvq_cases._tables()
    u = t.pvq_u_table()
    return [[u[r * 177 + c] if (r < 15 and c < 177) else 0 for c in range(192)] for r in range(16)]


def utab_queries():
    """(queries [n, 4] uint32, expected [n]): every (row, column) the registers can serve, and for every row n = 1 .. 14 the search
    at i = U(n, kk) - 1, U(n, kk), U(n, kk) + 1 for every kk of the row, bounded by kk, kk + 1 and the row's last column --
    against the linear search the emulation side of og_celt_bands.hpp runs, written out here."""
    u = u192_table()
    q, want = [], []
    for r in range(16):
        for c in range(192):
            q.append((0, r, c, 0))
            want.append(u[min(r, c)][max(r, c)])
            if c < 16 and c != r:  # (symmetric: the row may come second)
                q.append((0, c, r, 0))
                want.append(u[min(r, c)][max(r, c)])
    exact = pvq_cases._v  # U through V's memo
    memo = {}
    exact(2, 2, memo)

    def true_u(a, b):
        exact(a, b, memo)
        return memo[(a, b)]
    for n in range(1, 15):
        last = max(c for c in range(177) if true_u(n, c) < (1 << 32))  # the row is non-decreasing up to here
        for kk in range(last + 1):
            for i in (u[n][kk] - 1, u[n][kk], u[n][kk] + 1):
                if not 0 <= i <= M32:
                    continue
                for k in sorted({kk, min(kk + 1, last), last}):
                    x = k
                    while u[n][x] > i:
                        x -= 1
                    q.append((1, n, k, i))
                    want.append(x)
    return np.array(q, dtype=np.uint64).astype(np.uint32), np.array(want, dtype=np.uint64).astype(np.uint32)


# ---- (e) wave-uniform range decoding ---------------------------------------------------------------------------------------------
class RC(C.Structure):  # oc_rc, oracle/oc_opus.h
    _fields_ = [("buf", C.c_char_p), ("storage", C.c_uint32), ("end_offs", C.c_uint32), ("end_window", C.c_uint32),
                ("nend_bits", C.c_int32), ("nbits_total", C.c_int32), ("offs", C.c_uint32), ("rng", C.c_uint32), ("val", C.c_uint32),
                ("ext", C.c_uint32), ("rem", C.c_int32), ("error", C.c_int32)]


ICDF_PKT = bytes([0xA5, 0x00, 0xFF, 0x3C, 0x81, 0x7E, 0x01, 0xC3])
ICDF_RNGS = ((1 << 23) + 1, 0x00C0FFEE, 0x12345678, 0x7FFFFFFF, 1 << 31)  # 2^23 + 1, 2^31 and three values in between
# The byte tables og_silk.hpp hands to the wave form (SILK_TAB(...), the codebooks' CB1_iCDF / ec_iCDF, the shell tables, the
# pitch contours, the LTP gain tables and the stereo / LBRR ones).  A call starts anywhere a sub-table starts: every
# zero-terminated run of each is a table of its own here, and so is the one run entered one entry late (pulses_per_block's
# "+ (nLshifts == 10)").
ICDF_TABLES = ("type_vad_icdf", "type_novad_icdf", "delta_gain_icdf", "gain_icdf", "uniform8_icdf", "nb_cb1_icdf", "wb_cb1_icdf",
               "nb_cb2_icdf", "wb_cb2_icdf", "nlsf_ext_icdf", "nlsf_interp_icdf", "pitch_delta_icdf", "pitch_lag_icdf", "uniform4_icdf",
               "uniform6_icdf", "pitch_contour_icdf", "pitch_contour_nb_icdf", "pitch_contour_10ms_icdf", "pitch_contour_10ms_nb_icdf",
               "ltp_per_icdf", "ltp_gain_icdf0", "ltp_gain_icdf1", "ltp_gain_icdf2", "ltpscale_icdf", "shell0", "shell1", "shell2",
               "shell3", "rate_levels_icdf", "pulses_per_block_icdf", "lsb_icdf", "stereo_joint_icdf", "uniform3_icdf", "uniform5_icdf",
               "lbrr2_icdf", "lbrr3_icdf", "mid_only_icdf")
ICDF_PAD = 64


def icdf_tables():
    """(bytes of all tables, each with the ROM's 64 zero entries behind it; [(name, offset of a sub-table, its entries)])."""
    silk = pvq_cases._tables().SILK_TABLES
    blob, subs = bytearray(), []
    for name in ICDF_TABLES:
        ctype, vals = silk["rom_silk_" + name]
        assert ctype == "uint8_t", name
        base, start = len(blob), 0
        for i, v in enumerate(vals):
            if v == 0:
                subs.append((name, base + start, list(vals[start:i + 1])))
                start = i + 1
        assert start == len(vals), (name, "ends inside a run")
        if name == "pulses_per_block_icdf":
            subs.append((name, base + 18 * 9 + 1, list(vals[18 * 9 + 1:18 * 10])))
        blob += bytes(vals) + bytes(ICDF_PAD)
    return bytes(blob), subs


def icdf_cases():
    """[cases, 4] uint32: table offset | rng | val | rem -- for every sub-table and every rng of ICDF_RNGS, val exactly on, one
    below and one above every threshold (rng >> 8) * icdf[l], and at both ends of the state's range."""
    _, subs = icdf_tables()
    rows = []
    for si, (_, off, entries) in enumerate(subs):
        for rng in ICDF_RNGS:
            r = rng >> 8
            vals = {0, rng - 1}
            for e in entries:
                vals.update((r * e - 1, r * e, r * e + 1))
            for val in sorted(v for v in vals if 0 <= v < rng):
                rows.append((off, rng, val, (si * 37 + val) & 255))
    return np.array(rows, dtype=np.uint64).astype(np.uint32)


def icdf_reference(oracle, tabs, cases, nbits):
    """oc_rc_icdf on the same states: [cases, 6] symbol | val | rng | offs | rem | nbits_total."""
    f = C.CDLL(oracle.lib._name).oc_rc_icdf  # (a handle of its own: other tests bind this function's arguments their way)
    f.argtypes = [C.POINTER(RC), C.c_void_p, C.c_uint]
    f.restype = C.c_int
    out = np.zeros((len(cases), 6), dtype=np.uint32)
    buf = C.create_string_buffer(ICDF_PKT, len(ICDF_PKT))
    tab = C.create_string_buffer(tabs, len(tabs))
    for t, (off, rng, val, rem) in enumerate(cases.tolist()):
        rc = RC(C.cast(buf, C.c_char_p), len(ICDF_PKT), 0, 0, 0, nbits, 0, rng, val, 0, rem, 0)
        sym = f(C.byref(rc), C.addressof(tab) + off, 8)
        out[t] = (sym, rc.val, rc.rng, rc.offs, rc.rem & M32, rc.nbits_total & M32)
    return out
