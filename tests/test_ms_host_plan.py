"""The plan of the multistream host path (csrc/og_ms_framing.hpp) on the CPU: what opusgpu_ms_decode_packets decides about a call --
every refusal, the frames of every (packet, elementary stream), the arena, step k's tables of the two halves, what the returned
codes do to the next table, the results handed to k_ms_map -- and the stream memory.  tests/emul/og_ms_framing_test.cpp puts the
header behind a C interface; this test PLAYS THE DEVICE: for every frame of a step table it returns 960 (reference mode) or the
frame's duration (RFC mode), and for chosen (packet, stream, k) a negative code instead.  Nothing of the GPU is needed.

The expected values come from elsewhere: the oracle's parser in self-delimited mode (_oracle_validate of test_ms_framing.py),
libog_framing_test.so's ft_plan for what ONE elementary packet or one empty packet does to one stream (flags, stream memory), and
the rules of opus_multistream_packet_validate / opus_multistream_decode_native (src/opus_decoder.cpp:803-823, :840-880) restated in
expected_code() and half_index() below.

What this cannot see: that the call around the plan (csrc/og_ms.hpp) uploads these tables and bytes and launches on them --
tests/test_gpu_multistream.py checks that on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import ms_util
import rfc_common
from test_host_framing import BAD_ARG, CAPS, DUR_OF_CODE, INVALID, REF, RFC, TOO_SMALL, Desc, ft, plan  # noqa: F401 (ft: a fixture)
from test_ms_framing import _oracle_validate

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "emul", "libog_ms_framing_test.so")
N_DEC = 4
CELT_BAD = -18  # what a one-byte CELT frame returns: the code the played device injects
i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def mt():
    lib = C.CDLL(LIB)
    lib.mt_new.restype = C.c_void_p
    lib.mt_new.argtypes = [C.c_void_p, C.c_int]
    lib.mt_free.argtypes = [C.c_void_p]
    lib.mt_half.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, i32p]
    lib.mt_memory.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.mt_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mt_plan_get.argtypes = [C.c_void_p] + [C.c_void_p] * 5
    lib.mt_frames.argtypes = [C.c_void_p, C.c_void_p]
    lib.mt_arena.restype = C.c_int64
    lib.mt_arena.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.mt_step.argtypes = [C.c_void_p, C.c_int, i32p]
    lib.mt_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mt_fold.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.mt_results.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


# ---- the rules, restated ------------------------------------------------------------------------------------------------------------
def half_index(layout, d, s):
    """-> (half, the half's stream / row of (decoder or packet d, elementary stream s)): coupled streams on the 2-channel context,
    mono streams on the 1-channel one (include/opusgpu.h MULTISTREAM)"""
    _, S, coupled, _ = layout
    return (0, d * coupled + s) if s < coupled else (1, d * (S - coupled) + (s - coupled))


def expected_code(layout, mode, cap, decoder, length, pk, oracle):
    """-> (code, [[(offset, len)] per stream]) of a packet that is not empty.  The decoder and the length (opusgpu.h), then
    opus_multistream_decode_native: the packet's validation (:803-823, :855-865) -- with the documented reference-mode refusal of
    unequal frame counts --, its samples against frame_size = min(capacity x 960, 5760) (:840, :845-847), and in reference mode, where
    every frame decodes as 960 samples, the frame count against the capacity and the 40 / 60 ms frames that the second stream's check
    fails (:880)."""
    _, S, _, _ = layout
    if decoder < 0 or decoder >= N_DEC or length < 0:
        return BAD_ARG, None
    samples, frames = _oracle_validate(oracle, pk, S)
    if samples < 0:
        return samples, None
    if mode == REF and len({len(f) for f in frames}) > 1:
        return INVALID, None
    if samples > min(cap * 960, 5760):
        return TOO_SMALL, None
    if mode == REF and (len(frames[0]) > cap or (S > 1 and rfc_common.dur(pk[0]) > 960)):
        return TOO_SMALL, None
    return 0, frames


# ---- packets ------------------------------------------------------------------------------------------------------------------------
CELT20 = bytes([0x98]) + bytes(10)
# (TOC configuration, samples per frame): SILK NB 10 / 20 / 40 / 60 ms, hybrid 10 / 20 ms, CELT 2.5 / 5 / 10 / 20 ms
CONFIGS = [(0x00, 480), (0x08, 960), (0x10, 1920), (0x18, 2880), (0x60, 480), (0x68, 960), (0x80, 120), (0x88, 240), (0x90, 480), (0xF8, 960)]


def _ms(pkg, el):
    return ms_util.ms_packet(pkg, el)


def decodable(rng, pkg, layout, mode, cap):
    """elementary packets of one duration that the call has room for -> (elementary packets, frames of the longest one)"""
    _, S, _, _ = layout
    for _ in range(100):
        toc, spf = CONFIGS[int(rng.integers(len(CONFIGS)))]
        frames = int(rng.choice([1, 1, 2, 2, 3, 4, 6]))
        if frames * spf > cap * 960 or (mode == REF and (frames > cap or (S > 1 and spf > 960))):
            continue
        counts = [frames] * S
        if mode == RFC and S > 1 and frames % 2 == 0 and spf * 2 in (240, 480, 960) and rng.random() < 0.3:
            counts[int(rng.integers(S))] = frames // 2  # RFC mode: equal durations, unequal frame counts (twice the frame size)
        el = []
        for s in range(S):
            t = toc if counts[s] == frames else next(c for c, f in CONFIGS if f == spf * 2 and (c & 0x80) == (toc & 0x80) or (f == spf * 2 == 960 and c == 0xF8))
            el.append(ms_util.elementary_packet(rng, t | int(rng.integers(2)) << 2, counts[s], vbr=bool(rng.random() < 0.5),
                                                pad=int(rng.choice([0, 0, 3])) if counts[s] > 2 else 0))
        return el, frames
    return [ms_util.elementary_packet(rng, 0xF8, 1) for _ in range(S)], 1


def refusal(rng, pkg, layout, mode, cap, kind):
    """-> (decoder, length or None for the packet's own, packet) of the refusal kinds of the issue, or None where the layout, the
    mode or the capacity has no such packet"""
    _, S, _, _ = layout
    sd20 = ms_util.self_delimit(pkg, CELT20)
    good = _ms(pkg, [CELT20] * S)
    d = int(rng.integers(N_DEC))
    if kind == "decoder id":
        return int(rng.choice([-1, N_DEC, N_DEC + 7])), None, good
    if kind == "negative length":
        return d, -int(rng.integers(1, 5)), good
    if kind == "invalid: too short" and S >= 2:  # len < 2 * streams - 1 (:855)
        return d, None, bytes([0x98, 0] * (S - 1))
    if kind == "invalid: missing stream" and S >= 2:  # the streams before the last use every byte (:810)
        return d, None, sd20 * (S - 1)  # (12 bytes per stream: never the length rule above)
    if kind == "invalid: durations differ" and S >= 2:  # (:817)
        return d, None, sd20 * (S - 1) + bytes([0x90]) + bytes(4)
    if kind == "invalid: longer than 120 ms":  # code 3, 7 frames of 20 ms
        return d, None, sd20 * (S - 1) + bytes([0x9B, 7]) + bytes(7)
    if kind == "invalid: size past the end" and S >= 2:  # a self-delimited size past the end (:645-647)
        return d, None, bytes([0x98, 200]) + bytes(5) + sd20 * (S - 2) + CELT20
    if kind == "invalid: odd code 1":  # code 1 with an odd payload in the last (standard) stream
        return d, None, sd20 * (S - 1) + bytes([0x91, 1, 2, 3])
    if kind == "invalid: frame counts differ" and S >= 2 and mode == REF:  # 2 x 10 ms | 1 x 20 ms
        return d, None, ms_util.self_delimit(pkg, bytes([0x91]) + bytes(8)) + sd20 * (S - 2) + CELT20
    if kind == "too small: samples":  # more samples than min(capacity x 960, 5760)
        if cap == 6:
            return None  # (no packet that the parser lets through exceeds 5760 samples)
        return d, None, _ms(pkg, [ms_util.elementary_packet(rng, 0xF8, cap + 1) for _ in range(S)])  # 20 ms frames
    if kind == "too small: frames" and mode == REF and cap < 6:  # 10 ms frames: the samples fit, the frames do not
        frames = {1: 2, 2: 3, 3: 4}[cap]
        return d, None, _ms(pkg, [ms_util.elementary_packet(rng, 0x90, frames) for _ in range(S)])
    if kind == "too small: 40 / 60 ms" and mode == REF and S >= 2 and cap >= 2:
        toc = 0x10 if cap == 2 or rng.random() < 0.5 else 0x18
        return d, None, _ms(pkg, [ms_util.elementary_packet(rng, toc, 1) for _ in range(S)])
    return None


KINDS = ["decoder id", "negative length", "invalid: too short", "invalid: missing stream", "invalid: durations differ",
         "invalid: longer than 120 ms", "invalid: size past the end", "invalid: odd code 1", "invalid: frame counts differ",
         "too small: samples", "too small: frames", "too small: 40 / 60 ms"]
WANT_OF_KIND = {k: BAD_ARG if k in KINDS[:2] else INVALID if k.startswith("invalid") else TOO_SMALL for k in KINDS}


# ---- one call -----------------------------------------------------------------------------------------------------------------------
class Model:
    """the oracle side of one Mt: the stream memory per (decoder, stream) as ft_plan leaves it"""

    def __init__(self, layout):
        self.layout = layout
        self.mem = {(d, s): (0, 0) for d in range(N_DEC) for s in range(layout[1])}

    def memory_arrays(self, h):
        _, S, coupled, _ = self.layout
        hs = coupled if h == 0 else S - coupled
        lc, lf = np.zeros(N_DEC * hs, np.int32), np.zeros(N_DEC * hs, np.int32)
        for (d, s), (c, f) in self.mem.items():
            hh, e = half_index(self.layout, d, s)
            if hh == h:
                lc[e], lf[e] = c, f
        return lc, lf


def check_memory(mt, h, model, tag):
    for half in range(2):
        want_lc, want_lf = model.memory_arrays(half)
        lc, lf = np.zeros(len(want_lc) + 1, np.int32), np.zeros(len(want_lc) + 1, np.int32)
        assert mt.mt_memory(h, half, lc.ctypes.data, lf.ctypes.data) == len(want_lc)
        assert np.array_equal(lc[:-1], want_lc) and np.array_equal(lf[:-1], want_lf), (tag, "stream memory of half", half)


def run_call(mt, ft, oracle, h, model, mode, cap, items, rng, stats, tag):
    """items: [(decoder, length or None, packet bytes or None: empty, elementary packets or None, kind)].  Plans the call, checks the
    plan against the model, then plays the device step by step."""
    layout = model.layout
    _, S, coupled, _ = layout
    n = len(items)
    n_streams = [N_DEC * coupled, N_DEC * (S - coupled)]
    # -- the model: per (packet, stream) the expected descriptors (arena base added below) and the packet's code
    want_code, want_descs, base = [], [], [0]
    mem_before = dict(model.mem)
    for i, (d, length, pk, el, kind) in enumerate(items):
        empty = pk is None or len(pk) == 0
        ln = (0 if empty else len(pk)) if length is None else length
        base.append(base[-1] + (0 if empty or ln < 0 else ln))
        per_stream = [[] for _ in range(S)]
        if empty and 0 <= d < N_DEC and ln >= 0:
            # every stream as ft_plan(None) frames it from ITS memory: min(capacity, 6) passes of 960 in reference mode
            code = 0
            for s in range(S):
                hh, e = half_index(layout, d, s)
                p, descs = plan(ft, None, mode=mode, channels=2 if hh == 0 else 1, cap=cap if mode == RFC else min(cap, 6),
                                last=model.mem[(d, s)], stream=e, n_streams=n_streams[hh], arena_base=0)
                assert (p["last_count"], p["last_flags"]) == model.mem[(d, s)]
                code = p["code"] or code
                per_stream[s] = descs
                stats["empty, no packet yet"] += model.mem[(d, s)][0] == 0
            stats["empty refused"] += code != 0
            stats[("empty", mode)] += 1
        else:
            code, frames = expected_code(layout, mode, cap, d, ln, pk, oracle)
            if kind in WANT_OF_KIND:
                assert code == WANT_OF_KIND[kind], (tag, i, kind, code)  # (the generator made what it meant to make)
                stats[kind] += 1
            if code == 0:
                for s in range(S):
                    hh, e = half_index(layout, d, s)
                    p, own = plan(ft, el[s], mode=mode, channels=2 if hh == 0 else 1, cap=48, last=model.mem[(d, s)], stream=e,
                                  n_streams=n_streams[hh], arena_base=0)
                    assert p["code"] == 0 and p["frames"] == len(frames[s]), (tag, i, s, p)
                    per_stream[s] = [(e, base[i] + o, ln_, own[k][3]) for k, (o, ln_) in enumerate(frames[s])]
                    model.mem[(d, s)] = (p["last_count"], p["last_flags"])
                stats["decoded"] += 1
        if code:
            per_stream = [[] for _ in range(S)]
        want_code.append(code)
        want_descs.append(per_stream)
    # -- the plan
    blob = b"".join(b"" if it[2] is None else it[2] for it in items) + b"\0"
    buf = np.frombuffer(blob, dtype=np.uint8)
    ptrs, lens, at = np.zeros(n, np.uint64), np.zeros(n, np.int32), 0
    for i, (d, length, pk, el, kind) in enumerate(items):
        ptrs[i] = 0 if pk is None else buf.ctypes.data + at
        lens[i] = (0 if pk is None else len(pk)) if length is None else length
        at += 0 if pk is None else len(pk)
    ids = np.array([it[0] for it in items], np.int32)
    assert mt.mt_plan(h, mode, cap, n, ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data) == 0
    first, cnt, eres, placed = (np.zeros(n * S, np.int32) for _ in range(4))
    got_base = np.zeros(n + 1, np.int64)
    total = mt.mt_plan_get(h, first.ctypes.data, cnt.ctypes.data, eres.ctypes.data, placed.ctypes.data, got_base.ctypes.data)
    flat = [x for per in want_descs for f in per for x in f]
    assert total == len(flat), (tag, total, len(flat))
    fd = (Desc * max(total, 1))()
    mt.mt_frames(h, fd)
    # 4. refusals are decided here, before the first step: the code in every stream, no descriptor, the memory untouched
    assert [(x.stream, x.offset, x.len, x.flags) for x in fd[:total]] == flat, tag
    assert list(got_base) == base, tag
    assert not placed.any()
    at = 0
    for i in range(n):
        for s in range(S):
            e = i * S + s
            assert (first[e], cnt[e], eres[e]) == (at, len(want_descs[i][s]), want_code[i]), (tag, i, s, items[i][4])
            at += cnt[e]
    # (the model's memory moves with decoded packets alone) 5. ... where it is what ft_plan left for each elementary packet alone
    check_memory(mt, h, model, tag)
    # 6. the arena: bytes at the prefix sums, nothing for empty packets, 16 zero bytes of tail
    arena = np.full(base[-1] + 16 + 8, 0xAB, np.uint8)
    assert mt.mt_arena(h, ptrs.ctypes.data, arena.ctypes.data, len(arena)) == base[-1] + 16
    for i, it in enumerate(items):
        assert arena[base[i]:base[i + 1]].tobytes() == (b"" if base[i + 1] == base[i] else it[2]), (tag, i)
    assert not arena[base[-1]:base[-1] + 16].any() and (arena[base[-1] + 16:] == 0xAB).all()
    # 7. the layouts of one stream: the plain host path's plan, packet for packet
    if S == 1:
        mem = dict(mem_before)
        for i, (d, length, pk, el, kind) in enumerate(items):
            ln = (0 if pk is None else len(pk)) if length is None else length
            out, dd = (C.c_int32 * 8)(), (Desc * 64)()
            last = mem.get((d, 0), (0, 0))
            r = ft.ft_plan(pk if pk else None, ln, d, N_DEC, mode, 0, layout[0], cap, last[0], last[1], base[i], out, dd, 64)
            assert (out[0], r) == (want_code[i], cnt[i]), (tag, i, kind, out[0], want_code[i])
            assert [(x.stream, x.offset, x.len, x.flags) for x in dd[:r]] == want_descs[i][0], (tag, i)
            if 0 <= d < N_DEC:
                mem[(d, 0)] = (out[6], out[7])
        assert mem == model.mem
    # -- the steps: this test is the device
    fail_at = {}
    for i, per in enumerate(want_descs):
        longest = max(len(f) for f in per)
        if want_code[i] == 0 and items[i][2] and longest > 1 and rng.random() < 0.4:
            s = int(rng.choice([s for s in range(S) if len(per[s]) > 1]))
            fail_at[(i, s)] = int(rng.integers(1, len(per[s])))
            stats["failure at k >= 1"] += 1
        elif want_code[i] == 0 and rng.random() < 0.08:
            fail_at[(i, int(rng.integers(S)))] = 0
    m_eres = {(i, s): want_code[i] for i in range(n) for s in range(S)}
    m_placed = dict.fromkeys(m_eres, 0)
    k = 0
    while True:
        m = (C.c_int32 * 2)()
        more = mt.mt_step(h, k, m)
        assert more in (0, 1)
        # 1. frame k of every (packet, stream) with more than k frames and no failure so far, in (packet, stream) order, by half
        want = [[], []]
        for i in range(n):
            for s in range(S):
                if len(want_descs[i][s]) > k and m_eres[(i, s)] >= 0:
                    hh, row = half_index(layout, i, s)
                    want[hh].append((want_descs[i][s][k], (row, m_placed[(i, s)]), i * S + s))
        assert [m[0], m[1]] == [len(want[0]), len(want[1])], (tag, k)
        assert bool(more) == bool(want[0] or want[1])
        if not more:
            break
        for hh in range(2):
            tab, place, owner = (Desc * max(m[hh], 1))(), np.zeros(2 * m[hh], np.int32), np.zeros(m[hh], np.int32)
            mt.mt_table(h, hh, tab, place.ctypes.data, owner.ctypes.data)
            assert [(x.stream, x.offset, x.len, x.flags) for x in tab[:m[hh]]] == [w[0] for w in want[hh]], (tag, k, hh)
            assert place.reshape(-1, 2).tolist() == [list(w[1]) for w in want[hh]], (tag, k, hh)  # 2. (row, samples so far)
            assert owner.tolist() == [w[2] for w in want[hh]]
            got = np.zeros(m[hh], np.int32)
            for j, (desc, _, e) in enumerate(want[hh]):
                i, s = divmod(e, S)
                got[j] = CELT_BAD if fail_at.get((i, s)) == k else 960 if mode == REF else DUR_OF_CODE[desc[3] >> 6 & 7]
                if got[j] < 0:  # 3. a failure ends that stream's packet and no other's
                    m_eres[(i, s)] = int(got[j])
                else:
                    m_eres[(i, s)] += int(got[j])
                    m_placed[(i, s)] += int(got[j])
            mt.mt_fold(h, hh, got.ctypes.data)
        k += 1
        assert k <= 48
    mt.mt_plan_get(h, first.ctypes.data, cnt.ctypes.data, eres.ctypes.data, placed.ctypes.data, got_base.ctypes.data)
    assert eres.tolist() == [m_eres[(i, s)] for i in range(n) for s in range(S)], tag
    assert placed.tolist() == [m_placed[(i, s)] for i in range(n) for s in range(S)], tag
    for hh in range(2):  # ... and the split arrays handed to the map
        hs = coupled if hh == 0 else S - coupled
        want_r = np.zeros(n * hs, np.int32)
        for (i, s), v in m_eres.items():
            if half_index(layout, i, s)[0] == hh:
                want_r[half_index(layout, i, s)[1]] = v
        r = np.full(n * hs + 1, 77, np.int32)
        assert mt.mt_results(h, hh, r.ctypes.data) == n * hs and np.array_equal(r[:-1], want_r) and r[-1] == 77, (tag, hh)


def test_half_rule_known_answers(mt, pkg):
    """5.1: streams 0, 1 coupled, 2, 3 mono; decoder 3's stream 1 is stream 7 of the stereo context, its stream 3 stream 7 of the mono one"""
    lay = pkg.ms_layout(*ms_util.LAYOUTS["5.1"])
    out = (C.c_int32 * 3)()
    assert mt.mt_half(C.byref(lay), 0, 3, 1, out) == 7 and list(out) == [0, 2, 2]
    assert mt.mt_half(C.byref(lay), 1, 3, 3, out) == 7 and list(out) == [2, 2, 1]
    assert mt.mt_half(C.byref(lay), 1, 0, 2, out) == 0
    lay = pkg.ms_layout(*ms_util.LAYOUTS["family255-mono8"])
    assert mt.mt_half(C.byref(lay), 0, 0, 0, out) == 0 and list(out) == [0, 0, 2]  # an absent half
    assert mt.mt_half(C.byref(lay), 1, 2, 5, out) == 21 and list(out) == [0, 8, 1]
    assert mt.mt_new(C.byref(pkg.ms_layout(2, 1, 2, [0, 1])), 4) is None  # (ms_layout_ok: coupled > streams)


def test_ms_host_plan_walk(mt, ft, pkg, oracle):
    """every layout of ms_util.LAYOUTS x both modes: calls of decodable, empty / lost and refused packets on four decoders"""
    rng = np.random.default_rng(2024)
    stats = dict.fromkeys(KINDS + ["decoded", "failure at k >= 1", "empty, no packet yet", "empty refused", ("empty", REF), ("empty", RFC)], 0)
    for name, layout in ms_util.LAYOUTS.items():
        lay = pkg.ms_layout(*layout)
        for mode in (REF, RFC):
            h = mt.mt_new(C.byref(lay), N_DEC)
            assert h
            model = Model(layout)
            for call in range(14):
                cap = int(rng.choice(CAPS))
                items = []
                for i in range(10):
                    u = rng.random()
                    kind = KINDS[int(rng.integers(len(KINDS)))]
                    made = refusal(rng, pkg, layout, mode, cap, kind) if u < 0.42 else None
                    if made:
                        items.append(made + (None, kind))
                    elif u < 0.6 and call > 0 or u < 0.47:
                        items.append((int(rng.integers(N_DEC)), None, None if rng.random() < 0.5 else b"", None, "empty"))
                    else:
                        el, _ = decodable(rng, pkg, layout, mode, cap)
                        items.append((int(rng.integers(N_DEC)), None, _ms(pkg, el), el, "decodable"))
                run_call(mt, ft, oracle, h, model, mode, cap, items, rng, stats, (name, mode, call))
            mt.mt_free(h)
    # the walk cannot pass by skipping: the oracle-side model alone counts these
    assert stats["decoded"] >= 300, stats
    assert all(stats[k] >= 20 for k in KINDS), stats
    assert stats["failure at k >= 1"] >= 50, stats
    assert stats[("empty", REF)] >= 50 and stats[("empty", RFC)] >= 50, stats
    assert stats["empty, no packet yet"] >= 20 and stats["empty refused"] >= 5, stats
