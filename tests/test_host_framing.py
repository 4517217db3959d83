"""The framing of the host-buffer path (csrc/og_host_framing.hpp) on the CPU: what opusgpu_decode_packets / _fec and
opusgpu_ms_decode_packets (through csrc/og_ms_framing.hpp, tests/test_ms_host_plan.py) decide about one packet -- plan_packet: result code, frame count, kind --, the descriptors plan_descs
writes from that decision, the stream memory (last_count / last_flags) and conceal_pieces.  tests/emul/og_framing_test.cpp puts the
header behind a C interface; nothing of the GPU or its runtime is needed.

The expected values come from elsewhere: the oracle's parser (oc_packet_parse), the hand-derived table of tests/test_return_codes.py,
the rules of src/opus_decoder.cpp:323 restated here, opusgpu_empty_packet_to_frames, and tests/rfc_common.py's fec_plan /
conceal_pieces (written for the GPU parity tests).

What this cannot see: that the call around the framing (csrc/og_host_path.hpp) puts the descriptors and bytes where the prefix
sums say -- tests/test_gpu_modes.py, test_gpu_rfc.py and test_empty_packets.py check that on the device."""
import ctypes as C
import os

import numpy as np
import pytest

import ms_util
import rfc_common
from test_return_codes import KAT

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "emul", "libog_framing_test.so")
REF, RFC = 0, 1  # OPUSGPU_MODE_REFERENCE, OPUSGPU_MODE_RFC
NO_MODE = 1 << 11  # OPUSGPU_DESC_NO_MODE
BAD_ARG, TOO_SMALL, INVALID = -1, -2, -4
DECODED, EMPTY, FEC, CONCEAL_ONLY = 0, 1, 2, 3
CAPS = (1, 2, 3, 6)
DUR_OF_CODE = {0: 960, 1: 120, 2: 240, 3: 480, 4: 1920, 5: 2880}
CODE_OF_DUR = {v: k for k, v in DUR_OF_CODE.items()}


class Desc(C.Structure):
    _fields_ = [("stream", C.c_int32), ("offset", C.c_int32), ("len", C.c_int32), ("flags", C.c_int32)]


@pytest.fixture(scope="module")
def ft():
    lib = C.CDLL(LIB)
    lib.ft_plan.argtypes = [C.c_char_p] + [C.c_int32] * 10 + [C.POINTER(C.c_int32), C.POINTER(Desc), C.c_int]
    lib.ft_conceal_pieces.argtypes = [C.c_int, C.c_int, C.c_int32, C.POINTER(C.c_int32)]
    lib.ft_is_regular.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int, C.c_int]
    return lib


def plan(ft, pkt, mode=REF, fec=False, channels=2, cap=1, last=(0, 0), stream=3, n_streams=8, arena_base=1000):
    """-> (dict of the plan and the stream memory after it, [(stream, offset, len, flags)]); plan and descriptors must agree."""
    out = (C.c_int32 * 8)()
    room = 64
    d = (Desc * room)()
    r = ft.ft_plan(pkt, 0 if pkt is None else len(pkt), stream, n_streams, mode, int(fec), channels, cap, last[0], last[1], arena_base, out, d, room)
    p = dict(zip(("code", "frames", "flags", "kind", "in_arena", "pieces", "last_count", "last_flags"), out))
    assert r == p["frames"], ("plan_descs did not write exactly plan.frames descriptors", r, p)
    assert p["frames"] == 0 or p["code"] == 0, p
    return p, [(d[k].stream, d[k].offset, d[k].len, d[k].flags) for k in range(r)]


def toc_flags(toc, rfc=False):
    mode, bw = rfc_common.mode_bw(toc)
    f = (mode - 1000) | (bw - 1101) << 2 | (32 if toc & 4 else 0)
    return f | CODE_OF_DUR[rfc_common.dur(toc)] << 6 | 1 << 9 if rfc else f


def oracle_parse(oracle, pkt):
    lib = oracle.lib
    lib.oc_packet_parse.argtypes = [C.c_char_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    size = (C.c_int16 * 48)()
    toc, off = C.c_uint8(), C.c_int()
    n = lib.oc_packet_parse(pkt, len(pkt), 0, C.byref(toc), size, C.byref(off), None)
    if n < 0:
        return n, None
    at, frames = off.value, []
    for k in range(n):
        frames.append((at, size[k]))
        at += size[k]
    return n, frames


def check_normal_packet(ft, oracle, pkt, cap, last=(5, 9)):
    """Reference mode: the oracle's count / error and frames, the capacity rule (src/opus_decoder.cpp:323 on the TOC's duration, and
    one 960-sample block per frame: count <= frame_capacity), the stream memory, the regular probe."""
    n, frames = oracle_parse(oracle, pkt)
    p, descs = plan(ft, pkt, cap=cap, last=last)
    want = n if n < 0 else TOO_SMALL if (n * rfc_common.dur(pkt[0]) > cap * 960 or n > cap) else 0
    assert p["code"] == want, (pkt[:4].hex(), len(pkt), cap, p, n)
    if want:
        assert p["frames"] == 0 and descs == [] and (p["last_count"], p["last_flags"]) == last, p
    else:
        fl = toc_flags(pkt[0])
        assert p["kind"] == DECODED and p["in_arena"] == 1 and p["frames"] == n and p["flags"] == fl, p
        assert descs == [(3, 1000 + o, ln, fl) for o, ln in frames], (pkt[:4].hex(), descs, frames)
        assert (p["last_count"], p["last_flags"]) == (n, fl), p
    assert bool(ft.ft_is_regular(pkt, len(pkt), 3, 8, cap)) == (want == 0 and pkt[0] & 3 == 0), (pkt[:4].hex(), len(pkt), cap)
    return want


def test_return_code_table(ft, oracle):
    assert len(KAT) == 38
    for name, pkt, fs, ret, count, why in KAT:
        p, _ = plan(ft, pkt, cap=6)  # (room for everything the parser lets through: its verdict alone)
        assert (p["code"] or p["frames"]) == count, (name, p, why)
        check_normal_packet(ft, oracle, pkt, 6)
        if fs > 0 and fs % 960 == 0:
            p, _ = plan(ft, pkt, cap=fs // 960)
            assert p["code"] == (count if count < 0 else TOO_SMALL if ret == TOO_SMALL else 0), (name, p, why)
            check_normal_packet(ft, oracle, pkt, fs // 960)
    for pkt, ln in ((b"\xfc\x01\x02", -1),):  # a negative length (:309), a stream that does not exist
        out, d = (C.c_int32 * 8)(), (Desc * 4)()
        assert ft.ft_plan(pkt, ln, 3, 8, REF, 0, 2, 1, 0, 0, 0, out, d, 4) == 0 and out[0] == BAD_ARG
    for stream in (-1, 8):
        assert plan(ft, b"\xfc\x01\x02", stream=stream)[0]["code"] == BAD_ARG


def test_generated_packets_against_the_oracle_parser(ft, oracle):
    """all 32 TOC configurations x mono / stereo x codes 0 - 3, CBR / VBR, padding, frame_capacity 1, 2, 3, 6: every packet gets a verdict"""
    rng = np.random.default_rng(5)
    shapes = [(1, False, 0), (2, False, 0), (2, True, 0), (5, False, 3), (2, True, 300), (3, False, 0), (3, True, 0), (4, True, 3),
              (6, False, 300), (6, True, 0), (7, False, 0), (48, False, 0)]
    verdicts = {0: 0, TOO_SMALL: 0, INVALID: 0}
    seen = set()
    for cfg in range(32):
        for stereo in (0, 4):
            for frames, vbr, pad in shapes:
                for cap in CAPS:
                    pkt = ms_util.elementary_packet(rng, cfg << 3 | stereo, frames, vbr, pad)
                    verdicts[check_normal_packet(ft, oracle, pkt, cap)] += 1
                    seen.add((cfg, pkt[0] & 3))
    assert sum(verdicts.values()) == 32 * 2 * len(shapes) * len(CAPS) > 3000
    assert seen == {(c, k) for c in range(32) for k in range(4)}
    assert min(verdicts.values()) > 100, verdicts


@pytest.mark.parametrize("channels", [1, 2])
def test_empty_packets_reference_mode(ft, pkg, channels):
    """the descriptors of opusgpu_empty_packet_to_frames: no packet yet, then after a packet of each mode; the memory stays"""
    for cap in CAPS:
        for pkt in (b"", None):
            p, descs = plan(ft, pkt, channels=channels, cap=cap)
            assert (p["code"], p["kind"], p["in_arena"], p["frames"]) == (0, EMPTY, 0, cap)
            assert [d[1:] for d in descs] == pkg.empty_packet_to_frames(-1, channels, cap * 960) and all(d[0] == 3 for d in descs)
            assert descs[0][3] & NO_MODE and (p["last_count"], p["last_flags"]) == (0, 0)
        for toc in (0x0C, 0x08, 0x4B, 0x68, 0x7C, 0x98, 0xFC, 0xE1):  # SILK, hybrid, CELT; mono / stereo; codes 0, 1, 3
            first, _ = plan(ft, ms_util.elementary_packet(np.random.default_rng(toc), toc, 1 + (toc & 3)), cap=6)
            last = (first["last_count"], first["last_flags"])
            assert last == (1 + (toc & 3), toc_flags(toc))
            p, descs = plan(ft, b"", channels=channels, cap=cap, last=last)
            assert (p["code"], p["kind"], p["frames"]) == (0, EMPTY, cap) and (p["last_count"], p["last_flags"]) == last
            assert [d[1:] for d in descs] == pkg.empty_packet_to_frames(last[1], channels, cap * 960)


def test_the_mask_of_the_empty_flags_changes_nothing_within_one_mode():
    """`last_flags & 63` (opusgpu_empty_packet_to_frames, and since the plan every path) against last_flags verbatim: reference-mode
    flags never have a bit above 5 -- every TOC byte"""
    assert all(toc_flags(toc) & ~63 == 0 for toc in range(256))


@pytest.mark.parametrize("channels", [1, 2])
def test_lost_packets_rfc_mode(ft, channels):
    """concealed as long as the stream's last packet was, in its flags; one 20 ms CELT fullband frame when there was none"""
    p, descs = plan(ft, b"", mode=RFC, channels=channels, cap=1)
    fresh = 2 | 4 << 2 | (32 if channels == 2 else 0) | 1 << 9
    assert (p["code"], p["kind"], p["frames"]) == (0, EMPTY, 1) and descs == [(3, 0, 0, fresh)]
    assert ft.ft_lost_flags_no_packet_yet(channels) == fresh
    for toc in range(0, 256, 4):
        for count in (1, 2, 3):
            if count * rfc_common.dur(toc) > 5760:
                continue
            last = (count, toc_flags(toc, rfc=True))
            for cap in CAPS:
                p, descs = plan(ft, None, mode=RFC, channels=channels, cap=cap, last=last)
                assert (p["last_count"], p["last_flags"]) == last
                if count * rfc_common.dur(toc) > cap * 960:
                    assert (p["code"], p["frames"]) == (TOO_SMALL, 0)
                else:
                    assert (p["code"], p["kind"], p["in_arena"]) == (0, EMPTY, 0) and descs == [(3, 0, 0, last[1])] * count


def test_conceal_pieces(ft):
    base = toc_flags(0x7C, rfc=True) | 1 << 10 | 7 << 6  # (a duration field and an FEC bit to be replaced / cleared)
    for last_fs in (120, 240, 480, 960, 1920, 2880):
        for total in range(120, 5760 + 1, 120):
            fl = (C.c_int32 * 48)()
            n = ft.ft_conceal_pieces(total, last_fs, base, fl)
            assert 0 < n <= 48, (total, last_fs, n)
            durs = [DUR_OF_CODE[f >> 6 & 7] for f in fl[:n]]  # (KeyError: not a duration code)
            assert sum(durs) == total and durs == rfc_common.conceal_pieces(total, last_fs), (total, last_fs, durs)
            assert all(f & 1 << 9 and not f & 1 << 10 and f & 63 == base & 63 and f >> 11 == 0 for f in fl[:n])
    assert ft.ft_conceal_pieces(0, 960, base, (C.c_int32 * 48)()) == 0
    assert ft.ft_conceal_pieces(49 * 120, 120, base, (C.c_int32 * 48)()) == -1  # (a 49th piece is refused, not written)


def test_fec_kinds(ft):
    """opus_decode(decode_fec = 1): the FEC frame is used unless the lost duration is shorter than the packet's frame or either
    side is CELT-only; pieces + 1 descriptors or pieces, bit 10 on the last one exactly when it is; the memory stays"""
    rng = np.random.default_rng(9)
    lasts = [None] + [(c, t) for t in range(0, 256, 8) for c in (1, 2, 3, 6) if c * rfc_common.dur(t) <= 5760]
    used = unused = 0
    for last in lasts:
        mem = (last[0], toc_flags(last[1], rfc=True)) if last else (0, 0)
        for toc in range(0, 256, 4):
            pkt = ms_util.elementary_packet(rng, toc, int(rng.integers(1, 3)), bool(rng.integers(2)))
            lost, pieces, use = rfc_common.fec_plan((last[0], rfc_common.dur(last[1]), rfc_common.mode_bw(last[1])[0]) if last else None, toc, 2)
            celt = toc & 0x80 or (last and last[1] & 0x80)
            assert use == (not (lost < rfc_common.dur(toc) or celt))
            for cap in (1, 6):
                p, descs = plan(ft, pkt, mode=RFC, fec=True, cap=cap, last=mem)
                assert (p["last_count"], p["last_flags"]) == mem
                if lost > cap * 960:
                    assert (p["code"], p["frames"]) == (TOO_SMALL, 0)
                    continue
                assert p["code"] == 0 and p["kind"] == (FEC if use else CONCEAL_ONLY) and p["in_arena"] == int(use), (last, hex(toc), p)
                assert p["pieces"] == len(pieces) and p["frames"] == len(pieces) + int(use)
                assert [DUR_OF_CODE[d[3] >> 6 & 7] for d in descs[:len(pieces)]] == pieces
                assert all(d[:3] == (3, 0, 0) and d[3] & 1 << 9 and not d[3] & 1 << 10 for d in descs[:len(pieces)])
                assert all(d[3] & 63 == (mem[1] if last else toc_flags(toc)) & 63 for d in descs[:len(pieces)])
                if use:
                    _, own = plan(ft, pkt, mode=RFC, cap=6)
                    assert descs[-1] == own[0][:3] + (own[0][3] | 1 << 10,)
                    used += 1
                else:
                    unused += 1
    assert used > 1000 and unused > 1000, (used, unused)
    # reference mode has no decode_fec (the call refuses it before it frames), and an empty packet stays a lost packet
    p, _ = plan(ft, b"", mode=RFC, fec=True, cap=1)
    assert (p["kind"], p["frames"]) == (EMPTY, 1)
