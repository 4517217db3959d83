"""Multistream framing and layout checks on the host (include/opusgpu.h, MULTISTREAM; no GPU needed): opusgpu_ms_packet_to_frames
against the oracle's parser in self-delimited mode, the known answers of opus_multistream_packet_validate / _decode_native's
refusals (src/opus_decoder.cpp:803-823, :851-857), the layout checks (:742-770, :688-697), and k_ms_map's register budget."""
import ctypes as C
import re

import numpy as np
import pytest

import ms_util

INVALID, BAD_ARG = -4, -1


def _oracle_validate(oracle, data, S):
    """opus_multistream_packet_validate restated on the oracle's parser: -> (samples or code, [[(offset, len)] per stream])."""
    lib = oracle.lib
    lib.oc_packet_parse.argtypes = [C.c_char_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if len(data) == 0 or len(data) < 2 * S - 1:
        return INVALID, None
    at, samples, frames = 0, 0, []
    for s in range(S):
        rest = data[at:]
        if len(rest) <= 0:
            return INVALID, None
        size = (C.c_int16 * 48)()
        toc, off, po = C.c_uint8(), C.c_int(), C.c_int32()
        n = lib.oc_packet_parse(rest, len(rest), 1 if s != S - 1 else 0, C.byref(toc), size, C.byref(off), C.byref(po))
        if n < 0:
            return n, None
        t = rest[0]
        code = t & 3
        count = 1 if code == 0 else 2 if code != 3 else (rest[1] & 0x3F)
        spf = (48000 << ((t >> 3) & 3)) // 400 if t & 0x80 else ((960 if t & 8 else 480) if (t & 0x60) == 0x60 else
                                                                  (2880 if ((t >> 3) & 3) == 3 else (48000 << ((t >> 3) & 3)) // 100))
        tmp = count * spf
        if tmp * 25 > 48000 * 3:
            return INVALID, None
        if s and tmp != samples:
            return INVALID, None
        samples = tmp
        o = at + off.value
        fr = []
        for k in range(n):
            fr.append((o, size[k]))
            o += size[k]
        frames.append(fr)
        at += po.value
    return samples, frames


def _random_elementary(rng, dur_toc):
    frames = int(rng.choice([1, 1, 2, 2, 3, 4]))
    vbr = bool(rng.random() < 0.5)
    pad = int(rng.choice([0, 0, 3, 300])) if frames > 2 or rng.random() < 0.3 else 0
    big = rng.random() < 0.2  # sizes >= 252: two-byte lengths
    sizes = [int(rng.integers(252, 400)) if big else int(rng.integers(0, 60)) for _ in range(frames)]
    if not vbr:
        sizes = [sizes[0]] * frames
    return ms_util.elementary_packet(rng, dur_toc, frames, vbr, pad, sizes)


def test_ms_packet_to_frames_matches_oracle_parser(pkg, oracle):
    rng = np.random.default_rng(11)
    checked = refused = 0
    for it in range(1500):
        S = int(rng.integers(1, 9))
        coupled = int(rng.integers(0, S + 1))
        lay = pkg.ms_layout(S + coupled, S, coupled)
        toc = int(rng.choice([0x00, 0x08, 0x60, 0x68, 0x80, 0x90, 0x98, 0xF0]))  # 10 / 20 ms SILK, hybrid, CELT
        el = [_random_elementary(rng, toc | (int(rng.integers(0, 2)) << 2)) for _ in range(S)]
        if rng.random() < 0.15:  # one stream of another duration
            el[int(rng.integers(0, S))] = bytes([0x80 | 0x10 | 0]) + bytes(5)
        pk = bytearray(ms_util.ms_packet(pkg, el))
        if rng.random() < 0.25 and len(pk) > 2:  # damage: cut, or flip a byte
            if rng.random() < 0.5:
                pk = pk[:int(rng.integers(1, len(pk)))]
            else:
                pk[int(rng.integers(0, len(pk)))] = int(rng.integers(0, 256))
        pk = bytes(pk)
        want, frames = _oracle_validate(oracle, pk, S)
        for rfc in (False, True):
            got = pkg.ms_packet_to_frames(lay, pk, decoder=5, rfc=rfc)
            if want < 0:
                assert got == want, (it, rfc, got, want)
                refused += 1
                continue
            if not rfc and len({len(f) for f in frames}) > 1:  # the documented reference-mode refusal
                assert got == INVALID
                continue
            dur, descs = got
            assert dur == want
            assert [[(o, ln) for o, ln, _ in d] for d in descs] == frames, it
            checked += 1
    assert checked > 300 and refused > 300


def test_ms_refusals_known_answers(pkg):
    lay2 = pkg.ms_layout(2, 2, 0)
    celt20 = bytes([0x98]) + bytes(10)
    sd20 = ms_util.self_delimit(pkg, celt20)
    # len == 0, len < 2 * streams - 1 (:855)
    assert pkg.ms_packet_to_frames(lay2, b"") == INVALID
    assert pkg.ms_packet_to_frames(pkg.ms_layout(3, 3, 0), bytes([0x98, 0, 0x98, 0])) == INVALID
    # a missing stream: the first stream uses every byte (:810)
    assert pkg.ms_packet_to_frames(lay2, sd20) == INVALID
    # streams of different durations (:817)
    assert pkg.ms_packet_to_frames(lay2, sd20 + bytes([0x90]) + bytes(4)) == INVALID
    # a stream longer than 120 ms: code 3, 7 frames of 20 ms (opus_packet_parse_impl refuses it first)
    assert pkg.ms_packet_to_frames(pkg.ms_layout(1, 1, 0), bytes([0x9B, 7]) + bytes(7)) == INVALID
    # a self-delimited size past the end (:645-647)
    assert pkg.ms_packet_to_frames(lay2, bytes([0x98, 200]) + bytes(5) + celt20) == INVALID
    # code 1 with an odd payload in the last (standard) stream
    assert pkg.ms_packet_to_frames(lay2, sd20 + bytes([0x91, 1, 2, 3])) == INVALID
    # good packets: the duration, every frame
    dur, d = pkg.ms_packet_to_frames(lay2, sd20 + celt20)
    assert dur == 960 and d == [[(2, 10, 2)], [(13, 10, 2)]]
    # the reference-mode edge case: equal durations, different frame counts (2 x 10 ms | 1 x 20 ms)
    two10 = bytes([0x91]) + bytes(8)  # CELT NB 10 ms, code 1
    pk = ms_util.self_delimit(pkg, two10) + celt20
    assert pkg.ms_packet_to_frames(lay2, pk) == INVALID
    dur, d = pkg.ms_packet_to_frames(lay2, pk, rfc=True)
    assert dur == 960 and [len(x) for x in d] == [2, 1]
    assert d[0][0][2] & (1 << 9) and (d[0][0][2] >> 6) & 7 == 3  # RFC bit, 10 ms
    # negative length, bad layout
    lib = pkg.load_lib()
    fd = (pkg.FrameDesc * 96)()
    cnt = np.zeros(2, np.int32)
    assert lib.opusgpu_ms_packet_to_frames(C.byref(lay2), celt20, -1, 0, 0, fd, cnt.ctypes.data) == BAD_ARG
    assert lib.opusgpu_ms_packet_to_frames(C.byref(lay2), celt20, len(celt20), 0, 2, fd, cnt.ctypes.data) == BAD_ARG


@pytest.mark.parametrize("channels,streams,coupled,mapping,ok", [
    (6, 4, 2, [0, 4, 1, 2, 3, 5], True),
    (1, 1, 0, [0], True),
    (2, 1, 0, [0, 255], True),
    (3, 1, 1, [1, 0, 0], True),
    (255, 128, 127, [c % 255 for c in range(255)], True),  # streams + coupled = 255
    (0, 1, 0, [], False),            # channels < 1
    (256, 1, 0, [0] * 256, False),   # channels > 255
    (2, 0, 0, [255, 255], False),    # streams < 1
    (2, 1, 2, [0, 1], False),        # coupled > streams
    (2, 2, -1, [0, 1], False),       # coupled < 0
    (2, 128, 128, [0, 1], False),    # streams > 255 - coupled
    (2, 2, 1, [0, 3], False),        # mapping >= streams + coupled
    (2, 2, 1, [254, 0], False),
])
def test_ms_layout_checks(pkg, channels, streams, coupled, mapping, ok):
    lib = pkg.load_lib()
    lay = pkg.MsLayout()
    lay.channels, lay.streams, lay.coupled = channels, streams, coupled
    for c in range(256):
        lay.mapping[c] = mapping[c] if c < len(mapping) else 255
    S = max(streams, 1)
    pk = b"".join(ms_util.self_delimit(pkg, bytes([0x98, 0])) for _ in range(S - 1)) + bytes([0x98, 0])
    fd = (pkg.FrameDesc * (48 * S))()
    cnt = np.zeros(S, np.int32)
    r = lib.opusgpu_ms_packet_to_frames(C.byref(lay), pk, len(pk), 0, 0, fd, cnt.ctypes.data)
    assert (r == 960) if ok else (r == BAD_ARG), r
    if not ok:  # refused before any device is looked at
        h = C.c_void_p()
        assert lib.opusgpu_ms_create(0, C.byref(lay), 4, C.byref(h)) == BAD_ARG and not h


def test_ms_map_kernel_budget():
    """k_ms_map is data movement: no scratch, few registers, every instance (channel counts 1..8 and the general one)."""
    from test_kernel_budget import _kernel_metadata
    meta = _kernel_metadata()
    inst = {k: v for k, v in meta.items() if re.search(r"\d+k_ms_map", k)}
    assert len(inst) == 9, sorted(inst)
    for k, (vgpr, scratch, lds) in inst.items():
        assert scratch == 0 and vgpr <= 48 and lds <= 64, (k, vgpr, scratch, lds)
    for k in ("k_ms_split", "k_ms_gather"):
        hit = [v for m, v in meta.items() if re.search(r"\d+" + k + r"(P|E|v|x|$)", m)]
        assert hit and hit[0][1] == 0, (k, hit)
