"""Test helper for whole multistream files (include/opusgpu.h WHOLE FILES / MULTISTREAM): family-1 Ogg Opus files built in memory
with a family-0 stereo twin of the same page structure, granule positions and packet durations; the independent expectation (all
packets through ms_util.OracleMs, concatenated, pre-skip cut from the front and the end trim from the back); and a numpy model of
"decode the plan's rows, apply its segments"."""
import struct

import numpy as np

import files_util as fu
import ms_util
import ogg_util

# 20 ms TOCs an elementary stream keeps for its whole file: SILK NB, hybrid FB, CELT FB, each mono and stereo (the stereo bit
# disagrees with the decoder's channel count for half of them); TOC - 8 is the same configuration at 10 ms
TOCS = [0x08, 0x0C, 0x78, 0x7C, 0xF8, 0xFC]
PRE_SKIPS = (0, 1, 312, 959, 960, 1000)
END_TRIMS = (0, 1, 700)
# packet shapes (frames, vbr): codes 0, 1, 2 and 3
SHAPES = [(1, False), (2, False), (2, True), (3, True)]


def head(layout, pre_skip=312, family=1):
    ch, S, cp, mp = layout
    return b"OpusHead" + bytes([1, ch]) + struct.pack("<HIhB", pre_skip, 48000, 0, family) + bytes([S, cp]) + bytes(mp)


def stream_tocs(rng, layout, rfc=False):
    """One TOC per elementary stream; the streams of one file differ in mode and stereo bit.  RFC mode: no mono SILK-only TOC on a
    coupled stream -- there the oracle's own output depends on what its output buffer held before the call (a mono SILK-only frame
    in a stereo decoder defines half of the entries it mixes, Q3), so the oracle decoding a two-frame packet whole differs from the
    oracle decoding its frames one by one, and neither is an expectation.  Reference mode has that combination."""
    perm = rng.permutation(len(TOCS))
    tocs = [TOCS[perm[s % len(TOCS)]] for s in range(layout[1])]
    return [0x0C if rfc and s < layout[2] and t == 0x08 else t for s, t in enumerate(tocs)]


def packets(pkg, rng, tocs, shapes, ten_ms=()):
    """-> (elementary packets per multistream packet, the multistream packets); packets whose index is in ten_ms get 10 ms frames."""
    els = [[ms_util.elementary_packet(rng, t - (8 if i in ten_ms else 0), fr, vbr=vbr) for t in tocs] for i, (fr, vbr) in enumerate(shapes)]
    return els, [ms_util.ms_packet(pkg, e) for e in els]


def paged(pk, per_page):
    return [pk[i:i + per_page] for i in range(0, len(pk), per_page)]


def file_and_twin(layout, els, pkts, pre_skip, end_trim, per_page=3, serial=0x51):
    """-> (the family-1 file's pages, the family-0 stereo twin's pages): lists of pages, headers first.  The twin's packets are
    elementary stream 0's: the same first TOC byte and frame count, so the same duration."""
    _, a = fu.opus_file(paged(pkts, per_page), pre_skip=pre_skip, serial=serial, end_trim=end_trim, head=head(layout, pre_skip))
    _, b = fu.opus_file(paged([e[0] for e in els], per_page), 2, pre_skip, serial=serial, end_trim=end_trim)
    return a, b


def lace(n):
    return [255] * (n // 255) + [n % 255]


def spanning_file(head_packet, a, b, big, c, end_trim=0, serial=4):
    """Audio page 1: a, b and the first 255 bytes of big; audio page 2 (continued, EOS): the rest of big, then c."""
    assert len(big) > 255
    f = ogg_util.page(serial, 0, 0, [head_packet], bos=True) + ogg_util.page(serial, 1, 0, [ogg_util.opus_tags()])
    gp = fu.duration(a) + fu.duration(b)
    f += fu.raw_page(serial, 2, gp, lace(len(a)) + lace(len(b)) + [255], a + b + big[:255])
    gp += fu.duration(big) + fu.duration(c) - end_trim
    f += fu.raw_page(serial, 3, gp, lace(len(big) - 255) + lace(len(c)), big[255:] + c, flags=1 | 4)
    return f


def expected_track(orc, i, els, pre_skip, end_trim):
    """Clean file: every packet through decoder i of an OracleMs, back to back, pre_skip dropped in front, end_trim behind."""
    orc.reset(i)
    parts = []
    for e in els:
        cap = max(frame_count(p) for p in e)
        pcm, r = orc.decode(i, e, cap)
        assert r > 0, r
        parts.append(pcm[:r].copy())
    pcm = np.concatenate(parts)
    return pcm[pre_skip:len(pcm) - end_trim]


def frame_count(p):
    """Frame count of a standard packet by its TOC."""
    return 1 if p[0] & 3 == 0 else 2 if p[0] & 3 != 3 else p[1] & 0x3F


def model_decode(pkg, oracle, batch, layout):
    """What opusgpu_ms_files_decode computes, on the oracle: every row's elementary frames decoded one by one (a frame = a code-0
    packet of its descriptor's configuration) by an OracleMs, the step's segments applied with the failure rules of the assembly
    kernels.  -> (tracks [int16 [final length, channels]], final lengths, status [n, 2])."""
    orc = ms_util.OracleMs(oracle, layout, batch.n_files, rfc=batch.rfc)

    def decode_row(k, r, row, f):
        assert (row["stream"] == f).all()
        el = [bytes([fu.frame_toc(int(d["flags"]))]) + bytes(batch.arena[d["offset"]:d["offset"] + d["len"]]) for d in row]
        pcm, res = orc.decode(f, el, 6)
        return (None if pcm is None else pcm.copy()), res

    return fu.model_apply(batch, batch.step, decode_row)


def corpus(pkg, rng, layout, n_files, n_packets, rfc=False, per_page=4):
    """Clean files for the decode tests: [(file bytes, elementary packets per packet, pre_skip, end_trim)].  Reference mode: 20 ms
    frames, codes 0 - 3.  RFC mode: packets of 10, 20 and 40 ms (two 20 ms frames) -- every elementary stream of a packet has the
    packet's frame count and frame duration, as the device step asks."""
    out = []
    for i in range(n_files):
        tocs = stream_tocs(rng, layout, rfc)
        shapes = [SHAPES[(i + j) % 4] if not rfc else [(1, False), (1, False), (2, bool(j & 4))][(i + j) % 3] for j in range(n_packets)]
        ten = {j for j in range(n_packets) if rfc and (i + j) % 3 == 0}
        els, pk = packets(pkg, rng, tocs, shapes, ten)
        ps, trim = PRE_SKIPS[i % len(PRE_SKIPS)], END_TRIMS[(i // 2) % len(END_TRIMS)]
        data, _ = fu.opus_file(paged(pk, per_page), pre_skip=ps, serial=100 + i, end_trim=trim, head=head(layout, ps))
        out.append((data, els, ps, trim))
    return out
