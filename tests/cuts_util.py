"""Test helper for cuts of files (include/opusgpu.h WHOLE FILES / CUTS): longer files than files_util's, the list of cuts the tests
take from every file, and an independent restatement of which packets a cut decodes, read off the whole-file plan's own tables."""
import numpy as np

import files_util as fu

# samples of a frame by the duration code of its descriptor flags (bits 6 - 8; 0 in reference mode: 20 ms)
FRAME_SAMPLES = {0: 960, 1: 120, 2: 240, 3: 480, 4: 1920, 5: 2880}
PREROLL = 3840


def long_corpus(channels, seed=41):
    """Files of 30 - 60 packets of 20 ms frames: [(name, file bytes)].  Every mode, a file that changes its mode, multi-frame packets
    (a three-frame code-3 packet among them), a pre-skip longer than the first packet, end trims, a dropped page (a hole with its
    80 ms discard)."""
    rng = np.random.default_rng(seed + channels)
    silk, hyb, celt = fu.TOCS20[channels]
    P = lambda toc, n=60, **kw: fu.packet(rng, toc, n, **kw)
    out = []
    for name, toc, n, ps, trim, count in (("celt", celt, 100, 312, 123, 40), ("silk", silk, 35, 0, 0, 32), ("hybrid", hyb, 90, 4000, 700, 36)):
        pages = [[P(toc, n) for _ in range(4)] for _ in range(count // 4)]
        out.append((name, fu.opus_file(pages, channels, ps, end_trim=trim)[0]))
    seq = [celt] * 9 + [hyb] * 7 + [silk] * 10 + [celt] * 8
    out.append(("mode_switches", fu.opus_file([[P(t, 70) for t in seq[i:i + 5]] for i in range(0, len(seq), 5)], channels, 312)[0]))
    pk = [P(celt, 40, code=3, frames=3) if j % 5 == 2 else P(celt, 50, code=j % 3) for j in range(30)]
    out.append(("multi_frame", fu.opus_file([pk[i:i + 3] for i in range(0, 30, 3)], channels, 500, end_trim=1000)[0]))
    # 8,640 samples a page; behind the dropped page the 80 ms discard takes two packets and a frame of the third
    pages = [[P(celt), P(celt, code=1), P(celt, 40, code=3, frames=3), P(celt), P(celt, code=1)] for _ in range(9)]
    _, pg = fu.opus_file(pages, channels, 312, serial=12, end_trim=300)
    out.append(("hole", b"".join(pg[:6] + pg[7:])))
    return out


def file_tables(batch, i):
    """What the whole-file plan `batch` says of file i -> (frames, packets): frames in step order, each (packet_seq, frame bytes,
    flags, src_first, count, position in the track, arena offsets); packets: per packet_seq (decoded samples, planned start, decoded samples in front
    of its first kept one or None where it keeps nothing)."""
    frames = []
    for k in range(int(batch.info["frames"][i])):
        descs, files, segs = batch.step(k)[:3]
        j = int(np.nonzero(files == i)[0][0])
        d, sg = np.asarray(descs).reshape(len(files), -1)[j], segs[j]
        body = tuple(bytes(batch.arena[e["offset"]:e["offset"] + e["len"]]) for e in d)
        frames.append((int(sg["packet_seq"]), body, tuple(int(e["flags"]) for e in d), int(sg["src_first"]), int(sg["count"]),
                       int(sg["dst_first"] - batch.info["track_offset"][i]), tuple(int(e["offset"]) for e in d)))
    packets = []
    for p in range(int(batch.info["packets"][i])):
        mine = [f for f in frames if f[0] == p]
        spf = FRAME_SAMPLES[(mine[0][2][0] >> 6) & 7]
        kept = [j * spf + f[3] for j, f in enumerate(mine) if f[4] > 0]
        packets.append((len(mine) * spf, batch.packet_start(i, p), kept[0] if kept else None))
    return frames, packets


def expected_cut(packets, length, start, count, preroll):
    """The rule of include/opusgpu.h (WHICH PACKETS), by trying every packet -> (first_packet, packets, lead, exact, start, count)."""
    start = min(max(start, 0), length)
    count = length - start if count is None or count < 0 else min(count, length - start)
    if count == 0:
        return 0, 0, 0, 1, start, 0
    preroll = PREROLL if preroll < 0 else preroll
    ends = [packets[p + 1][1] if p + 1 < len(packets) else length for p in range(len(packets))]
    pa = [p for p in range(len(packets)) if packets[p][1] <= start < ends[p]][0]
    pb = [p for p in range(len(packets)) if packets[p][1] <= start + count - 1 < ends[p]][0]
    lead = lambda p: sum(q[0] for q in packets[p:pa]) + packets[pa][2] + start - packets[pa][1]
    ok = [p for p in range(pa + 1) if lead(p) >= preroll]
    first = ok[-1] if ok else 0
    return first, pb - first + 1, lead(first), int(first == 0), start, count


def cut_list(i, packets, length):
    """The cuts the tests take from file i of `packets` (file_tables) and `length` samples: [(file, start, count[, preroll])]."""
    n = len(packets)
    if n < 12:
        return [(i, 0, None), (i, 100, 500)]
    mid = packets[n // 2][1]
    clean = packets[n // 3][1]  # (a packet boundary: the packets from here to the middle are whole in these files)
    cuts = [(i, 0, None),                      # the whole track
            (i, 100, 500),                     # a start inside the first packet (exact: less than the pre-roll in front of it)
            (i, mid, 2000),                    # a start on a packet boundary
            (i, mid + 500, 2000),              # overlapping the cut before
            (i, clean + PREROLL, 1500),        # start - preroll on a packet boundary
            (i, 1000, 3000),                   # start < preroll
            (i, mid + 123, 1500, 0),           # no pre-roll
            (i, mid + 123, 1500, 960 * 8),     # 160 ms of it
            (i, length - 700, 5000),           # across the end of the track
            (i, 5000, 0),                      # nothing
            (i, length + 1000, 100),           # past the end
            (i, 7777, -1)]                     # to the end
    return cuts
