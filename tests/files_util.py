"""Test helper for the whole-file path (include/opusgpu.h WHOLE FILES): Ogg Opus files built in memory (on top of ogg_util), the
single-file double's output as the expectation, and a numpy model of the decode steps + track assembly that runs on the oracle."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import ogg_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CT_LIB = os.path.join(ROOT, "tests", "emul", "libog_container_test.so")
OP_HOLE = -3
INT32_MAX = 2**31 - 1

# stereo / mono TOCs of 20 ms frames: SILK NB, hybrid FB, CELT FB
TOCS20 = {2: (0x0C, 0x7C, 0xFC), 1: (0x08, 0x78, 0xF8)}


def load_ct():
    subprocess.check_call(["make", "-C", os.path.dirname(CT_LIB), "-s"])
    lib = C.CDLL(CT_LIB)
    lib.ct_open.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
    lib.ct_read_stereo.argtypes = [C.c_void_p, C.c_int]
    lib.ct_channels.restype = C.c_int
    return lib


def drain(ct, data, eof_code=0):
    """The single-file reader (with the oracle as decoder) over one file, reading on after OP_HOLE: -> (open code, int16
    [samples, 2] (mono duplicated, as op_read_stereo does), samples per read call, the code that ended the loop)."""
    r = ct.ct_open(bytes(data), len(data), eof_code)
    if r != 0:
        return r, np.zeros((0, 2), np.int16), [], r
    buf = np.zeros(5760 * 2, dtype=np.int16)
    chunks, holes = [], 0
    while True:
        r = ct.ct_read_stereo(buf.ctypes.data, 5760 * 2)
        if r == OP_HOLE:
            holes += 1
            continue
        if r <= 0:
            break
        chunks.append(buf[:2 * r].copy().reshape(-1, 2))
    pcm = np.concatenate(chunks) if chunks else np.zeros((0, 2), np.int16)
    return 0, pcm, [len(c) for c in chunks], r


def as_stereo(track):
    """A planned track [samples, channels] the way op_read_stereo hands it out."""
    return track if track.shape[1] == 2 else np.repeat(track, 2, axis=1)


# ---- files ---------------------------------------------------------------------------------------------
def raw_page(serial, seqno, granule, lacing, body, flags=0):
    hdr = bytearray(b"OggS\x00" + bytes([flags]) + struct.pack("<qIII", granule, serial, seqno, 0) + bytes([len(lacing)]) + bytes(lacing))
    hdr[22:26] = struct.pack("<I", ogg_util.ogg_crc(bytes(hdr) + bytes(body)))
    return bytes(hdr) + bytes(body)


def head_family1(channels=2, pre_skip=312):
    """OpusHead of channel mapping family 1 (one coupled stream for stereo)."""
    return (b"OpusHead" + bytes([1, channels]) + struct.pack("<HIhB", pre_skip, 48000, 0, 1) +
            bytes([1, channels - 1]) + bytes(range(channels)))


def duration(p):
    """Samples at 48 kHz of a packet by its TOC (0 for an invalid TOC sequence)."""
    if len(p) < 1:
        return 0
    t = p[0]
    if t & 0x80:
        spf = (48000 << ((t >> 3) & 3)) // 400
    elif (t & 0x60) == 0x60:
        spf = 960 if t & 8 else 480
    else:
        a = (t >> 3) & 3
        spf = 2880 if a == 3 else (48000 << a) // 100
    n = 1 if t & 3 == 0 else 2 if t & 3 != 3 else (p[1] & 0x3F if len(p) > 1 else 0)
    return n * spf if 0 < n * spf <= 5760 else 0


def packet(rng, toc, n, code=0, frames=3):
    """A packet of TOC `toc` (its code bits are replaced): code 0 one frame of n bytes; 1 two frames of n bytes; 2 frames of n and
    n + 7 bytes; 3 `frames` frames of n bytes each (CBR)."""
    body = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    toc &= 0xFC
    if code == 0:
        return bytes([toc]) + body(n)
    if code == 1:
        return bytes([toc | 1]) + body(2 * n)
    if code == 2:
        assert n < 252
        return bytes([toc | 2, n]) + body(n) + body(n + 7)
    return bytes([toc | 3, frames]) + body(frames * n)


def opus_file(pages, channels=2, pre_skip=312, serial=0x51, end_trim=0, head=None, tags=None, eos=True):
    """pages: list of lists of packets.  Granule positions count the packets' durations; the last page's is `end_trim` less and
    carries EOS.  -> (bytes, the audio pages alone as a list: headers are pages 0 and 1)."""
    out = [ogg_util.page(serial, 0, 0, [head or ogg_util.opus_head(channels=channels, pre_skip=pre_skip)], bos=True),
           ogg_util.page(serial, 1, 0, [tags or ogg_util.opus_tags()])]
    gp = 0
    for i, pk in enumerate(pages):
        gp += sum(duration(p) for p in pk)
        last = i == len(pages) - 1
        out.append(ogg_util.page(serial, 2 + i, gp - (end_trim if last else 0), pk, eos=last and eos))
    return b"".join(out), out


def corpus20(channels, seed=5, channel_switches=True):
    """The 20 ms corpus: [(name, file bytes, packets or None)] -- packets: the audio packets in order where the file is clean (every
    one of them reaches the decoder), None where holes / dropped packets / damage make that the reader's business.
    channel_switches=False leaves out the one file whose packets also switch between mono and stereo TOCs: the planner handles it
    like any other (tests/test_files_plan.py), but the device decode itself -- opusgpu_decode_step_device, before and without this
    path -- differs from the oracle on it: a mono SILK-only frame right behind a stereo CELT-only frame of a stereo stream comes
    out different from sample 480 on ("found on the way").  That is the decoder's to fix, not this path's."""
    rng = np.random.default_rng(seed + channels)
    silk, hyb, celt = TOCS20[channels]
    P = lambda toc, n=60, **kw: packet(rng, toc, n, **kw)
    out = []

    def add(name, data, packets=None):
        out.append((name, data, packets))

    if channels == 2:
        import random
        random.seed(7)
        kat = [[bytes([0xFC]) + bytes(random.getrandbits(8) for _ in range(160)) for _ in range(10)] for _ in range(10)]
        add("kat3", ogg_util.kat3_file(), [p for pg in kat for p in pg])
    # the end-trim file of test_container.py: mono, junk between pages
    r1 = np.random.default_rng(1)
    pk = [bytes([0xF8]) + r1.integers(0, 256, 60, dtype=np.uint8).tobytes() for _ in range(6)]
    f = ogg_util.page(77, 0, 0, [ogg_util.opus_head(channels=1, pre_skip=100)], bos=True) + ogg_util.page(77, 1, 0, [ogg_util.opus_tags()])
    f += ogg_util.page(77, 2, 2880, pk[:3]) + b"OggS-not-a-page" + bytes(40) + ogg_util.page(77, 3, 2880 + 2000, pk[3:], eos=True)
    if channels == 1:
        add("end_trim_mono_junk", f, pk)
    for ps in (0, 312, 3840, 4000):  # 4000: more than the first page's 2880 samples
        pages = [[P(celt) for _ in range(3)] for _ in range(3)]
        add(f"pre_skip_{ps}", opus_file(pages, channels, ps, end_trim=77 * (ps % 7))[0], [p for pg in pages for p in pg])
    # OpusTags over three pages
    tags = ogg_util.opus_tags(vendor=bytes(580))
    pages = [[P(hyb, 80) for _ in range(4)], [P(hyb, 90) for _ in range(2)]]
    _, pg = opus_file(pages, channels, 312, serial=9)
    t = [raw_page(9, 1, -1, [255], tags[:255]), raw_page(9, 2, -1, [255], tags[255:510], flags=1),
         raw_page(9, 3, 0, [len(tags) - 510], tags[510:], flags=1)]
    aud = [ogg_util.page(9, 4, 3840, pages[0]), ogg_util.page(9, 5, 5760, pages[1], eos=True)]
    add("tags_three_pages", pg[0] + b"".join(t) + b"".join(aud), [p for x in pages for p in x])
    # an audio packet spanning two pages
    a, b, big, c = P(celt, 100), P(celt, 120), P(celt, 400), P(celt, 90)
    f = ogg_util.page(4, 0, 0, [ogg_util.opus_head(channels=channels, pre_skip=312)], bos=True) + ogg_util.page(4, 1, 0, [ogg_util.opus_tags()])
    f += raw_page(4, 2, 1920, [101, 121, 255], a + b + big[:255])
    f += raw_page(4, 3, 3840, [len(big) - 255, 91], big[255:] + c, flags=1 | 4)
    add("packet_spans_pages", f, [a, b, big, c])
    # code 1 / 2 / 3 packets of 20 ms frames, all three modes
    pages = [[P(celt, 70, code=1), P(celt, 50, code=2), P(celt, 40, code=3, frames=3)],
             [P(silk, 30, code=1), P(silk, 25, code=2), P(hyb, 60, code=3, frames=2), P(hyb, 64, code=1)]]
    add("multi_frame_packets", opus_file(pages, channels, 500, end_trim=1000)[0], [p for pg in pages for p in pg])
    # a dropped page in mid-file and before the EOS page
    pages = [[P(celt) for _ in range(4)] for _ in range(6)]
    _, pg = opus_file(pages, channels, 312, serial=12, end_trim=300)
    add("hole_mid_file", b"".join(pg[:4] + pg[5:]))
    add("hole_before_eos", b"".join(pg[:6] + pg[7:]))
    add("two_holes", b"".join(pg[:3] + pg[4:6] + pg[7:]))
    # invalid-TOC packets (code 3 with no frames, an empty packet) between valid ones
    bad = bytes([celt | 3, 0])
    pages = [[P(celt), bad, P(celt), b"", P(celt)], [bad, P(silk, 30), P(silk, 30)], [P(celt), bad]]
    add("invalid_toc_between", opus_file(pages, channels, 312)[0])
    # an EOS granule position before the previous page's
    pages = [[P(celt) for _ in range(3)] for _ in range(3)]
    _, pg = opus_file(pages, channels, 100, serial=13)
    pg[-1] = ogg_util.page(13, 4, 5760 - 500, pages[2], eos=True)
    add("eos_granule_backwards", b"".join(pg))
    # truncated files
    whole, pg = opus_file([[P(celt) for _ in range(5)] for _ in range(4)], channels, 312, serial=14)
    for name, cut in (("empty", 0), ("in_head", 30), ("after_head", len(pg[0])), ("after_tags", len(pg[0]) + len(pg[1])),
                      ("in_first_audio_page", len(pg[0]) + len(pg[1]) + 200), ("in_third_audio_page", len(whole) - len(pg[-1]) - 100),
                      ("no_eos_page", len(whole) - len(pg[-1]))):
        add("truncated_" + name, whole[:cut])
    # every mode, and mode switches
    for name, toc, n in (("silk", silk, 35), ("hybrid", hyb, 90), ("celt", celt, 120)):
        pages = [[P(toc, n) for _ in range(5)] for _ in range(3)]
        add("mode_" + name, opus_file(pages, channels, 312, end_trim=123)[0], [p for pg in pages for p in pg])
    seq = [celt, celt, hyb, silk, silk, hyb, celt, silk, celt, hyb, hyb, silk, celt, celt, silk]
    other = TOCS20[3 - channels]  # (a mono file may hold stereo packets and the other way round: the decoder mixes, Q3)
    seq2 = [other[2], celt, other[0], silk, hyb, other[1], celt]
    for name, s in (("mode_switches", seq), ("mode_and_channel_switches", seq2))[:2 if channel_switches else 1]:
        pages = [[P(t, 70) for t in s[i:i + 4]] for i in range(0, len(s), 4)]
        add(name, opus_file(pages, channels, 312)[0], [p for pg in pages for p in pg])
    return out


def refusal_files(channels):
    """[(name, file, expected status)]: the only files of the suite a reference-mode plan refuses."""
    rng = np.random.default_rng(17)
    celt = TOCS20[channels][2]
    pages = [[packet(rng, celt, 60) for _ in range(3)] for _ in range(2)]
    ten_ms = [[packet(rng, celt, 60), packet(rng, (celt & ~0x18) | 0x10, 40), packet(rng, celt, 60)]]  # CELT FB 10 ms in the middle
    return [("channel_mismatch", opus_file(pages, 3 - channels)[0], -1),
            ("family_1", opus_file(pages, channels, head=head_family1(channels))[0], -5),
            ("ten_ms_toc", opus_file(ten_ms, channels)[0], -5)]


def corpus_rfc(channels, seed=23):
    """RFC mode: every frame duration and mixed multi-frame packets; clean files, so the expectation is plain Ogg Opus arithmetic.
    [(name, file, packets, pre_skip, end_trim)]"""
    rng = np.random.default_rng(seed + channels)
    st = 4 if channels == 2 else 0
    celt = lambda d: 0x80 | (3 << 5) | (d << 3) | st  # FB: 2.5 / 5 / 10 / 20 ms
    silk = lambda a: (1 << 5) | (a << 3) | st         # MB: 10 / 20 / 40 / 60 ms
    hyb = lambda d: 0x70 | (d << 3) | st              # FB: 10 / 20 ms
    P = lambda toc, n=50, **kw: packet(rng, toc, n, **kw)
    out = []
    for name, pages, ps, trim in (
            ("celt_short", [[P(celt(0), 20), P(celt(1), 30), P(celt(2), 40), P(celt(3), 60)] * 2, [P(celt(0), 20, code=3, frames=4), P(celt(2), 35, code=1)]], 312, 50),
            ("silk_long", [[P(silk(0), 20), P(silk(1), 30), P(silk(2), 60), P(silk(3), 90)], [P(silk(2), 50, code=1), P(silk(3), 80, code=3, frames=2)]], 1000, 700),
            ("hybrid_10_20", [[P(hyb(0), 50), P(hyb(1), 80), P(hyb(0), 45, code=2)], [P(hyb(1), 70, code=3, frames=3)]], 0, 0),
            ("mixed", [[P(celt(3), 60), P(silk(2), 60), P(hyb(0), 50), P(celt(1), 30, code=3, frames=5)], [P(silk(0), 25, code=2), P(celt(2), 40), P(hyb(1), 75)]], 5000, 333)):
        out.append((name, opus_file(pages, channels, ps, end_trim=trim)[0], [p for pg in pages for p in pg], ps, trim))
    return out


def rfc_expected(oracle, channels, packets, pre_skip, end_trim):
    """Clean file: the packets' PCM back to back, the first pre_skip samples dropped, the last end_trim too."""
    d = oracle.decoder(channels)
    d.init()
    d.set_rfc(True)
    parts = []
    for p in packets:
        buf, r = d.decode(p)
        assert r == duration(p), (p[:2].hex(), r)
        parts.append(buf[:r].copy())
    pcm = np.concatenate(parts)
    return pcm[pre_skip:len(pcm) - end_trim]


# ---- the device path's model -------------------------------------------------------------------------------
def frame_toc(flags):
    """A code-0 TOC byte that frames to these descriptor flags (mode, bandwidth, stereo; RFC mode: the duration)."""
    mode, bw, stereo, dur = flags & 3, (flags >> 2) & 7, (flags >> 5) & 1, (flags >> 6) & 7
    if mode == 2:
        toc = 0x80 | ({0: 0, 2: 1, 3: 2, 4: 3}[bw] << 5) | ({1: 0, 2: 1, 3: 2, 0: 3}[dur] << 3)
    elif mode == 1:
        toc = 0x60 | (0x10 if bw == 4 else 0) | ({3: 0, 0: 1}[dur] << 3)
    else:
        toc = (bw << 5) | ({3: 0, 0: 1, 4: 2, 5: 3}[dur] << 3)
    return toc | (4 if stereo else 0)


def model_apply(batch, step_tables, decode_slot):
    """The part of the model both kinds of batch share: per step, every slot decoded -- decode_slot(k, slot, descriptors of the
    slot, its file) -> (PCM rows or None, result) -- and the step's segments applied with the failure rules of the assembly
    kernels; then the fold into lengths and status.  step_tables(k) -> (descriptors per slot, file per slot, segments).
    -> (tracks [int16 [final length, channels]], final lengths, status [n, 2])."""
    ch, n = batch.channels, batch.n_files
    packed = np.zeros((max(int(batch.track_samples), 1), ch), dtype=np.int16)
    first_bad = np.full(n, INT32_MAX, dtype=np.int64)
    code = np.zeros(n, dtype=np.int32)
    for k in range(batch.n_steps):
        descs, files, segs = step_tables(k)
        rows, res = {}, {}
        for slot, (d, f) in enumerate(zip(descs, files)):
            rows[slot], res[slot] = decode_slot(k, slot, d, int(f))
        for sg in segs:
            t, slot = int(sg["track"]), int(sg["slot"])
            if res[slot] < 0:
                if sg["packet_seq"] < first_bad[t]:
                    first_bad[t], code[t] = sg["packet_seq"], res[slot]
                continue
            if sg["packet_seq"] >= first_bad[t] or sg["count"] <= 0:
                continue
            assert sg["src_first"] + sg["count"] <= res[slot], (t, k, sg, res[slot])
            packed[sg["dst_first"]:sg["dst_first"] + sg["count"]] = rows[slot][sg["src_first"]:sg["src_first"] + sg["count"]]
    lengths = np.array([batch.packet_start(i, int(first_bad[i])) if first_bad[i] != INT32_MAX else batch.info["track_samples"][i]
                        for i in range(n)], dtype=np.int64)
    status = np.array([[code[i], first_bad[i]] if first_bad[i] != INT32_MAX else [batch.info["status"][i], -1] for i in range(n)],
                      dtype=np.int64).reshape(n, 2)
    return [packed[o:o + ln] for o, ln in zip(batch.info["track_offset"], lengths)], lengths, status


def model_decode(pkg, oracle, batch):
    """What opusgpu_files_decode computes, on the oracle: every step's frames decoded one by one (a frame = a code-0 packet of
    its descriptor's configuration, which is what the device decodes), the step's segments applied with the failure rules of
    k_tracks_assemble.  -> (tracks [int16 [final length, channels]], final lengths, status [n, 2], planned frames seen)."""
    dec = {}
    frames = []

    def decode_slot(k, slot, d, f):
        assert d["stream"] == f
        if f not in dec:
            dec[f] = oracle.decoder(batch.channels)
            dec[f].init()
            dec[f].set_rfc(batch.rfc)
        toc = frame_toc(int(d["flags"]))
        assert pkg.packet_to_frames(bytes([toc, 0, 0]))[0][2] == (int(d["flags"]) & 63), hex(toc)
        body = bytes(batch.arena[d["offset"]:d["offset"] + d["len"]])
        frames.append((f, k, body, int(d["flags"])))
        buf, r = dec[f].decode(bytes([toc]) + body)
        return buf[:max(r, 0)].copy(), r

    return model_apply(batch, lambda k: batch.step(k)[:3], decode_slot) + (frames,)


# ---- large batches (numpy all the way: the pure-Python page builder is too slow for them) ----------------------------------
def _crc_fill(pkg, rows):
    rows[:, 22:26] = 0
    rows[:, 22:26] = pkg.ogg_crc_rows(rows).astype("<u4").reshape(-1, 1).view(np.uint8)


def bulk_files(pkg, n, toc, L, pages=3, per_page=10, seed=3, channels=2):
    """n files of `pages` audio pages x `per_page` code-0 packets of TOC `toc` and L payload bytes (LCG payloads), random
    pre-skips (0..2000) and end trims (0..2000).  -> (uint8 [n, file_len], pre_skips, end_trims)"""
    rng = np.random.default_rng(seed)
    pre = rng.integers(0, 2001, n)
    trim = rng.integers(0, 2001, n)
    serial = np.arange(n, dtype=np.uint32) + 1000
    pay = pkg.lcg_payloads(n, pages * per_page, L, seed_base=seed * 7919 + 1)
    head = np.frombuffer(ogg_util.page(0, 0, 0, [ogg_util.opus_head(channels=channels, pre_skip=0)], bos=True), dtype=np.uint8)
    tags = np.frombuffer(ogg_util.page(0, 1, 0, [ogg_util.opus_tags()]), dtype=np.uint8)
    H = np.tile(head, (n, 1))
    T = np.tile(tags, (n, 1))
    for rows in (H, T):
        rows[:, 14:18] = serial.astype("<u4").reshape(n, 1).view(np.uint8)
    H[:, 28 + 10:28 + 12] = pre.astype("<u2").reshape(n, 1).view(np.uint8)  # 27 + 1 lacing value, then OpusHead: pre-skip at 10
    _crc_fill(pkg, H)
    _crc_fill(pkg, T)
    parts = [H, T]
    for p in range(pages):
        pg = pkg.build_pages(toc, pay[p * per_page:(p + 1) * per_page], serial, seqno=2 + p)
        gp = np.full(n, (p + 1) * per_page * 960, dtype=np.int64)
        if p == pages - 1:
            gp -= trim
            pg[:, 5] = 4
        pg[:, 6:14] = gp.astype("<i8").reshape(n, 1).view(np.uint8)
        _crc_fill(pkg, pg)
        parts.append(pg)
    return np.concatenate(parts, axis=1), pre, trim


def failing_files(channels, seed=31):
    """Files with a CELT-only / hybrid frame of at most one byte, which the decoder refuses (-18), among clean ones:
    [(name, file, index of the packet that holds the failing frame, or None)]"""
    rng = np.random.default_rng(seed + channels)
    _, hyb, celt = TOCS20[channels]
    body = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    ok = lambda toc=celt: packet(rng, toc, 80)
    only = bytes([celt, 0x55])                                  # the packet's only frame: one byte
    second = bytes([celt | 2, 60]) + body(60) + b"\x33"         # code 2: a frame of 60 bytes, then one of 1 byte
    first = bytes([hyb])                                        # hybrid, a frame of no bytes, as the file's first packet
    spec = [("clean_a", [[ok() for _ in range(4)], [ok() for _ in range(3)]], None),
            ("only_frame", [[ok(), ok(), ok(), only, ok()], [ok(), ok()]], 3),
            ("second_frame", [[ok(), ok(), second, ok()], [ok()]], 2),
            ("first_packet", [[first, ok(hyb), ok(hyb)], [ok(hyb)]], 0),
            ("clean_b", [[ok(hyb) for _ in range(5)]], None)]
    return [(name, opus_file(pages, channels, 312, serial=40 + i, end_trim=100)[0], bad) for i, (name, pages, bad) in enumerate(spec)]
