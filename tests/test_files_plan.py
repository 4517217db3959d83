"""The file planner (opusgpu_files_plan, include/opusgpu.h WHOLE FILES): whole Ogg Opus files -> decode steps + track segments.
No GPU involved.  The expectation is the single-file reader itself (tests/emul/libog_container_test.so: og_container.hpp with the
oracle as decoder), drained by a loop that reads on after OP_HOLE; the planner's segments are applied to oracle-decoded frames in
numpy (files_util.model_decode) and must give the same samples."""
import numpy as np
import pytest

import files_util as fu
from oracle_py import fnv1a_u16


@pytest.fixture(scope="module")
def ct():
    return fu.load_ct()


def _check_against_reader(pkg, oracle, ct, corpus, channels, **kw):
    names = [c[0] for c in corpus]
    b = pkg.FileBatch([c[1] for c in corpus], channels=channels, **kw)
    tracks, lengths, status, _ = fu.model_decode(pkg, oracle, b)
    for i, name in enumerate(names):
        code, want, _, final = fu.drain(ct, corpus[i][1])
        info = b.info[i]
        print(name, "status", info["status"], "packets", info["packets"], "frames", info["frames"], "holes", info["holes"], "samples",
              lengths[i], "reader", code, len(want), final)
        if code != 0:  # the reader does not open the file: no plan, its code
            assert info["status"] == code and info["frames"] == 0 and lengths[i] == 0, name
            continue
        assert info["status"] in (0, final), name  # the code that ends the reader's loop (0: end of stream)
        assert lengths[i] == info["track_samples"] == len(want), name
        assert status[i, 1] == -1, name
        assert np.array_equal(fu.as_stereo(tracks[i]), want), name
        assert info["track_offset"] % 64 == 0
    return b, tracks, lengths


@pytest.mark.parametrize("channels", [2, 1])
def test_plan_reproduces_the_single_file_reader(pkg, oracle, ct, channels):
    corpus = fu.corpus20(channels)
    b, tracks, lengths = _check_against_reader(pkg, oracle, ct, corpus, channels)
    names = [c[0] for c in corpus]
    # the cap: no file of the 20 ms corpus is refused, and every kind is there
    assert not set(b.info["status"]) & {-1, -5}
    for must in ("pre_skip_0", "pre_skip_4000", "tags_three_pages", "packet_spans_pages", "multi_frame_packets", "hole_mid_file",
                 "hole_before_eos", "invalid_toc_between", "eos_granule_backwards", "truncated_in_third_audio_page", "mode_switches"):
        assert must in names
    assert b.info["holes"][names.index("hole_mid_file")] == 1 and b.info["holes"][names.index("two_holes")] == 2
    assert (lengths > 0).sum() >= len(corpus) - 5
    if channels == 2:  # survey KAT 3, the reference-origin pin
        i = names.index("kat3")
        assert lengths[i] == 95688 and fnv1a_u16(tracks[i]) == 0xA6FEB1E8
        assert (b.info[i]["pre_skip"], b.info[i]["channels"], b.info[i]["packets"], b.info[i]["frames"]) == (312, 2, 100, 100)
    else:
        i = names.index("end_trim_mono_junk")
        assert lengths[i] == 2880 + 2000 - 100
    b.close()


@pytest.mark.parametrize("flags", [0, 2, 4])
def test_step_tables(pkg, oracle, flags):
    """A stream at most once per step, frame k of a file in step k with the bytes and flags of the packet split, the grouping
    flags as in the page batch, the 16-byte arena tail, segments inside their rows and tracks."""
    corpus = [c for c in fu.corpus20(2) if c[2] is not None]
    b = pkg.FileBatch([c[1] for c in corpus], channels=2, flags=flags, threads=3)
    want = {}
    for i, (_, _, packets) in enumerate(corpus):
        k = 0
        for seq, p in enumerate(packets):
            for off, ln, fl in pkg.packet_to_frames(p, i):
                want[(i, k)] = (p[off:off + ln], fl, seq)
                k += 1
        assert b.info["frames"][i] == k and b.info["packets"][i] == len(packets)
    seen = {}
    assert b.n_steps == max(b.info["frames"])
    assert b.arena.size >= 16 and not b.arena[-16:].any()
    for s in range(b.n_steps):
        descs, files, segs, modes = b.step(s)
        assert len(set(descs["stream"])) == len(descs) and (descs["stream"] == files).all()
        assert (segs["slot"] == np.arange(len(segs))).all() and (segs["track"] == files).all()
        mode = (descs["flags"] & 3).astype(int)
        assert (modes & 7) == sum(1 << m for m in set(mode))
        if flags:
            assert (np.diff(mode) >= 0).all()
            for m in range(3):
                if flags == 2:
                    assert list(files[mode == m]) == sorted(files[mode == m])
        else:
            assert list(files) == sorted(files)
        for d, f, sg in zip(descs, files, segs):
            seen[(int(f), s)] = (bytes(b.arena[d["offset"]:d["offset"] + d["len"]]), int(d["flags"]), int(sg["packet_seq"]))
            assert 0 <= sg["src_first"] and sg["src_first"] + sg["count"] <= 960 and sg["count"] >= 0
            rel = sg["dst_first"] - b.info["track_offset"][f]
            assert 0 <= rel and rel + sg["count"] <= b.info["track_samples"][f]
            assert rel >= b.packet_start(int(f), int(sg["packet_seq"]))
    assert seen == want
    # a file keeps its mode or it does not: the planner's word per step
    names = [c[0] for c in corpus]
    one = pkg.FileBatch([corpus[names.index("mode_switches")][1]], channels=2)
    keeps = [bool(one.step(s)[3] & pkg.STEP_KEEPS_MODE) for s in range(one.n_steps)]
    assert keeps[:2] == [True, True] and not any(keeps[2:])  # CELT, CELT, then hybrid: from there on the file has changed its mode
    one.close()
    b.close()


def test_refusals_leave_the_neighbours_alone(pkg, oracle, ct):
    good = [c for c in fu.corpus20(2) if c[0] in ("pre_skip_312", "multi_frame_packets", "hole_mid_file", "mode_celt")]
    bad = fu.refusal_files(2)
    mixed = [good[0], bad[0], good[1], bad[1], bad[2], good[2], good[3]]
    a = pkg.FileBatch([c[1] for c in good], channels=2)
    m = pkg.FileBatch([c[1] for c in mixed], channels=2)
    at = {0: 0, 2: 1, 5: 2, 6: 3}
    for i, c in enumerate(mixed):
        if i in at:
            assert m.info["status"][i] == a.info["status"][at[i]] and m.info["track_samples"][i] == a.info["track_samples"][at[i]]
        else:
            assert m.info["status"][i] == c[2], c[0]
            assert m.info["frames"][i] == 0 and m.info["track_samples"][i] == 0
    assert m.info["channels"][1] == 1 and m.info["mapping_family"][3] == 1
    assert m.n_steps == a.n_steps
    for s in range(a.n_steps):
        da, fa, sa, ma = a.step(s)
        dm, fm, sm, mm = m.step(s)
        assert ma == mm and len(da) == len(dm)
        assert [at[int(f)] for f in fm] == list(fa)
        for x, y, p, q in zip(da, dm, sa, sm):
            assert bytes(a.arena[x["offset"]:x["offset"] + x["len"]]) == bytes(m.arena[y["offset"]:y["offset"] + y["len"]])
            assert x["flags"] == y["flags"] and (p["src_first"], p["count"], p["packet_seq"]) == (q["src_first"], q["count"], q["packet_seq"])
            assert p["dst_first"] - a.info["track_offset"][p["track"]] == q["dst_first"] - m.info["track_offset"][q["track"]]
    a.close()
    m.close()
    # the ten-millisecond file is RFC mode's business: accepted there
    r = pkg.FileBatch([bad[2][1]], channels=2, rfc=True)
    assert r.info["status"][0] == 0 and r.info["track_samples"][0] == 960 + 480 + 960 - 312
    r.close()
    # a mono context refuses the stereo files the same way
    mono = pkg.FileBatch([good[0][1], fu.corpus20(1)[1][1]], channels=1)
    assert list(mono.info["status"]) == [-1, 0]
    mono.close()


@pytest.mark.parametrize("channels", [2, 1])
def test_rfc_mode(pkg, oracle, ct, channels):
    corpus = fu.corpus_rfc(channels)
    b = pkg.FileBatch([c[1] for c in corpus], channels=channels, rfc=True, flags=2)
    tracks, lengths, status, _ = fu.model_decode(pkg, oracle, b)
    for i, (name, data, packets, pre, trim) in enumerate(corpus):
        want = fu.rfc_expected(oracle, channels, packets, pre, trim)
        _, reader, chunks, final = fu.drain(ct, data)  # (the reference-mode double: its sample COUNTS are the same bookkeeping)
        print(name, "samples", lengths[i], "expected", len(want), "reader", len(reader))
        assert b.info["status"][i] == 0 and status[i, 1] == -1
        assert lengths[i] == len(want) == len(reader), name
        assert np.array_equal(tracks[i], want), name
        for s in range(b.n_steps):
            descs, files, segs, _ = b.step(s)
            for d, sg in zip(descs[files == i], segs[files == i]):
                assert d["flags"] & (1 << 9)
                assert sg["src_first"] + sg["count"] <= pkg.RFC_FRAME
    # the 20 ms corpus gives the same tracks' LENGTHS in RFC mode (the bookkeeping does not depend on the mode)
    c20 = fu.corpus20(channels)
    r = pkg.FileBatch([c[1] for c in c20], channels=channels, rfc=True)
    p = pkg.FileBatch([c[1] for c in c20], channels=channels)
    assert np.array_equal(r.info["track_samples"], p.info["track_samples"])
    r.close()
    p.close()
    b.close()


def test_failed_frames_end_the_track_in_the_model(pkg, oracle, ct):
    """The failure rules (a frame of <= 1 byte in CELT-only / hybrid mode: -18) against the reader, which returns OP_EBADPACKET at
    that packet: as the only frame of a packet, as the second frame of a two-frame packet, in the first packet."""
    files = fu.failing_files(2)
    b = pkg.FileBatch([f[1] for f in files], channels=2)
    tracks, lengths, status, _ = fu.model_decode(pkg, oracle, b)
    for i, (name, data, bad_seq) in enumerate(files):
        _, want, _, final = fu.drain(ct, data)
        print(name, "final length", lengths[i], "planned", b.info["track_samples"][i], "reader", len(want), final)
        if bad_seq is None:
            assert final == 0 and status[i, 1] == -1 and lengths[i] == b.info["track_samples"][i]
        else:
            assert final == -136 and tuple(status[i]) == (-18, bad_seq)
            assert lengths[i] == b.packet_start(i, bad_seq) < b.info["track_samples"][i]
        assert lengths[i] == len(want) and np.array_equal(tracks[i], want), name
    b.close()


def test_empty_batch_and_bad_arguments(pkg):
    b = pkg.FileBatch([], channels=2)
    assert b.n_steps == 0 and b.track_samples == 0
    with pytest.raises(IndexError):
        b.step(0)
    b.close()
    with pytest.raises(pkg.OpusGpuError):
        pkg.FileBatch([b"x"], channels=3)
    b = pkg.FileBatch([b"not an ogg file at all", b""], channels=2)
    assert list(b.info["status"]) == [-132, -132] and b.n_steps == 0  # OP_ENOTFORMAT
    b.close()
