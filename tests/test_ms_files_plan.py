"""The multistream file planner (opusgpu_file_layout / opusgpu_ms_files_plan, include/opusgpu.h WHOLE FILES / MULTISTREAM).  No
GPU involved.  The container bookkeeping is pinned against the existing stereo planner on a family-0 twin of every file (the same
pages, granule positions and packet durations): the reader looks at nothing else, so the segments must be the same.  The rows are
pinned against opusgpu_ms_packet_to_frames, the tracks against an OracleMs that decodes every packet whole."""
import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
import ms_util
import ogg_util
from ms_util import LAYOUTS

UNIMPLEMENTED, BAD_ARG, EBADPACKET = -5, -1, -136
L51 = LAYOUTS["5.1"]


def _same_plan(ms, tw):
    """An MsFileBatch and the FileBatch of its twins: the same bookkeeping, field by field."""
    for name in ("status", "packets", "frames", "holes", "track_samples", "track_offset", "pre_skip"):
        assert np.array_equal(ms.info[name], tw.info[name]), (name, ms.info[name], tw.info[name])
    assert ms.n_steps == tw.n_steps and ms.track_samples == tw.track_samples
    for k in range(ms.n_steps):
        _, fa, sa = ms.step(k)
        _, fb, sb, _ = tw.step(k)
        assert np.array_equal(fa, fb), k
        assert (sa["slot"] == np.arange(len(sa))).all() and (sa["track"] == fa).all() and (sa["reserved"] == 0).all()
        for name in ("slot", "src_first", "count", "track", "packet_seq"):
            assert np.array_equal(sa[name], sb[name]), (k, name)
        assert np.array_equal(sa["dst_first"] - ms.info["track_offset"][sa["track"]], sb["dst_first"] - tw.info["track_offset"][sb["track"]]), k
    for i in range(ms.n_files):
        for seq in range(int(ms.info["packets"][i]) + 2):
            assert ms.packet_start(i, seq) == tw.packet_start(i, seq), (i, seq)
        assert ms.info["track_offset"][i] % 64 == 0


@pytest.mark.parametrize("name", [n for n in LAYOUTS if LAYOUTS[n][0] <= 8])
def test_bookkeeping_equals_the_stereo_twin(pkg, name):
    layout = LAYOUTS[name]
    rng = np.random.default_rng(sum(name.encode()))
    files, twins = [], []
    for i, (ps, trim) in enumerate((p, t) for p in mf.PRE_SKIPS for t in mf.END_TRIMS):
        shapes = [mf.SHAPES[(i + j) % 4] for j in range(6)]  # codes 0 - 3
        els, pk = mf.packets(pkg, rng, mf.stream_tocs(rng, layout), shapes)
        a, b = mf.file_and_twin(layout, els, pk, ps, trim, per_page=2 + i % 2, serial=60 + i)
        files.append(b"".join(a))
        twins.append(b"".join(b))
    ms = pkg.MsFileBatch(files, layout, threads=2)
    tw = pkg.FileBatch(twins, channels=2)
    assert (ms.info["status"] == 0).all() and (ms.info["mapping_family"] == 1).all() and (ms.info["channels"] == layout[0]).all()
    assert (ms.info["track_samples"] > 0).all()
    _same_plan(ms, tw)
    ms.close()
    tw.close()


def test_bookkeeping_of_damaged_files_equals_the_twin(pkg):
    """A dropped page (a hole and the 80 ms discard behind it), a packet that spans two pages, a page with a damaged checksum."""
    rng = np.random.default_rng(77)
    files, twins = [], []
    tocs = mf.stream_tocs(rng, L51)
    els, pk = mf.packets(pkg, rng, tocs, [mf.SHAPES[j % 4] for j in range(18)])
    a, b = mf.file_and_twin(L51, els, pk, 312, 300, per_page=3, serial=12)
    for drop in ((4,), (6,), (3, 6)):  # mid-file, before the EOS page, both
        files.append(b"".join(p for i, p in enumerate(a) if i not in drop))
        twins.append(b"".join(p for i, p in enumerate(b) if i not in drop))
    for at in (3, 5):  # a flipped byte in the page's body: the checksum fails, the reader resyncs
        for pages, out in ((a, files), (b, twins)):
            bad = bytearray(pages[at])
            bad[-1] ^= 0x40
            out.append(b"".join(pages[:at] + [bytes(bad)] + pages[at + 1:]))
    for trim in (0, 500):
        e4 = [[ms_util.elementary_packet(rng, t, 1, sizes=[n]) for t in tocs] for n in (100, 120, 400, 90)]
        p4 = [ms_util.ms_packet(pkg, e) for e in e4]
        files.append(mf.spanning_file(mf.head(L51, 312), *p4, end_trim=trim))
        twins.append(mf.spanning_file(ogg_util.opus_head(channels=2, pre_skip=312), *[e[0] for e in e4], end_trim=trim))
    ms = pkg.MsFileBatch(files, L51)
    tw = pkg.FileBatch(twins, channels=2)
    print("holes", ms.info["holes"], "packets", ms.info["packets"], "samples", ms.info["track_samples"], "status", ms.info["status"])
    assert list(ms.info["holes"][:3]) == [1, 1, 2] and (ms.info["holes"][3:5] == 1).all() and (ms.info["holes"][5:] == 0).all()
    assert list(ms.info["packets"][5:]) == [4, 4] and list(ms.info["track_samples"][5:]) == [4 * 960 - 312, 4 * 960 - 312 - 500]
    _same_plan(ms, tw)
    ms.close()
    tw.close()


@pytest.mark.parametrize("rfc", [False, True])
def test_step_rows_are_the_packets_frames(pkg, rfc):
    """Row r of step k = frame k of the file's packets as opusgpu_ms_packet_to_frames splits them, offsets rebased into the arena."""
    layout = LAYOUTS["7.1"]
    lay = pkg.ms_layout(*layout)
    rng = np.random.default_rng(3)
    corpus = mf.corpus(pkg, rng, layout, 5, 7, rfc=rfc)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, rfc=rfc)
    assert (b.info["status"] == 0).all()
    assert b.arena.size >= 16 and not b.arena[-16:].any()
    want = {}
    for i, (_, els, _, _) in enumerate(corpus):
        k = 0
        for e in els:
            p = ms_util.ms_packet(pkg, e)
            dur, fr = pkg.ms_packet_to_frames(lay, p, decoder=i, rfc=rfc)
            for j in range(len(fr[0])):
                want[(i, k)] = [(p, o, ln, fl) for o, ln, fl in (s[j] for s in fr)]
                k += 1
        assert b.info["frames"][i] == k and b.info["packets"][i] == len(els)
    seen = set()
    for k in range(b.n_steps):
        descs, files, segs = b.step(k)
        assert descs.shape == (len(files), layout[1]) and list(files) == sorted(set(files))
        for row, f, sg in zip(descs, files, segs):
            exp = want[(int(f), k)]
            p = exp[0][0]
            base = int(row[0]["offset"]) - exp[0][1]
            assert bytes(b.arena[base:base + len(p)]) == p  # the whole packet lies there
            for d, (_, o, ln, fl) in zip(row, exp):
                assert (d["stream"], d["offset"], d["len"], d["flags"]) == (f, base + o, ln, fl)
            assert 0 <= sg["src_first"] and sg["src_first"] + sg["count"] <= b.row_samples
            seen.add((int(f), k))
    assert seen == set(want)
    b.close()


def _plan_one(pkg, data, layout=L51, rfc=False, neighbours=True):
    """Plans [good, data, good] and returns data's info record; the neighbours must be planned whatever data is."""
    rng = np.random.default_rng(9)
    good = mf.corpus(pkg, rng, layout, 2, 4, rfc=rfc)
    b = pkg.MsFileBatch([good[0][0], data, good[1][0]], layout, rfc=rfc)
    info = b.info[1].copy()
    assert list(b.info["status"][[0, 2]]) == [0, 0] and (b.info["track_samples"][[0, 2]] > 0).all()
    if info["frames"] == 0:
        assert all((b.step(k)[1] != 1).all() for k in range(b.n_steps))
    b.close()
    return info


def _file51(pkg, seed=5, layout=L51, **kw):
    rng = np.random.default_rng(seed)
    return mf.corpus(pkg, rng, layout, 1, 4, **kw)[0][0]


def test_refusal_channel_count(pkg):
    info = _plan_one(pkg, _file51(pkg, layout=(5, 4, 2, [0, 4, 1, 2, 3])))
    assert (info["status"], info["frames"], info["track_samples"], info["channels"]) == (BAD_ARG, 0, 0, 5)


def test_refusal_coupled_count(pkg):
    info = _plan_one(pkg, _file51(pkg, layout=(6, 4, 1, [0, 1, 2, 3, 4, 4])), layout=(6, 4, 2, [0, 1, 2, 3, 4, 4]))
    assert (info["status"], info["frames"], info["track_samples"]) == (BAD_ARG, 0, 0)


def test_refusal_one_mapping_entry(pkg):
    info = _plan_one(pkg, _file51(pkg, layout=(6, 4, 2, [0, 4, 1, 2, 3, 255])))
    assert (info["status"], info["frames"], info["track_samples"]) == (BAD_ARG, 0, 0)


def test_refusal_stream_count_and_family_0(pkg):
    info = _plan_one(pkg, _file51(pkg, layout=(6, 5, 1, [0, 4, 1, 2, 3, 5])))
    assert (info["status"], info["frames"]) == (BAD_ARG, 0)
    stereo = fu.corpus20(2)[1][1]  # a family-0 stereo file is the layout (2, 1, 1, [0, 1]), not 5.1
    assert _plan_one(pkg, stereo)["status"] == BAD_ARG
    b = pkg.MsFileBatch([stereo], LAYOUTS["stereo"])
    t = pkg.FileBatch([stereo], channels=2)
    _same_plan(b, t)
    b.close()
    t.close()


def test_refusal_family_255(pkg):
    rng = np.random.default_rng(2)
    els, pk = mf.packets(pkg, rng, mf.stream_tocs(rng, L51), [(1, False)] * 3)
    data = fu.opus_file([pk], head=mf.head(L51, 312, family=255))[0]
    info = _plan_one(pkg, data)
    assert (info["status"], info["frames"], info["track_samples"]) == (UNIMPLEMENTED, 0, 0)
    with pytest.raises(pkg.OpusGpuError) as e:
        pkg.file_layout(data)
    assert e.value.code == UNIMPLEMENTED


def test_refusal_reference_mode_ten_ms_packet(pkg):
    rng = np.random.default_rng(4)
    els, pk = mf.packets(pkg, rng, mf.stream_tocs(rng, L51), [(1, False)] * 3, ten_ms={1})
    data = fu.opus_file([pk], head=mf.head(L51, 312))[0]
    info = _plan_one(pkg, data)
    assert (info["status"], info["packets"], info["frames"], info["track_samples"]) == (UNIMPLEMENTED, 0, 0, 0)
    info = _plan_one(pkg, data, rfc=True)  # RFC mode's business: accepted there
    assert (info["status"], info["packets"], info["frames"], info["track_samples"]) == (0, 3, 3, 960 + 480 + 960 - 312)


def test_refusal_rfc_mode_rows_of_two_durations(pkg):
    """Elementary stream 0 carries 2 x 10 ms, the others 1 x 20 ms: a valid packet, but no row of one duration."""
    rng = np.random.default_rng(6)
    tocs = mf.stream_tocs(rng, L51)
    ok = [[ms_util.elementary_packet(rng, t, 1) for t in tocs] for _ in range(2)]
    odd = [ms_util.elementary_packet(rng, tocs[0] - 8, 2)] + [ms_util.elementary_packet(rng, t, 1) for t in tocs[1:]]
    pk = [ms_util.ms_packet(pkg, e) for e in (ok[0], odd, ok[1])]
    assert pkg.ms_packet_to_frames(pkg.ms_layout(*L51), pk[1], rfc=True)[0] == 960
    data = fu.opus_file([pk], head=mf.head(L51, 312))[0]
    info = _plan_one(pkg, data, rfc=True)
    assert (info["status"], info["packets"], info["frames"], info["track_samples"]) == (UNIMPLEMENTED, 0, 0, 0)
    # reference mode: the framing itself rejects unequal frame counts, which ends the plan at that packet
    info = _plan_one(pkg, data)
    assert (info["status"], info["packets"], info["frames"], info["track_samples"]) == (EBADPACKET, 1, 1, 960 - 312)


def test_packet_too_short_for_its_streams_ends_the_plan(pkg):
    rng = np.random.default_rng(8)
    els, pk = mf.packets(pkg, rng, mf.stream_tocs(rng, L51), [(1, False), (2, False), (1, False), (1, False)])
    pk[2] = bytes([0xFC, 0x11])  # a valid 20 ms TOC, but 2 bytes cannot hold 4 elementary packets (2 * streams - 1 = 7 at least)
    data = fu.opus_file([pk[:2], pk[2:]], head=mf.head(L51, 312))[0]
    b = pkg.MsFileBatch([data], L51)
    info = b.info[0]
    assert (info["status"], info["packets"], info["frames"], info["track_samples"]) == (EBADPACKET, 2, 3, 3 * 960 - 312)
    assert b.n_steps == 3 and b.packet_start(0, 2) == 3 * 960 - 312 and b.packet_start(0, 3) == -1
    b.close()


def test_file_layout(pkg):
    for ch in (1, 2):
        data = fu.corpus20(ch)[1][1]
        lay, info = pkg.file_layout(data)
        assert lay == (ch, 1, ch - 1, list(range(ch))) and (info["status"], info["channels"], info["mapping_family"]) == (0, ch, 0)
    for name, layout in LAYOUTS.items():
        data = _file51(pkg, layout=layout)
        lay, info = pkg.file_layout(data)
        assert lay == tuple(layout), name
        assert (info["status"], info["channels"], info["mapping_family"], info["pre_skip"]) == (0, layout[0], 1, 0)
    # a head cut short: what the stereo planner says of the same bytes
    data = _file51(pkg)
    for cut in (0, 20, 40):
        t = pkg.FileBatch([data[:cut]], channels=2)
        with pytest.raises(pkg.OpusGpuError) as e:
            pkg.file_layout(data[:cut])
        assert e.value.code == t.info["status"][0] < 0, cut
        t.close()


def test_bad_arguments_and_empty_batch(pkg):
    b = pkg.MsFileBatch([], L51)
    assert b.n_steps == 0 and b.track_samples == 0
    with pytest.raises(IndexError):
        b.step(0)
    b.close()
    for bad in ((6, 4, 5, [0] * 6), (0, 1, 0, []), (2, 1, 0, [0, 1])):  # coupled > streams, no channel, a mapping entry out of range
        with pytest.raises(pkg.OpusGpuError) as e:
            pkg.MsFileBatch([b"x"], bad)
        assert e.value.code == BAD_ARG
    b = pkg.MsFileBatch([b"not an ogg file at all", b""], L51)
    assert list(b.info["status"]) == [-132, -132] and b.n_steps == 0  # OP_ENOTFORMAT
    b.close()


@pytest.mark.parametrize("name,rfc", [("5.1", False), ("duplicated", False), ("muted", True)])
def test_track_model_equals_whole_packet_decoding(pkg, oracle, name, rfc):
    """Rows decoded one by one and placed by the segments == every packet decoded whole, concatenated, cut at both ends."""
    layout = LAYOUTS[name]
    rng = np.random.default_rng(31)
    corpus = mf.corpus(pkg, rng, layout, 6, 6, rfc=rfc)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, rfc=rfc)
    tracks, lengths, status = mf.model_decode(pkg, oracle, b, layout)
    orc = ms_util.OracleMs(oracle, layout, len(corpus), rfc=rfc)
    for i, (_, els, ps, trim) in enumerate(corpus):
        want = mf.expected_track(orc, i, els, ps, trim)
        assert tuple(status[i]) == (0, -1) and lengths[i] == b.info["track_samples"][i] == len(want), i
        assert np.array_equal(tracks[i], want), i
    b.close()
