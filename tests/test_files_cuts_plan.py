"""Cuts of files as tracks (opusgpu_files_plan_cuts / opusgpu_ms_files_plan_cuts; include/opusgpu.h WHOLE FILES / CUTS): which
packets a cut decodes, what its segments keep, what the arena holds and where strided tracks lie, all against the whole-file plan of
the same files.  No GPU: the "decoder" of the model emits the sample's own position in the file's track."""
import numpy as np
import pytest

import cuts_util as cu
import files_util as fu
import ms_files_util as mfu
from ms_util import LAYOUTS


def _check_cuts(pkg, whole, cut, tables, lengths):
    """Every property of the cut batch `cut` that follows from the whole-file batch `whole` of the same files."""
    recs, ci = cut.cuts, cut.cut_info
    # the rule of the first and the last packet, and the per-cut info
    for t, c in enumerate(recs):
        i = int(c["file"])
        frames, packets = tables[i]
        first, n_p, lead, exact, start, count = cu.expected_cut(packets, lengths[i], int(c["start"]), int(c["count"]), int(c["preroll"]))
        got = tuple(int(ci[t][f]) for f in ("first_packet", "packets", "lead", "exact", "start"))
        assert got == (first, n_p, lead, exact, start), (t, c, got)
        assert exact or lead >= (cu.PREROLL if c["preroll"] < 0 else c["preroll"])
        assert cut.info["track_samples"][t] == count and cut.info["packets"][t] == n_p
        for f in ("status", "channels", "pre_skip", "output_gain", "mapping_family", "holes"):
            assert cut.info[f][t] == whole.info[f][i], (t, f)
        # the cut's own packet table: 0 for the pre-roll, clamped to the cut
        for j in range(n_p + 1):
            at = packets[first + j][1] if first + j < len(packets) else lengths[i]
            assert cut.packet_start(t, j) == min(max(at - start, 0), count), (t, j)
        assert cut.packet_start(t, n_p + 1) == -1
    # descriptors: the whole plan's, for the packets first .. last, in order; packet_seq counted from the first
    mine = {t: [] for t in range(len(recs))}
    for k in range(cut.n_steps):
        descs, files, segs = cut.step(k)[:3]
        descs = np.asarray(descs).reshape(len(files), -1)
        assert len(set(files)) == len(files) and (segs["track"] == files).all() and (descs["stream"] == files[:, None]).all()
        for d, f, sg in zip(descs, files, segs):
            body = tuple(bytes(cut.arena[e["offset"]:e["offset"] + e["len"]]) for e in d)
            mine[int(f)].append((int(sg["packet_seq"]), body, tuple(int(e["flags"]) for e in d), int(sg["src_first"]), int(sg["count"]),
                                 int(sg["dst_first"] - cut.info["track_offset"][f]), tuple(int(e["offset"]) for e in d)))
    for t, c in enumerate(recs):
        i = int(c["file"])
        first, n_p = int(ci[t]["first_packet"]), int(ci[t]["packets"])
        start, count = int(ci[t]["start"]), int(cut.info["track_samples"][t])
        want = [f for f in tables[i][0] if first <= f[0] < first + n_p]
        assert cut.info["frames"][t] == len(want) == len(mine[t]), t
        assert [(f[0] - first, f[1], f[2]) for f in want] == [f[:3] for f in mine[t]], t
        # segments, applied to rows that hold every sample's whole-file position: [start, start + count) once each, in order
        written = np.full(count, -1, dtype=np.int64)
        times = np.zeros(count, dtype=np.int64)
        for w, m in zip(want, mine[t]):
            row = np.full(cut.row_samples, -1, dtype=np.int64)
            row[w[3]:w[3] + w[4]] = w[5] + np.arange(w[4])
            assert 0 <= m[3] and m[3] + m[4] <= cut.row_samples and 0 <= m[5] and m[5] + m[4] <= count, (t, m)
            written[m[5]:m[5] + m[4]] = row[m[3]:m[3] + m[4]]
            times[m[5]:m[5] + m[4]] += 1
        assert (times == 1).all() and np.array_equal(written, start + np.arange(count)), t

    # the model of the device path over the whole batch, its decoder emitting the position (mod 2^16: the tracks are int16)
    def decode_slot(k, slot, d, f):
        w = [x for x in tables[int(recs[f]["file"])][0] if x[0] >= ci[f]["first_packet"]][k]
        row = np.full((cut.row_samples, cut.channels), -1, dtype=np.int16)
        row[w[3]:w[3] + w[4]] = (w[5] + np.arange(w[4])).astype(np.int16)[:, None]
        return row, cut.row_samples
    tracks, got_lengths, status = fu.model_apply(cut, lambda k: cut.step(k)[:3], decode_slot)
    for t in range(len(recs)):
        start, count = int(ci[t]["start"]), int(cut.info["track_samples"][t])
        assert got_lengths[t] == count and status[t, 1] == -1
        assert np.array_equal(tracks[t][:, 0], (start + np.arange(count)).astype(np.int16)), t
    # the arena holds every file's bytes once: all cuts of a file lie at ONE distance from the whole-file arena's offsets, and
    # the arena is as long as the spans between the earliest first and the latest last packet (in front of the first frame of a
    # span lie its packet's header bytes: a TOC, up to 2 length bytes, and in a multistream packet 2 more of the self-delimiting
    # framing, for every elementary stream)
    spans, delta = {}, {}
    for t, c in enumerate(recs):
        i = int(c["file"])
        first, n_p = int(ci[t]["first_packet"]), int(ci[t]["packets"])
        if not n_p:
            continue
        want = [f for f in tables[i][0] if first <= f[0] < first + n_p]
        for w, m in zip(want, mine[t]):
            d = {oc - ow for oc, ow in zip(m[6], w[6])}
            assert len(d) == 1 and delta.setdefault(i, min(d)) == min(d), (t, m[0])
            lo, hi = min(w[6]), max(o + len(body) for o, body in zip(w[6], w[1]))
            a, b = spans.get(i, (lo, hi))
            spans[i] = (min(a, lo), max(b, hi))
    stored = cut.arena.size - 16
    need = sum(b - a for a, b in spans.values())
    assert need <= stored <= need + 5 * cut._width * len(spans), (stored, need)
    assert not cut.arena[-16:].any()


def _plan_both(pkg, files, channels, rfc=False, flags=0, extra=(), stride=None):
    whole = pkg.FileBatch(files, channels=channels, rfc=rfc, flags=flags, threads=2)
    tables = [cu.file_tables(whole, i) for i in range(len(files))]
    lengths = [int(v) for v in whole.info["track_samples"]]
    cuts = [c for i in range(len(files)) for c in cu.cut_list(i, tables[i][1], lengths[i])] + list(extra)
    cut = pkg.FileBatch(files, channels=channels, rfc=rfc, flags=flags, threads=3, cuts=cuts, stride=stride)
    return whole, cut, tables, lengths


@pytest.mark.parametrize("channels", [2, 1])
def test_cuts_of_the_long_corpus(pkg, channels):
    corpus = cu.long_corpus(channels)
    names = [c[0] for c in corpus]
    files = [c[1] for c in corpus]
    w0 = pkg.FileBatch(files, channels=channels)
    tb = {n: cu.file_tables(w0, names.index(n)) for n in ("multi_frame", "hole", "hybrid")}
    w0.close()
    mf, hole = names.index("multi_frame"), names.index("hole")
    three = [p for p in range(len(tb["multi_frame"][1])) if tb["multi_frame"][1][p][0] == 2880][2]
    after_hole = [p for p in range(1, len(tb["hole"][1])) if tb["hole"][1][p][2]][0]  # the packet whose front the 80 ms discard takes
    extra = [(mf, tb["multi_frame"][1][three][1] + 960 + 100, 300),          # inside the second frame of a three-frame packet
             (mf, tb["multi_frame"][1][three][1] + 960 + 100, 300, 0),       # (and without pre-roll: one packet)
             (hole, tb["hole"][1][after_hole][1] - 700, 3000),               # across the hole and its discard
             (hole, tb["hole"][1][after_hole][1], 100, 0),                   # the first sample behind the discard
             (names.index("hybrid"), 0, 2000)]                               # a pre-skip of 4000: longer than the first packet
    whole, cut, tables, lengths = _plan_both(pkg, files, channels, flags=pkg.PAGES_GROUP_BY_MODE, extra=extra)
    assert tb["hole"][1][after_hole][2] == 960 and whole.info["holes"][hole] == 1 and whole.info["pre_skip"][names.index("hybrid")] == 4000
    _check_cuts(pkg, whole, cut, tables, lengths)
    ci = cut.cut_info
    n = len(cut.cuts)
    assert ci["packets"][n - 4] == 1 and ci["first_packet"][n - 4] == three and ci["lead"][n - 4] == 960 + 100
    # start - preroll on a packet boundary: decoding starts at exactly that packet
    for t, c in enumerate(cut.cuts):
        i = int(c["file"])
        q = len(tables[i][1]) // 3
        if c["start"] == tables[i][1][q][1] + cu.PREROLL and c["count"] == 1500 and whole.info["holes"][i] == 0:
            assert (ci["first_packet"][t], ci["lead"][t], ci["exact"][t]) == (q, cu.PREROLL, 0), t
    # a file that changes its mode: cuts that begin behind the change keep theirs, the planner's word per step
    ms = names.index("mode_switches")
    one = pkg.FileBatch(files, channels=channels, cuts=[(ms, 27 * 960, 5 * 960, 0), (ms, 0, 12 * 960)])
    keeps = [bool(one.step(s)[3] & pkg.STEP_KEEPS_MODE) for s in range(one.n_steps)]
    assert one.n_steps == 13 and keeps[:9] == [True] * 9 and not any(keeps[9:])  # nine CELT frames, then the second cut meets hybrid
    one.close()
    whole.close()
    cut.close()


@pytest.mark.parametrize("channels", [2, 1])
def test_cuts_of_the_20ms_corpus_and_refused_files(pkg, channels):
    """Holes, dropped packets, truncated files, plans that end in an error, and the files a plan refuses: every cut has its file's
    status, a refused file's cuts have no frames, and what was planned is cut like any other track."""
    corpus = fu.corpus20(channels) + fu.refusal_files(channels)
    files = [c[1] for c in corpus]
    whole, cut, tables, lengths = _plan_both(pkg, files, channels)
    _check_cuts(pkg, whole, cut, tables, lengths)
    refused = {c[0]: c[2] for c in fu.refusal_files(channels)}
    for t, c in enumerate(cut.cuts):
        name = corpus[int(c["file"])][0]
        if name in refused:
            assert cut.info["status"][t] == refused[name] and cut.info["frames"][t] == 0 and cut.info["track_samples"][t] == 0, name
    assert (whole.info["status"] != 0).sum() > len(refused)  # (files whose plan ends in an error are among them)
    whole.close()
    cut.close()


@pytest.mark.parametrize("channels", [2, 1])
def test_cuts_in_rfc_mode(pkg, channels):
    """Packets of 2.5 to 60 ms and mixed multi-frame packets: the lead counts decoded samples, whatever a packet's duration."""
    corpus = fu.corpus_rfc(channels)
    files = [c[1] for c in corpus]
    w0 = pkg.FileBatch(files, channels=channels, rfc=True)
    extra = []
    for i in range(len(files)):
        _, packets = cu.file_tables(w0, i)
        for p in range(1, len(packets)):
            if packets[p][2] is not None and packets[p][0] in (120, 2880, 5760):  # a 2.5 ms packet, a 60 ms one, two of 60 ms
                extra += [(i, packets[p][1] + 7, 90, pre) for pre in (0, 120, 1000, -1)]
    assert len(extra) >= 12
    w0.close()
    whole, cut, tables, lengths = _plan_both(pkg, files, channels, rfc=True, flags=pkg.PAGES_GROUP_BY_MODE, extra=extra)
    _check_cuts(pkg, whole, cut, tables, lengths)
    whole.close()
    cut.close()


def test_multistream_cuts(pkg):
    layout = LAYOUTS["5.1"]
    rng = np.random.default_rng(5)
    files = [c[0] for c in mfu.corpus(pkg, rng, layout, 4, 30)]
    whole = pkg.MsFileBatch(files, layout, threads=2)
    tables = [cu.file_tables(whole, i) for i in range(len(files))]
    lengths = [int(v) for v in whole.info["track_samples"]]
    cuts = [c for i in range(len(files)) for c in cu.cut_list(i, tables[i][1], lengths[i])]
    cut = pkg.MsFileBatch(files, layout, threads=2, cuts=cuts)
    _check_cuts(pkg, whole, cut, tables, lengths)
    whole.close()
    cut.close()
    with pytest.raises(pkg.OpusGpuError):
        pkg.MsFileBatch(files, layout, cuts=[(4, 0, 10)])


def test_strided_tracks_and_refusals(pkg):
    files = [c[1] for c in cu.long_corpus(2)]
    cuts = [(0, 5000, 4000), (1, 100, 4096), (2, 9000, 1), (0, 0, 0), (3, 960 * 20, 3000, 0)]
    b = pkg.FileBatch(files, channels=2, cuts=cuts, stride=4096)
    assert list(b.info["track_offset"]) == [t * 4096 for t in range(5)] and b.track_samples == 5 * 4096 and b.stride == 4096
    assert list(b.info["track_samples"]) == [4000, 4096, 1, 0, 3000]
    assert load_stride(pkg, b) == 4096
    packed = pkg.FileBatch(files, channels=2, cuts=cuts)
    assert list(packed.info["track_offset"]) == [0, 4032, 8128, 8192, 8192] and load_stride(pkg, packed) == 0
    for k in range(b.n_steps):  # the same plan but for where the tracks lie
        (da, fa, sa, ma), (db, fb, sb, mb) = b.step(k), packed.step(k)
        assert np.array_equal(da, db) and np.array_equal(fa, fb) and ma == mb
        assert np.array_equal(sa["dst_first"] - b.info["track_offset"][fa], sb["dst_first"] - packed.info["track_offset"][fb])
    b.close()
    packed.close()
    for bad in (dict(cuts=cuts, stride=4032), dict(cuts=cuts, stride=100), dict(cuts=[(6, 0, 10)]), dict(cuts=[(-1, 0, 10)])):
        with pytest.raises(pkg.OpusGpuError) as e:
            pkg.FileBatch(files, channels=2, **bad)
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        pkg.FileBatch(files, channels=2, stride=4096)
    with pytest.raises(ValueError):
        pkg.FileBatch(files, channels=2, cuts=[(0, 1)])
    lib = pkg.load_lib()
    import ctypes as C
    h = C.c_void_p()
    assert lib.opusgpu_files_plan_cuts(0, None, None, 1, None, 0, 2, 0, 0, 1, None, None, C.byref(h)) == -1
    assert lib.opusgpu_files_plan_cuts(0, None, None, 0, None, 0, 2, 0, 0, 1, None, None, C.byref(h)) == 0
    assert lib.opusgpu_file_batch_steps(h) == 0 and lib.opusgpu_file_batch_track_samples(h) == 0
    lib.opusgpu_file_batch_free(h)
    assert pkg.cut_seconds(3, 1.5, 10) == (3, 72000, 480000) and pkg.cut_seconds(0, 0.00001, 0.00003) == (0, 0, 1)


def load_stride(pkg, batch):
    return pkg.load_lib().opusgpu_file_batch_track_stride(batch.h)


def test_strided_requests(pkg):
    """files_request for a strided batch: planes the stride apart, everything with a grid of its own refused before any device work."""
    files = [c[1] for c in cu.long_corpus(2)]
    cuts = [(0, 5000, 4000), (1, 100, 4096)]
    b = pkg.FileBatch(files, channels=2, cuts=cuts, stride=4160)
    req = pkg.files_request(b, format="f32_planar")
    assert req.entry == "files_decode_as" and req.stride == 4160 and list(req.planes) == [4160, 4160] and req.total == 2 * 4160
    assert np.array_equal(req.cut_info, b.cut_info)
    for kw in (dict(rate=16000), dict(mono=True), dict(mix="mono"), dict(resample=44100), dict(features="logmel", rate=16000, mono=True),
               dict(features=pkg.kaldi_fbank(num_mel_bins=80), rate=16000, mono=True), dict(loudness="measure", format="f32")):
        with pytest.raises(ValueError, match="stride"):
            pkg.files_request(b, **kw)
    assert pkg.files_request(b, loudness="measure").entry == "files_decode"
    b.close()
    p = pkg.FileBatch(files, channels=2, cuts=cuts)
    assert pkg.files_request(p, rate=16000, mono=True).entry == "files_decode_resampled" and pkg.files_request(p).stride == 0
    p.close()


def test_whole_file_plans_are_what_they_were(pkg):
    """opusgpu_files_plan through its accessors: equal to the cut planner's plan of every file from 0 to its end, which goes through
    the same code with other tables -- and a batch made with cuts=None is that plan."""
    for channels, rfc, flags in ((2, False, 0), (2, False, 4), (1, False, 2), (2, True, 2)):
        corpus = fu.corpus_rfc(channels) if rfc else fu.corpus20(channels) + fu.refusal_files(channels)
        files = [c[1] for c in corpus]
        a = pkg.FileBatch(files, channels=channels, rfc=rfc, flags=flags, threads=2)
        n = pkg.FileBatch(files, channels=channels, rfc=rfc, flags=flags, cuts=None)
        c = pkg.FileBatch(files, channels=channels, rfc=rfc, flags=flags, cuts=[(i, 0, None, 2**31 - 1) for i in range(len(files))])  # (a pre-roll no file has)
        assert (c.cut_info["exact"] == 1).all() and (c.cut_info["first_packet"] == 0).all() and n.cut_info is None
        for other in (n, c):
            assert np.array_equal(a.info, other.info) and a.n_steps == other.n_steps and a.track_samples == other.track_samples
            assert np.array_equal(a.arena, other.arena)
            for k in range(a.n_steps):
                for x, y in zip(a.step(k), other.step(k)):
                    assert np.array_equal(x, y), k
            for i in range(len(files)):
                for p in range(int(a.info["packets"][i]) + 2):
                    assert a.packet_start(i, p) == other.packet_start(i, p)
        for b in (a, n, c):
            b.close()


def test_failed_frames_in_the_model(pkg, oracle):
    """The failure rule as it is, on a cut's own packet table: a failed frame in the pre-roll ends the cut at 0 samples, one inside
    it at its packet's start, one behind it does not concern it."""
    files = fu.failing_files(2)
    names = [f[0] for f in files]
    i, bad = names.index("only_frame"), 3
    w = pkg.FileBatch([f[1] for f in files], channels=2)
    at = w.packet_start(i, bad)
    cuts = [(i, at + 960 + 200, 1000),      # the bad packet in the pre-roll
            (i, 100, at - 100 - 50),        # ends before it
            (i, at - 1000, 2500),           # spans it
            (i, at + 960 + 200, 1000, 0),   # begins behind it, without pre-roll: whole
            (names.index("clean_a"), 500, 3000)]
    b = pkg.FileBatch([f[1] for f in files], channels=2, cuts=cuts)
    assert list(b.cut_info["first_packet"]) == [0, 0, 0, bad + 1, 0]
    tracks, lengths, status, _ = fu.model_decode(pkg, oracle, b)
    whole, _, _, _ = fu.model_decode(pkg, oracle, w)
    assert list(lengths) == [0, at - 150, 1000, 1000, 3000]
    assert [tuple(s) for s in status] == [(-18, bad), (0, -1), (-18, bad), (0, -1), (0, -1)]
    assert np.array_equal(tracks[1], whole[i][100:at - 50]) and np.array_equal(tracks[2], whole[i][at - 1000:at])
    assert np.array_equal(tracks[4], whole[names.index("clean_a")][500:3500])
    w.close()
    b.close()
