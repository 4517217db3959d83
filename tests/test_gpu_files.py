"""Whole Ogg Opus files on the GPU (opusgpu_files_decode / Context.decode_files, k_tracks_assemble; include/opusgpu.h WHOLE
FILES): N files in, N trimmed tracks out, against the single-file reader running on the oracle (tests/files_util.py)."""
import numpy as np
import pytest

import files_util as fu

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ct():
    return fu.load_ct()


@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("channels", [2, 1])
def test_corpus_reference_mode_equals_the_single_file_reader(pkg, ctx, ct, channels, pipeline):
    corpus = fu.corpus20(channels, channel_switches=False) + fu.refusal_files(channels)
    ctx.streams_alloc(len(corpus), channels)
    ctx.set_pipeline(pipeline)
    tracks, info = ctx.decode_files([c[1] for c in corpus], threads=2)
    refused = {c[0]: c[2] for c in fu.refusal_files(channels)}
    for i, c in enumerate(corpus):
        if c[0] in refused:
            assert info["final_status"][i] == refused[c[0]] and len(tracks[i]) == 0, c[0]
            continue
        code, want, _, final = fu.drain(ct, c[1])
        print(c[0], "status", info["final_status"][i], "samples", len(tracks[i]), "reader", code, len(want), final)
        if code != 0:
            assert info["final_status"][i] == code and len(tracks[i]) == 0, c[0]
            continue
        assert info["final_status"][i] in (0, final) and info["bad_packet"][i] == -1, c[0]
        assert info["track_samples"][i] == len(tracks[i]) == len(want), c[0]
        assert np.array_equal(fu.as_stereo(tracks[i]), want), c[0]


@pytest.mark.parametrize("channels", [2, 1])
def test_corpus_rfc_mode(pkg, ctx, oracle, channels):
    corpus = fu.corpus_rfc(channels)
    c20 = [c for c in fu.corpus20(channels, channel_switches=False) if c[2] is not None]
    files = [c[1] for c in corpus] + [c[1] for c in c20] + [fu.refusal_files(channels)[2][1]]  # (the 10 ms file: accepted here)
    ctx.streams_alloc(len(files), channels)
    tracks, info = ctx.decode_files(files, rfc=True)
    for i, (name, _, packets, pre, trim) in enumerate(corpus):
        want = fu.rfc_expected(oracle, channels, packets, pre, trim)
        assert info["final_status"][i] == 0 and len(tracks[i]) == len(want), name
        assert np.array_equal(tracks[i], want), name
    # every file, the 20 ms ones too, against the model of the device path on the RFC-mode oracle
    b = pkg.FileBatch(files, channels=channels, rfc=True, flags=pkg.PAGES_GROUP_BY_MODE)
    m_tracks, m_len, m_status, _ = fu.model_decode(pkg, oracle, b)
    for i in range(len(files)):
        assert (info["final_status"][i], info["bad_packet"][i]) == tuple(m_status[i]) and len(tracks[i]) == m_len[i], i
        assert np.array_equal(tracks[i], m_tracks[i]), i
    assert info["final_status"][-1] == 0 and len(tracks[-1]) == 960 + 480 + 960 - 312
    b.close()


@pytest.mark.parametrize("pipeline", [0, 1])
def test_failed_frames_end_their_track_only(pkg, ctx, ct, pipeline):
    """A CELT-only / hybrid frame of <= 1 byte (-18) as a packet's only frame, as the second frame of a two-frame packet, in the
    first packet: the track ends where that packet would have begun, the status names code and packet, the neighbours are whole."""
    files = fu.failing_files(2)
    ctx.streams_alloc(len(files), 2)
    ctx.set_pipeline(pipeline)
    b = pkg.FileBatch([f[1] for f in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE)
    tracks, info = ctx.decode_files(None, batch=b)
    for i, (name, data, bad_seq) in enumerate(files):
        _, want, _, final = fu.drain(ct, data)
        print(name, "final", len(tracks[i]), "planned", b.info["track_samples"][i], "status", info["final_status"][i], info["bad_packet"][i])
        if bad_seq is None:
            assert (info["final_status"][i], info["bad_packet"][i]) == (0, -1) and len(tracks[i]) == b.info["track_samples"][i]
        else:
            assert (info["final_status"][i], info["bad_packet"][i]) == (-18, bad_seq)
            assert len(tracks[i]) == b.packet_start(i, bad_seq)
        assert len(tracks[i]) == len(want) and np.array_equal(tracks[i], want), name
    b.close()


def _scale(pkg, ctx, ct, n, toc, L, checked):
    half = n // 2
    uniq, pre, trim = fu.bulk_files(pkg, half, toc, L)
    files = [r.tobytes() for r in uniq] * 2  # the second half replays the first half's files
    ctx.streams_alloc(n, 2)
    b = pkg.FileBatch(files, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=16)
    assert (b.info["status"] == 0).all() and (b.info["frames"] == 30).all()
    assert (b.info["track_samples"] == 28800 - np.tile(pre + trim, 2)).all()
    ctx.set_pipeline(0)
    t0, i0 = ctx.decode_files(None, batch=b)
    ctx.set_pipeline(1)
    t1, i1 = ctx.decode_files(None, batch=b)
    ctx.set_pipeline(0)
    assert np.array_equal(i0, i1) and (i0["final_status"] == 0).all() and (i0["track_samples"] == b.info["track_samples"]).all()
    for i in range(n):
        assert np.array_equal(t0[i], t1[i]), i  # in order == pipelined
    for i in range(half):
        assert np.array_equal(t0[i], t0[i + half]), i  # the replay
    for i in np.unique(np.linspace(0, n - 1, checked).astype(int)):
        code, want, _, final = fu.drain(ct, files[i])
        assert code == 0 and final == 0 and np.array_equal(t0[i], want), i
    b.close()


def test_scale_celt_16384_files(pkg, ctx, ct):
    _scale(pkg, ctx, ct, 16384, pkg.TOC_CELT_FB_STEREO, 160, 258)


def test_scale_hybrid_4096_files(pkg, ctx, ct):
    _scale(pkg, ctx, ct, 4096, pkg.TOC_HYBRID_FB_STEREO, 120, 258)


@pytest.mark.parametrize("channels", [1, 2])
def test_assembly_kernel_alone(pkg, ctx, channels):
    """k_tracks_assemble on crafted segment lists against a numpy scatter: every src_first / count / dst_first residue modulo 8
    samples, counts of 1, 7, 8, 9, 959, 960 and 2,880, every segment's last sample the last of its track with the guard words
    behind every track intact, failed frames and the tracks they end, n_segs = 0."""
    rng = np.random.default_rng(channels)
    C, ROW = channels, 2880
    ctx.streams_alloc(1, C)
    combos = [(s, c, d) for s in range(8) for c in range(1, 9) for d in range(8)]
    combos += [(s, c, d) for c in (1, 7, 8, 9, 959, 960, 2880) for s in (0, 3, 8) for d in (0, 1, 5, 8, 63)]
    combos = [(s, c, d) for s, c, d in combos if s + c <= ROW]
    n = len(combos)
    n_rows = 37
    pcm = rng.integers(-32768, 32768, (n_rows, ROW, C), dtype=np.int16)
    segs = np.zeros(n, dtype=pkg.TRACK_SEG_DTYPE)
    at = 0
    for i, (s, c, d) in enumerate(combos):  # track i: d samples of guard, the segment, then guard up to the next multiple of 64 (+ 64)
        segs[i] = (rng.integers(0, n_rows), s, c, i, at + d, i % 5, 0)
        at = (at + d + c + 63) // 64 * 64 + 64
    total = at
    res = np.full(n_rows, 960, dtype=np.int32)
    bad_rows = [5, 21]
    res[bad_rows] = -18
    state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
    state["first_bad"] = 2**31 - 1
    closed = rng.choice(n, 40, replace=False)  # tracks that an earlier step has ended at packet 2: segments of packets 2.. write nothing
    state["first_bad"][closed], state["code"][closed] = 2, -18
    want = np.full((total, C), 0x5A5A, dtype=np.int16)
    want_state = state.copy()
    for sg in segs:
        t = sg["track"]
        if res[sg["slot"]] < 0:
            if sg["packet_seq"] < want_state["first_bad"][t]:
                want_state[t] = (sg["packet_seq"], -18)
        elif sg["packet_seq"] < want_state["first_bad"][t]:
            want[sg["dst_first"]:sg["dst_first"] + sg["count"]] = pcm[sg["slot"], sg["src_first"]:sg["src_first"] + sg["count"]]
    bufs = [ctx.dev_alloc(x) for x in (segs.nbytes, pcm.nbytes, res.nbytes, 2 * total * C, state.nbytes)]
    d_segs, d_pcm, d_res, d_tracks, d_state = bufs
    try:
        ctx.h2d(d_segs, segs)
        ctx.h2d(d_pcm, pcm)
        ctx.h2d(d_res, res)
        ctx.h2d(d_tracks, np.full((total, C), 0x5A5A, dtype=np.int16))
        ctx.h2d(d_state, state)
        ctx.tracks_assemble_device(0, d_segs, d_pcm, ROW, d_res, d_tracks, d_state)  # n_segs = 0: nothing
        ctx.synchronize()
        got = np.zeros((total, C), dtype=np.int16)
        ctx.d2h(got, d_tracks)
        assert (got == 0x5A5A).all()
        ctx.tracks_assemble_device(n, d_segs, d_pcm, ROW, d_res, d_tracks, d_state)
        ctx.synchronize()
        ctx.d2h(got, d_tracks)
        got_state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
        ctx.d2h(got_state, d_state)
    finally:
        for p in bufs:
            ctx.dev_free(p)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], [c for c, sg in zip(combos, segs) if sg["dst_first"] <= bad[0] < sg["dst_first"] + sg["count"] + 64][:2])
    assert np.array_equal(got_state, want_state)
    assert (want != 0x5A5A).any(axis=1).sum() > 0.5 * sum(c for _, c, _ in combos)
