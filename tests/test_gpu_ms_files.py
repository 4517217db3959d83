"""Whole multistream Ogg Opus files on the GPU (opusgpu_ms_files_decode / MultistreamContext.decode_files, k_ms_tracks_assemble;
include/opusgpu.h WHOLE FILES / MULTISTREAM): N family-1 files in, N trimmed interleaved tracks out, every sample against an
OracleMs that decodes every packet whole (tests/ms_files_util.py)."""
import numpy as np
import pytest

import files_util as fu
import ms_files_util as mf
import ms_util
from ms_util import LAYOUTS, OracleMs

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A


@pytest.mark.parametrize("rfc", [False, True])
@pytest.mark.parametrize("name", ["5.1", "7.1", "muted", "duplicated", "all-coupled", "mono", "stereo"])
def test_whole_files_equal_the_oracle(pkg, oracle, name, rfc):
    """Pre-skips of 0 - 1,000, end trims of 0 - 700; reference mode: packets of codes 0 - 3; RFC mode: packets of 10, 20 and 40 ms."""
    layout = LAYOUTS[name]
    n = 9
    rng = np.random.default_rng(sum(name.encode()) + rfc)
    corpus = mf.corpus(pkg, rng, layout, n, 7, rfc=rfc)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, rfc=rfc, threads=2)
    assert (b.info["status"] == 0).all()
    tracks, info = ms.decode_files(None, batch=b)
    orc = OracleMs(oracle, layout, n, rfc=rfc)
    for i, (_, els, ps, trim) in enumerate(corpus):
        want = mf.expected_track(orc, i, els, ps, trim)
        print(name, rfc, i, "pre-skip", ps, "trim", trim, "samples", len(tracks[i]), "planned", b.info["track_samples"][i], "oracle", len(want))
        assert (info["final_status"][i], info["bad_packet"][i]) == (0, -1), i
        assert info["track_samples"][i] == b.info["track_samples"][i] == len(tracks[i]) == len(want), i
        bad = np.argwhere(tracks[i] != want)
        assert not len(bad), (i, "first differences (sample, channel)", bad[:4].tolist(), len(bad))
    b.close()
    ms.close()


@pytest.mark.parametrize("rfc", [False, True])
def test_two_runs_of_one_batch_are_identical(pkg, rfc):
    """Reset and the reuse of the elementary PCM buffers across steps: the second run starts from the first one's leftovers."""
    layout = LAYOUTS["5.1"]
    rng = np.random.default_rng(12)
    corpus = mf.corpus(pkg, rng, layout, 10, 6, rfc=rfc)
    ms = pkg.MultistreamContext(0, 12, *layout)
    b = pkg.MsFileBatch([c[0] for c in corpus], layout, rfc=rfc)
    t0, i0 = ms.decode_files(None, batch=b)
    t1, i1 = ms.decode_files(None, batch=b)
    assert np.array_equal(i0, i1) and (i0["final_status"] == 0).all() and (i0["track_samples"] > 0).all()
    for x, y in zip(t0, t1):
        assert np.array_equal(x, y)
    b.close()
    ms.close()


def test_a_failed_elementary_frame_ends_its_track_only(pkg, oracle):
    """One elementary stream's CELT frame cut to one byte (-18) in packet p of one file: that track ends where packet p would have
    begun, and every other file is what it is without the damaged file in the batch."""
    layout = LAYOUTS["5.1"]
    rng = np.random.default_rng(40)
    n, p, victim = 8, 3, 2
    files, all_els = [], []
    for i in range(n):
        tocs = mf.stream_tocs(rng, layout)
        if i == victim:
            tocs[1] = 0xFC  # the stream that is damaged: CELT FB
        els, pk = mf.packets(pkg, rng, tocs, [(1, False) if j == p else mf.SHAPES[(i + j) % 4] for j in range(7)])
        if i == victim:
            els[p][1] = bytes([0xFC, 0x55])
            pk[p] = ms_util.ms_packet(pkg, els[p])
        files.append(fu.opus_file(mf.paged(pk, 3), pre_skip=mf.PRE_SKIPS[i % 6], serial=70 + i, end_trim=100 * i,
                                  head=mf.head(layout, mf.PRE_SKIPS[i % 6]))[0])
        all_els.append(els)
    ms = pkg.MultistreamContext(0, n, *layout)
    b = pkg.MsFileBatch(files, layout)
    assert (b.info["status"] == 0).all()
    tracks, info = ms.decode_files(None, batch=b)
    others = [f for i, f in enumerate(files) if i != victim]
    clean, cinfo = ms.decode_files(others)
    assert (cinfo["final_status"] == 0).all()
    print("victim: final", len(tracks[victim]), "planned", b.info["track_samples"][victim], "status", info["final_status"][victim], info["bad_packet"][victim])
    assert (info["final_status"][victim], info["bad_packet"][victim]) == (-18, p)
    assert len(tracks[victim]) == info["track_samples"][victim] == b.packet_start(victim, p) > 0
    orc = OracleMs(oracle, layout, 1)
    want = mf.expected_track(orc, 0, all_els[victim][:p], mf.PRE_SKIPS[victim % 6], 0)
    assert np.array_equal(tracks[victim], want)  # what lies before packet p is whole
    for i, t in zip([i for i in range(n) if i != victim], clean):
        assert (info["final_status"][i], info["bad_packet"][i]) == (0, -1) and np.array_equal(tracks[i], t), i
    b.close()
    ms.close()


KERNEL_LAYOUTS = {
    "mono": LAYOUTS["mono"],                              # C = 1
    "c3-unused-stream": (3, 3, 1, [3, 255, 0]),           # C = 3: stream 1 feeds nothing and is not staged
    "muted": LAYOUTS["muted"],                            # C = 5
    "duplicated": LAYOUTS["duplicated"],                  # C = 5
    "5.1": LAYOUTS["5.1"],                                # C = 6
    "c8-muted-duplicated": (8, 5, 3, [0, 6, 1, 2, 255, 4, 4, 7]),  # C = 8, 2,880-sample rows: more than one LDS tile
}


@pytest.mark.parametrize("name", list(KERNEL_LAYOUTS))
def test_fused_assembly_kernel_alone(pkg, name):
    """k_ms_tracks_assemble on crafted elementary PCM and segment lists against a numpy scatter through ms_util.mapping_apply:
    every src_first / count / dst_first residue modulo 8 samples, counts of 0, 1, 7, 8, 9, 959, 960 and 2,880, guard words around
    every track, failed rows (a negative result in a middle elementary stream; two of them: the first in stream order counts) and
    the tracks they end, tracks an earlier step has closed, n_segs = 0."""
    layout = KERNEL_LAYOUTS[name]
    C, S, cp, mp = layout
    mono = S - cp
    rng = np.random.default_rng(C + S)
    ROW, n_rows = 2880, 13
    combos = [(s, c, d) for s in range(8) for c in range(1, 9) for d in range(8)]
    combos += [(s, c, d) for c in (0, 1, 7, 8, 9, 959, 960, 2880) for s in (0, 3, 8, 1913) for d in (0, 1, 5, 8, 63)]
    combos = [(s, c, d) for s, c, d in combos if s + c <= ROW]
    n = len(combos)
    pc = rng.integers(-32768, 32768, (n_rows * cp, ROW, 2), dtype=np.int16)
    pm = rng.integers(-32768, 32768, (n_rows * mono, ROW), dtype=np.int16)
    rc = np.full(n_rows * cp, ROW, dtype=np.int32)
    rm = np.full(n_rows * mono, ROW, dtype=np.int32)
    codes = np.full((n_rows, S), ROW, dtype=np.int32)
    codes[5, S // 2] = -18          # a middle elementary stream
    if S >= 3:
        codes[9, 1], codes[9, S - 1] = -4, -18  # the first negative one in stream order is the row's
    codes[11] = 960                 # a shorter row: a result, not an error
    for r in range(n_rows):
        rc[r * cp:(r + 1) * cp] = codes[r, :cp]
        rm[r * mono:(r + 1) * mono] = codes[r, cp:]
    row_res = np.array([next((v for v in codes[r] if v < 0), codes[r, 0]) for r in range(n_rows)])
    mapped = [ms_util.mapping_apply(layout, [pc[r * cp + s] if s < cp else pm[r * mono + s - cp][:, None] for s in range(S)], ROW)
              for r in range(n_rows)]
    segs = np.zeros(n, dtype=pkg.TRACK_SEG_DTYPE)
    at = 0
    for i, (s, c, d) in enumerate(combos):  # track i: d samples of guard, the segment, then guard up to the next multiple of 64 (+ 64)
        row = int(rng.integers(0, n_rows))
        if row == 11 and s + c > 960:
            row = 0
        segs[i] = (row, s, c, i, at + d, i % 5, 0)
        at = (at + d + c + 63) // 64 * 64 + 64
    total = at
    state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
    state["first_bad"] = 2**31 - 1
    closed = rng.choice(n, 40, replace=False)  # tracks that an earlier step has ended at packet 2: segments of packets 2.. write nothing
    state["first_bad"][closed], state["code"][closed] = 2, -18
    want = np.full((total, C), GUARD, dtype=np.int16)
    want_state = state.copy()
    for sg in segs:
        t, r = sg["track"], sg["slot"]
        if row_res[r] < 0:
            if sg["packet_seq"] < want_state["first_bad"][t]:
                want_state[t] = (sg["packet_seq"], row_res[r])
        elif sg["packet_seq"] < want_state["first_bad"][t]:
            want[sg["dst_first"]:sg["dst_first"] + sg["count"]] = mapped[r][sg["src_first"]:sg["src_first"] + sg["count"]]
    ms = pkg.MultistreamContext(0, 1, *layout)
    ctx = pkg.Context(0)
    bufs = [ctx.dev_alloc(max(x, 16)) for x in (segs.nbytes, pc.nbytes, pm.nbytes, rc.nbytes, rm.nbytes, 2 * total * C, state.nbytes)]
    d_segs, d_pc, d_pm, d_rc, d_rm, d_tracks, d_state = bufs
    try:
        for dptr, a in ((d_segs, segs), (d_pc, pc), (d_pm, pm), (d_rc, rc), (d_rm, rm), (d_state, state)):
            if a.nbytes:
                ctx.h2d(dptr, a)
        ctx.h2d(d_tracks, np.full((total, C), GUARD, dtype=np.int16))
        ms.tracks_assemble_device(0, d_segs, d_pc, d_pm, ROW, d_rc, d_rm, d_tracks, d_state)  # n_segs = 0: nothing
        ms.synchronize()
        got = np.zeros((total, C), dtype=np.int16)
        ctx.d2h(got, d_tracks)
        assert (got == GUARD).all()
        ms.tracks_assemble_device(n, d_segs, d_pc, d_pm, ROW, d_rc, d_rm, d_tracks, d_state)
        ms.synchronize()
        ctx.d2h(got, d_tracks)
        got_state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
        ctx.d2h(got_state, d_state)
    finally:
        for p in bufs:
            ctx.dev_free(p)
        ctx.close()
        ms.close()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (len(bad), bad[:8], [c for c, sg in zip(combos, segs) if sg["dst_first"] - 64 <= bad[0] < sg["dst_first"] + sg["count"] + 64][:2])
    assert np.array_equal(got_state, want_state)
    assert (want_state["first_bad"] != state["first_bad"]).sum() > 0
    written = sum(c for (_, c, _), sg in zip(combos, segs) if row_res[sg["slot"]] >= 0 and sg["packet_seq"] < state["first_bad"][sg["track"]])
    assert (want != GUARD).any(axis=1).sum() > 0.5 * written
