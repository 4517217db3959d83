"""Multistream decoding on the GPU (include/opusgpu.h, MULTISTREAM), every sample against the oracle composition: each elementary
packet decoded by an oracle decoder of 2 channels (coupled streams) or 1 (mono streams), then mapped to the output channels."""
import numpy as np
import pytest

import ms_util
from ms_util import LAYOUTS, TOCS_20MS, OracleMs

pytestmark = pytest.mark.gpu

SENTINEL = 0x1357


def _stream_tocs(rng, layout, n):
    """Every elementary stream keeps one TOC configuration and stereo bit (which disagrees with the stream type for about half of
    them); stream 0 is CELT FB, the stream the error rows damage."""
    _, S, _, _ = layout
    t = rng.choice(np.array(TOCS_20MS, np.uint8), (n, S))
    t[:, 0] = 0xF8 | (t[:, 0] & 4)
    return t


def _step_packets(rng, layout, n, frames=1, bad=(), toc_of=None):
    """n multistream packets of `frames` 20 ms frames per elementary stream (TOC toc_of[i, s]); rows in
    `bad` carry one-byte CELT frames in stream 0 (-18)."""
    _, S, _, _ = layout
    els = []
    for i in range(n):
        el = [ms_util.elementary_packet(rng, int(toc_of[i, s]), frames, vbr=bool(rng.random() < 0.5)) for s in range(S)]
        if i in bad:
            el[0] = bytes([0xFC if frames == 1 else 0xFD]) + bytes([7]) * frames  # CELT FB, one byte per frame
        els.append(el)
    return els


def _check(res, pcm, want, cap, i, tag):
    wp, wr = want
    assert res[i] == wr, (tag, i, res[i], wr)
    if wr > 0:
        bad = np.argwhere(pcm[i, :wr] != wp)
        assert not len(bad), (tag, i, "first differences (sample, channel)", bad[:4].tolist(), len(bad))
    else:
        assert (pcm[i] == SENTINEL).all(), (tag, i, "a failed row's PCM block was written")


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_ms_host_path_matches_oracle(pkg, oracle, name):
    layout = LAYOUTS[name]
    ch, S, cp, mp = layout
    n = 6
    rng = np.random.default_rng(sum(name.encode()))
    ms = pkg.MultistreamContext(0, n, ch, S, cp, mp)
    orc = OracleMs(oracle, layout, n)
    tocs = _stream_tocs(rng, layout, n)
    # 20 ms steps, a step of two-frame packets, error rows, empty packets, a partial reset, two-frame packets with an error row (a
    # failing first frame ends its stream's packet)
    plan = [(1, 1, ()), (1, 1, (2,)), (2, 2, ()), (1, 1, ()), ("empty", 2, ()), (1, 1, (0, 5)), ("reset", 0, ()), (1, 1, ()),
            ("empty", 1, ()), (2, 2, (4,))]
    for k, (frames, cap, bad) in enumerate(plan):
        if frames == "reset":
            ms.reset(1, 2)
            orc.reset(1)
            orc.reset(2)
            continue
        if frames == "empty":
            els = _step_packets(rng, layout, n, toc_of=tocs)
            els = [None if i % 2 == 0 else e for i, e in enumerate(els)]
        else:
            els = _step_packets(rng, layout, n, frames, bad, toc_of=tocs)
        pkts = [None if e is None else ms_util.ms_packet(pkg, e) for e in els]
        pcm = np.full((n, cap * 960, ch), SENTINEL, dtype=np.int16)
        pcm, res = ms.decode_packets(range(n), pkts, frame_capacity=cap, pcm=pcm)
        for i in range(n):
            _check(res, pcm, orc.decode(i, els[i], cap), cap, i, (name, k))
    ms.close()


@pytest.mark.parametrize("name", ["mono", "stereo"])
def test_ms_single_stream_equals_plain_context(pkg, name):
    ch, S, cp, mp = LAYOUTS[name]
    n = 16
    rng = np.random.default_rng(5)
    ms = pkg.MultistreamContext(0, n, ch, S, cp, mp)
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, ch)
    tocs = _stream_tocs(rng, LAYOUTS[name], n)
    for k in range(4):
        els = _step_packets(rng, LAYOUTS[name], n, bad=(3,) if k == 1 else (), toc_of=tocs)
        pk = [e[0] for e in els]
        if k == 3:
            pk[4] = b""
        a_pcm, a_res = ms.decode_packets(range(n), [ms_util.ms_packet(pkg, e) if p else b"" for e, p in zip(els, pk)])
        b_pcm, b_res = ctx.decode_packets(np.arange(n), pk)
        assert np.array_equal(a_res, b_res), k
        ok = a_res > 0
        assert np.array_equal(a_pcm[ok], b_pcm[ok]), k
    ctx.close()
    ms.close()


def _device_rows(pkg, layout, pkts, decoders):
    """Single-frame multistream packets -> (row descriptors [n * streams], arena) for opusgpu_ms_decode_step_device."""
    lay = pkg.ms_layout(*layout)
    descs, arena, base = [], [], 0
    for p, d in zip(pkts, decoders):
        dur, fr = pkg.ms_packet_to_frames(lay, p, decoder=d)
        for s in fr:
            o, ln, fl = s[0]
            descs.append((d, base + o, ln, fl))
        arena.append(p)
        base += len(p)
    return np.array(descs, dtype=pkg.DESC_DTYPE), np.frombuffer(b"".join(arena) + bytes(16), dtype=np.uint8)


def _run_device(pkg, ctx, ms, n, ch, descs, arena, rfc=False):
    fr = 2880 if rfc else 960
    bufs = [ctx.dev_alloc(descs.nbytes), ctx.dev_alloc(arena.nbytes), ctx.dev_alloc(n * fr * ch * 2), ctx.dev_alloc(4 * n)]
    try:
        ctx.h2d(bufs[0], descs)
        ctx.h2d(bufs[1], arena)
        ctx.h2d(bufs[2], np.full(n * fr * ch, SENTINEL, np.int16))
        ms.decode_step_device(n, bufs[0], bufs[1], bufs[2], bufs[3])
        ms.synchronize()
        pcm = np.zeros((n, fr, ch), np.int16)
        res = np.zeros(n, np.int32)
        ctx.d2h(pcm, bufs[2])
        ctx.d2h(res, bufs[3])
    finally:
        for b in bufs:
            ctx.dev_free(b)
    return pcm, res


@pytest.mark.parametrize("name", ["5.1", "7.1", "duplicated", "muted", "family255-mono8"])
def test_ms_device_path_equals_host_path(pkg, oracle, name):
    layout = LAYOUTS[name]
    ch, S, cp, mp = layout
    n = 8
    rng = np.random.default_rng(21)
    a = pkg.MultistreamContext(0, n, ch, S, cp, mp)
    b = pkg.MultistreamContext(0, n, ch, S, cp, mp)
    ctx = pkg.Context(0)
    orc = OracleMs(oracle, layout, n)
    order = rng.permutation(n)  # rows in any order of decoders
    tocs = _stream_tocs(rng, layout, n)
    for k in range(3):
        els = _step_packets(rng, layout, n, bad=(1,) if k == 1 else (), toc_of=tocs)
        pkts = [ms_util.ms_packet(pkg, e) for e in els]
        h_pcm = np.full((n, 960, ch), SENTINEL, np.int16)
        h_pcm, h_res = a.decode_packets(range(n), pkts, pcm=h_pcm)
        descs, arena = _device_rows(pkg, layout, [pkts[d] for d in order], order)
        d_pcm, d_res = _run_device(pkg, ctx, b, n, ch, descs, arena)
        for r, d in enumerate(order):
            assert d_res[r] == h_res[d], (k, d)
            assert np.array_equal(d_pcm[r], h_pcm[d]), (k, d)
            _check(h_res, h_pcm, orc.decode(d, els[d]), 1, d, (name, k))
    # refused rows: decoders that differ within a row, a decoder out of range -- nothing of them is decoded
    els = _step_packets(rng, layout, n, toc_of=tocs)
    pkts = [ms_util.ms_packet(pkg, e) for e in els]
    descs, arena = _device_rows(pkg, layout, pkts, range(n))
    if S > 1:
        descs[1 * S + S - 1]["stream"] = 0
    descs[2 * S:3 * S]["stream"] = n + 3
    d_pcm, d_res = _run_device(pkg, ctx, b, n, ch, descs, arena)
    bad = {2} | ({1} if S > 1 else set())
    for r in range(n):
        if r in bad:
            assert d_res[r] == -1 and (d_pcm[r] == SENTINEL).all()
        else:
            _check(d_res, d_pcm, orc.decode(r, els[r]), 1, r, (name, "refusals"))
    # the refused rows' decoders were not touched: their next packets decode like the oracle's
    for r in sorted(bad):
        e = _step_packets(rng, layout, 1, toc_of=tocs[r:r + 1])[0]
        p, res = b.decode_packets([r], [ms_util.ms_packet(pkg, e)])
        w = orc.decode(r, e)
        assert res[0] == w[1] and np.array_equal(p[0, :w[1]], w[0])
    ctx.close()
    a.close()
    b.close()


def test_ms_rfc_mode_with_losses(pkg, oracle):
    layout = LAYOUTS["5.1"]
    ch, S, cp, mp = layout
    n, cap = 6, 3
    rng = np.random.default_rng(8)
    ms = pkg.MultistreamContext(0, n, ch, S, cp, mp)
    ms.set_mode(True)
    orc = OracleMs(oracle, layout, n, rfc=True)
    # coupled streams CELT FB, mono streams SILK WB (a stream keeps its mode): 20, 10, 40 ms, a loss, 60 ms, frame counts that
    # differ between streams of one packet (RFC mode takes them), a loss
    celt10, celt20, silk10, silk20, silk40, silk60 = 0xF0, 0xF8, 0x40, 0x48, 0x50, 0x58
    plan = [
        [(celt20, 1)] * cp + [(silk20, 1)] * (S - cp),
        [(celt10, 1)] * cp + [(silk10, 1)] * (S - cp),
        [(celt10 | 4, 4)] * cp + [(silk40, 1)] * (S - cp),
        "lost",
        [(celt20, 3)] * cp + [(silk60, 1)] * (S - cp),
        [(celt10, 2), (celt20 | 4, 1)] + [(silk20, 1), (silk10, 2)],
        "lost",
        [(celt10, 4)] * cp + [(silk40, 1)] * (S - cp),
    ]
    for k, step in enumerate(plan):
        if step == "lost":
            els = [None] * n
        else:
            els = [[ms_util.elementary_packet(rng, t, f, vbr=bool(rng.random() < 0.5)) for t, f in step] for _ in range(n)]
            if k == 4:
                els[3] = None  # a loss in a step of packets
        pkts = [None if e is None else ms_util.ms_packet(pkg, e) for e in els]
        pcm = np.full((n, cap * 960, ch), SENTINEL, dtype=np.int16)
        pcm, res = ms.decode_packets(range(n), pkts, frame_capacity=cap, pcm=pcm)
        for i in range(n):
            _check(res, pcm, orc.decode(i, els[i], cap), cap, i, ("rfc", k))
    ms.close()


def test_ms_fullsize_51_device(pkg, oracle):
    """65,536 5.1 decoders x 3 steps on the device path, every sample against batch_decode_var of the elementary streams."""
    layout = LAYOUTS["5.1"]
    ch, S, cp, mp = layout
    n, steps = 65536, 3
    rng = np.random.default_rng(65536)
    ms = pkg.MultistreamContext(0, n, ch, S, cp, mp)
    ctx = pkg.Context(0)
    # one per elementary stream for all three steps: hybrid and CELT, mono and stereo packets
    tocs = np.array([0x68, 0x7C, 0xF8, 0xFC, 0xBC, 0x6C, 0x98], np.uint8)
    el_arena, el_off, el_len = [], np.zeros((steps, n, S), np.int64), np.zeros((steps, n, S), np.int32)
    descs_all, arenas = [], []
    at = 0
    for k in range(steps):
        # elementary packets: one TOC per (decoder, stream), payloads of 40..160 bytes
        toc = tocs[(np.arange(n * S) * 7 + (np.arange(n * S) // 5)) % len(tocs)].reshape(n, S)
        lens = rng.integers(40, 161, (n, S)).astype(np.int32)
        pay = rng.integers(0, 256, int(lens.sum()) + n * S, dtype=np.uint8)
        # multistream packet of decoder d: [toc, len, payload] for every stream but the last, [toc, payload] for the last
        tot = (1 + lens).sum(axis=1) + (S - 1)
        ms_base = np.concatenate([[0], np.cumsum(tot)[:-1]])
        blob = np.zeros(int(tot.sum()) + 16, np.uint8)
        descs = np.zeros(n * S, dtype=pkg.DESC_DTYPE)
        p = 0
        cur = ms_base.copy()
        for s in range(S):
            blob[cur] = toc[:, s]
            cur += 1
            if s != S - 1:
                blob[cur] = lens[:, s]  # < 252: one byte
                cur += 1
            idx = cur[:, None] + np.arange(160)[None, :]
            m = np.arange(160)[None, :] < lens[:, s][:, None]
            src = p + np.concatenate([[0], np.cumsum(lens[:, s])[:-1]])
            blob[idx[m]] = pay[(src[:, None] + np.arange(160)[None, :])[m]]
            descs["stream"][s::S] = np.arange(n)
            descs["offset"][s::S] = cur
            descs["len"][s::S] = lens[:, s]
            # elementary packet in standard framing for the oracle: TOC at cur - 1 (- 2 for the self-delimited ones)
            el_off[k, :, s] = at + (cur - (2 if s != S - 1 else 1))
            el_len[k, :, s] = lens[:, s] + (2 if s != S - 1 else 1)
            p += int(lens[:, s].sum())
            cur += lens[:, s]
        # flags from the TOC bytes (opusgpu_packet_to_frames' fields: mode, bandwidth, stereo)
        flag_of = {int(t): pkg.packet_to_frames(bytes([int(t), 0, 0]))[0][2] for t in tocs}
        descs["flags"] = np.vectorize(lambda t: flag_of[int(t)])(toc.reshape(-1))
        # the oracle's packets: self-delimited ones become standard ones by dropping their length byte
        std = blob.copy()
        for s in range(S - 1):
            o = (el_off[k, :, s] - at).astype(np.int64)
            std[o + 1] = std[o]  # [toc, len, payload] -> [., toc, payload]: the standard packet starts one byte later
            el_off[k, :, s] += 1
            el_len[k, :, s] -= 1
        el_arena.append(std)
        at += std.size
        descs_all.append(descs)
        arenas.append(blob)
    arena = np.concatenate(el_arena)
    want = {}
    for kind, ss, c in (("c", range(cp), 2), ("m", range(cp, S), 1)):
        offs = el_off[:, :, list(ss)].reshape(steps, -1)
        lens_ = el_len[:, :, list(ss)].reshape(steps, -1)
        pcm_o, ret_o = oracle.batch_decode_var(c, arena, offs, lens_)
        want[kind] = (pcm_o.reshape(n, len(ss), steps, 960, c), ret_o.reshape(n, len(ss), steps))
    bufs = [ctx.dev_alloc(n * S * 16), ctx.dev_alloc(max(a.nbytes for a in arenas)), ctx.dev_alloc(n * 960 * ch * 2), ctx.dev_alloc(4 * n)]
    try:
        for k in range(steps):
            ctx.h2d(bufs[0], descs_all[k])
            ctx.h2d(bufs[1], arenas[k])
            ms.decode_step_device(n, bufs[0], bufs[1], bufs[2], bufs[3])
            ms.synchronize()
            pcm = np.zeros((n, 960, ch), np.int16)
            res = np.zeros(n, np.int32)
            ctx.d2h(pcm, bufs[2])
            ctx.d2h(res, bufs[3])
            rets = np.concatenate([want["c"][1][:, :, k], want["m"][1][:, :, k]], axis=1)
            first_neg = np.where((rets < 0).any(axis=1), rets.min(axis=1), 960)  # (one negative code at most per row here)
            assert np.array_equal(res, first_neg), k
            for c in range(ch):
                m = mp[c]
                src = want["c"][0][:, m // 2, k, :, m % 2] if m < 2 * cp else want["m"][0][:, m - 2 * cp, k, :, 0]
                ok = res > 0
                bad = np.argwhere(pcm[ok, :, c] != src[ok])
                assert not len(bad), (k, c, bad[:3].tolist(), len(bad))
    finally:
        for b in bufs:
            ctx.dev_free(b)
        ctx.close()
        ms.close()
