"""Shared by the RFC-mode parity tests (tests/test_emul_rfc.py via tools/fuzz_emul_rfc.py, tests/test_gpu_rfc.py): packet
generation over all TOC configurations, framing, and WHICH output entries a packet defines -- the comparison domain."""
import ctypes as C
import json
import os

import numpy as np

MODE_SILK, MODE_HYBRID, MODE_CELT = 1000, 1001, 1002


def dur(toc):
    """samples per frame at 48 kHz named by the TOC (RFC 6716 section 3.1)"""
    if toc & 0x80:
        return (48000 << ((toc >> 3) & 3)) // 400
    if (toc & 0x60) == 0x60:
        return 960 if toc & 8 else 480
    a = (toc >> 3) & 3
    return 2880 if a == 3 else (48000 << a) // 100


def mode_bw(toc):
    if toc & 0x80:
        bw = 1102 + ((toc >> 5) & 3)
        return MODE_CELT, (1101 if bw == 1102 else bw)
    if (toc & 0x60) == 0x60:
        return MODE_HYBRID, (1105 if toc & 0x10 else 1104)
    return MODE_SILK, 1101 + ((toc >> 5) & 3)


def make_packet(rng, cfg, stereo, code, L):
    """One packet of configuration cfg (0..31) with frame-count code 0..3 and random payload; L: bytes per frame (0 or 1: DTX)."""
    toc = (cfg << 3) | (4 if stereo else 0) | code
    body = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    if code == 0:
        return bytes([toc]) + body(L)
    if code == 1:
        return bytes([toc]) + body(2 * L)
    if code == 2:
        L = min(L, 250)
        return bytes([toc, L]) + body(L + int(rng.integers(0, 120)))
    cnt = int(rng.integers(1, 5))
    while dur(toc) * cnt > 5760:
        cnt -= 1
    return bytes([toc, cnt]) + body(cnt * L)


def frame_payloads(oracle, pkt):
    """-> list of the packet's frame payloads (opus_packet_parse_impl through the oracle), or None when the framing fails."""
    lib = oracle.lib
    lib.oc_packet_parse.argtypes = [C.c_char_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    size = (C.c_int16 * 48)()
    tocb, off = C.c_uint8(), C.c_int()
    cnt = lib.oc_packet_parse(pkt, len(pkt), 0, C.byref(tocb), size, C.byref(off), None)
    if cnt < 0 or cnt * dur(pkt[0]) > 5760:
        return None
    out, at = [], off.value
    for k in range(cnt):
        out.append(pkt[at:at + size[k]])
        at += size[k]
    return out


def same_pcm(got, want, fs, frame_lens, prev_mode, toc_mode, pch, channels):
    """Compare a packet's PCM ([frames * fs, channels] each) over the entries the decoder defines.  A frame of at most one
    byte -- and every frame of a lost packet (frame_lens all 0) -- is concealed in the mode of the frame before it; the others
    run in the TOC's mode.  Q3: a SILK-only frame with fewer channels than the decoder defines only its first fs * pch LINEAR
    entries -- of every 20 ms chunk when a longer frame is concealed (the concealment goes 20 ms at a time)."""
    mode = prev_mode
    for k, ln in enumerate(frame_lens):
        concealed = ln <= 1
        if not concealed:
            mode = toc_mode
        a, b = got[k * fs:(k + 1) * fs].reshape(-1), want[k * fs:(k + 1) * fs].reshape(-1)
        if mode == MODE_SILK and pch < channels:
            if concealed and fs > 960:
                keep = np.concatenate([np.arange(c * 960 * channels, c * 960 * channels + 960 * pch) for c in range(fs // 960)])
                a, b = a[keep], b[keep]
            else:
                a, b = a[:fs * pch], b[:fs * pch]
        if not np.array_equal(a, b):
            return False, k
    return True, -1


def conceal_pieces(lost_dur, last_fs):
    """How a concealment of lost_dur samples is cut into device frames (valid duration codes): a frame of the last packet's size
    at a time like opus_decode(NULL), what is left over (30 / 50 ms) as 20 / 40 ms + 10 ms."""
    out, rem = [], lost_dur
    while rem > 0:
        w = min(rem, last_fs)
        rem -= w
        while w > 0:
            piece = next(v for v in (2880, 1920, 960, 480, 240, 120) if v <= w)
            out.append(piece)
            w -= piece
    return out


def fec_plan(last, toc, channels):
    """RFC 6716's opus_decode(decode_fec = 1) for the packet with this TOC after a lost packet; last = (frames, frame duration,
    mode) of the stream's last packet or None.  -> (samples to produce, [concealment frame durations], use the FEC frame?)"""
    lost_dur, last_fs, last_mode = (last[0] * last[1], last[1], last[2]) if last else (960, 120, 0)
    pfs, pmode = dur(toc), mode_bw(toc)[0]
    if lost_dur < pfs or pmode == MODE_CELT or last_mode == MODE_CELT:
        return lost_dur, conceal_pieces(lost_dur, last_fs), False
    return lost_dur, conceal_pieces(lost_dur - pfs, last_fs), True


_REDUNDANT = None


def redundancy_packet(rng, channels_pref=None):
    """A hybrid packet whose redundancy flag is set (tests/golden/rfc_hybrid_redundancy_seeds.json, found by
    tools/find_redundancy_seeds.py: the flag is one range-coded bit of probability 2^-12, random payloads almost never set it).
    -> (packet bytes, kind)"""
    global _REDUNDANT
    if _REDUNDANT is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfc_hybrid_redundancy_seeds.json")
        _REDUNDANT = json.load(open(path))
    pool = [e for e in _REDUNDANT if channels_pref is None or bool(e["toc"] & 4) == (channels_pref == 2)] or _REDUNDANT
    e = pool[int(rng.integers(len(pool)))]
    pay = np.random.default_rng(e["seed"]).integers(0, 256, e["len"], dtype=np.uint8).tobytes()
    return bytes([e["toc"]]) + pay, e["kind"]


# ---- one packet of one stream against its own oracle decoder in RFC mode (any TOC, any frame count, losses, decode_fec) ------------------
def oracle_step(oracle, d, pkt, last, channels):
    """The packet `pkt` (empty: lost, concealed for as long as the stream's last packet was) through the oracle decoder d.
    last = (frame count, frame duration, packet channels, mode) of the stream's last packet that framed, or None.
    -> (reference PCM [5760 + 960, channels] (the decoder's buffer), samples or error, what same_pcm needs: (frame duration, frame
    lengths or None when the framing failed, mode before, TOC mode, packet channels), the new `last`)"""
    before = d.prev_mode()
    if len(pkt) == 0:
        cnt, fs, pch = last[:3] if last else (1, 960, channels)
        ref, r = d.conceal(cnt * fs)
        return ref, r, (fs, [0] * cnt, before, before, pch), last
    ref, r = d.decode(pkt)
    pays = frame_payloads(oracle, pkt)
    toc = pkt[0]
    fs, pch, toc_mode = dur(toc), (2 if toc & 4 else 1), mode_bw(toc)[0]
    lens = None
    if pays is not None:
        last, lens = (len(pays), fs, pch, toc_mode), [len(p) for p in pays]
    return ref, r, (fs, lens, before, toc_mode, pch), last


def same_step(got, res, ref, r, domain, channels):
    """-> None when the decoder under test (PCM `got`, return value `res`) gave what the oracle gave for this packet over the entries the
    packet defines, else what differs"""
    if int(res) != r:
        return ("return value", int(res), r)
    if r <= 0:
        return None
    fs, lens, before, toc_mode, pch = domain
    ok, k = same_pcm(np.asarray(got)[:r], ref[:r], fs, lens, before, toc_mode, pch, channels)
    return None if ok else ("PCM of frame", k)


def oracle_fec_step(oracle, d, pkt, last, channels):
    """opus_decode(decode_fec = 1) of `pkt` for the packet lost before it, through the oracle decoder d.
    -> (reference PCM, samples or error, [(start, duration, frame length, mode, packet channels)]: the spans to compare in turn,
    the mode before)"""
    toc = pkt[0]
    total, pieces, use = fec_plan((last[0], last[1], last[3]) if last else None, toc, channels)
    before = d.prev_mode()
    ref = np.zeros((5760, channels), dtype=np.int16)
    oracle.lib.oc_decode_fec.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int]
    r = oracle.lib.oc_decode_fec(d.h, pkt, len(pkt), ref.ctypes.data, total)
    lpch = last[2] if last else channels
    spans, at = [], 0
    for w in pieces:  # concealed in the mode of the frame before, over the last packet's channels
        spans.append((at, w, 0, None, lpch))
        at += w
    if use:
        spans.append((at, dur(toc), len(frame_payloads(oracle, pkt)[0]), mode_bw(toc)[0], 2 if toc & 4 else 1))
    return ref, r, spans, before


def same_fec_step(got, res, ref, r, spans, before, channels):
    if int(res) != r:
        return ("fec: return value", int(res), r)
    if r <= 0:
        return None
    for at, w, ln, m, pch in spans:
        ok, _ = same_pcm(np.asarray(got)[at:at + w], ref[at:at + w], w, [ln], before, before if m is None else m, pch, channels)
        if not ok:
            return ("fec: PCM of the span at", at)
    return None


# ---- the RFC walks of tests/test_gpu_rfc.py: what each plan draws (tools/kernel_branches.py decodes the same packets in emulation) ---------
def _walk(p_new, pick_cfg=None):
    """a pick() that keeps a stream's configuration and draws a new one with probability p_new"""
    state = {}

    def pick(s, f, rng):
        if s not in state or rng.random() < p_new:
            state[s] = pick_cfg(rng) if pick_cfg else int(rng.integers(32))
        return state[s], int(rng.choice([0, 0, 0, 1, 2, 3]))
    return pick


def rfc_plan(name):
    """A fresh plan (its pick() keeps state per stream): streams, steps, pick(stream, step, rng) -> (cfg, code), the seed's base (the
    seed is base + decoder channels), the shares of lost packets, DTX frames, packets recovered with decode_fec before them, and
    of hybrid packets with the redundancy flag set."""
    plans = {
        # stream s decodes configuration s % 32 with frame-count code (s // 32) % 4
        "all_configs": dict(streams=256, steps=4, pick=lambda s, f, rng: (s % 32, (s // 32) % 4), seed=11),
        "switches": dict(streams=384, steps=8, pick=_walk(0.4), seed=77, p_redundant=0.06),
        "loss": dict(streams=512, steps=10, pick=_walk(0.3), seed=501, p_loss=0.3, p_dtx=0.06, p_redundant=0.05),
        # (mostly SILK-only / hybrid)
        "fec": dict(streams=384, steps=10, seed=801, p_loss=0.15, p_dtx=0.04, p_fec=0.3,
                    pick=_walk(0.25, lambda rng: int(rng.integers(32)) if rng.random() < 0.3 else int(rng.integers(16)))),
        "celt_bursts": dict(streams=640, steps=14, pick=lambda s, f, rng: (16 + s % 16, int(rng.choice([0, 0, 1, 3]))), seed=901,
                            p_loss=0.5, p_dtx=0.03),
    }
    return dict({"p_loss": 0.0, "p_dtx": 0.0, "p_fec": 0.0, "p_redundant": 0.0, "name": name}, **plans[name])


RFC_PLANS = ("all_configs", "switches", "loss", "fec", "celt_bursts")


def draw_step(oracle, plan, rng, f, channels):
    """One step of a plan: -> (the packet of every stream, b"" where it is lost; the streams that first recover the packet before
    from this one).  The order of the draws is part of the plans: a change moves every test that walks them."""
    pk = []
    for s in range(plan["streams"]):
        if rng.random() < plan["p_loss"]:
            pk.append(b"")
            continue
        cfg, code = plan["pick"](s, f, rng)
        stereo = (channels == 2) if rng.random() < 0.85 else bool(rng.integers(2))
        L = int(rng.integers(0, 2)) if rng.random() < plan["p_dtx"] else int(rng.choice([3, 8, 20, 40, 80, 120, 160, 300]))
        if rng.random() < plan["p_redundant"]:  # a hybrid packet with its redundancy flag set
            pk.append(redundancy_packet(rng, channels if rng.random() < 0.85 else None)[0])
        else:
            pk.append(make_packet(rng, cfg, stereo, code, L))
    who = [s for s in range(plan["streams"]) if len(pk[s]) and rng.random() < plan["p_fec"] and frame_payloads(oracle, pk[s]) is not None]
    return pk, who
