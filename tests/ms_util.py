"""Helpers of the multistream tests: self-delimited framing (RFC 6716 Appendix B), multistream packets made of standard
elementary packets, and the oracle composition a multistream decode must equal (each elementary packet decoded by an oracle
decoder of 2 channels for coupled streams and 1 for mono ones, then mapped to the output channels)."""
import numpy as np

# the layouts of the multistream tests: (channels, streams, coupled, mapping)
LAYOUTS = {
    "5.1": (6, 4, 2, [0, 4, 1, 2, 3, 5]),
    "7.1": (8, 5, 3, [0, 6, 1, 2, 3, 4, 5, 7]),
    "family255-mono8": (8, 8, 0, list(range(8))),
    "all-coupled": (4, 2, 2, [0, 1, 2, 3]),
    "muted": (5, 3, 1, [0, 1, 255, 2, 3]),
    "duplicated": (5, 2, 1, [0, 1, 2, 0, 2]),
    "mono": (1, 1, 0, [0]),
    "stereo": (2, 1, 1, [0, 1]),
}

# TOC bytes (code 0) of the payload mix: SILK NB / WB, hybrid SWB / FB, CELT NB / WB / FB, mono and stereo (the stereo bit
# disagrees with the stream type for half of them, whatever the stream is)
TOCS_20MS = [0x08, 0x0C, 0x48, 0x4C, 0x68, 0x7C, 0x98, 0xBC, 0xF8, 0xFC]


def enc_size(n):
    """RFC 6716 section 3.2.1: one byte below 252, else two."""
    if n < 252:
        return bytes([n])
    b0 = 252 + (n & 3)
    return bytes([b0, (n - b0) >> 2])


def self_delimit(pkg, pkt):
    """Standard framing -> self-delimited framing (RFC 6716 Appendix B): the size of the last frame (CBR codes: of every frame)
    goes in front of the frame data, behind every other length."""
    fr = pkg.packet_to_frames(pkt)
    assert not isinstance(fr, int), (fr, pkt[:4])
    po = fr[0][0]
    return pkt[:po] + enc_size(fr[-1][1]) + pkt[po:]


def ms_packet(pkg, elementary):
    """Multistream packet of elementary packets P_0 .. P_{S-1} in standard framing."""
    return b"".join(self_delimit(pkg, p) for p in elementary[:-1]) + bytes(elementary[-1])


def rand_payload(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def elementary_packet(rng, toc, frames=1, vbr=False, pad=0, sizes=None):
    """A standard-framing packet of `frames` frames with TOC `toc` (frame-count code bits are set here) and random payloads."""
    toc &= 0xFC
    if sizes is None:
        sizes = [int(rng.integers(3, 120))] * frames if not vbr else [int(rng.integers(3, 300)) for _ in range(frames)]
    pays = [rand_payload(rng, s) for s in sizes]
    if frames == 1:
        return bytes([toc]) + pays[0]
    if frames == 2 and not vbr and not pad:
        return bytes([toc | 1]) + b"".join(pays)
    if frames == 2 and vbr and not pad:
        return bytes([toc | 2]) + enc_size(sizes[0]) + b"".join(pays)
    ch = frames | (0x80 if vbr else 0) | (0x40 if pad else 0)
    hdr = bytes([toc | 3, ch])
    if pad:
        p, padb = pad, b""
        while p >= 255:
            padb += b"\xff"
            p -= 254
        hdr += padb + bytes([p])  # (the `pad` padding bytes themselves go at the end)
    if vbr:
        hdr += b"".join(enc_size(s) for s in sizes[:-1])
    return hdr + b"".join(pays) + bytes(pad)


def mapping_apply(layout, per_stream, T):
    """per_stream[s]: int16 [>= T, 2 or 1] -> int16 [T, channels] (get_left / right / mono_channel)."""
    channels, streams, coupled, mapping = layout
    out = np.zeros((T, channels), dtype=np.int16)
    for c in range(channels):
        m = mapping[c]
        if m == 255:
            continue
        if m < 2 * coupled:
            out[:, c] = per_stream[m // 2][:T, m % 2]
        else:
            out[:, c] = per_stream[m - coupled][:T, 0]
    return out


class OracleMs:
    """n multistream decoders of one layout on the oracle: one oracle decoder per elementary stream."""

    def __init__(self, oracle, layout, n, rfc=False):
        self.layout = layout
        _, streams, coupled, _ = layout
        self.decs = [[oracle.decoder(2 if s < coupled else 1) for s in range(streams)] for _ in range(n)]
        self.last = [[0] * streams for _ in range(n)]  # RFC mode: duration of the stream's last packet (0: none)
        for row in self.decs:
            for d in row:
                d.init()
                if rfc:
                    d.set_rfc(True)
        self.rfc = rfc

    def reset(self, i):
        for s, d in enumerate(self.decs[i]):
            d.init()
            if self.rfc:
                d.set_rfc(True)
            self.last[i][s] = 0

    def decode(self, i, elementary, cap=1):
        """elementary: list of standard packets, or None for an empty / lost packet -> (pcm [T, ch] or None, result).
        Every elementary stream is decoded (the library's documented difference: the reference stops at a failing stream)."""
        _, streams, coupled, _ = self.layout
        outs, rets = [], []
        for s in range(streams):
            d = self.decs[i][s]
            if elementary is None:
                if self.rfc:
                    buf, r = d.conceal(self.last[i][s] or 960)
                else:
                    buf, r = d.decode_cap(b"", min(cap, 6))
            else:
                buf, r = d.decode_cap(elementary[s], cap)
                if self.rfc and r > 0:
                    self.last[i][s] = r
            outs.append(buf.copy())
            rets.append(r)
        res = next((r for r in rets if r < 0), rets[0])
        if res < 0:
            return None, res
        assert all(r == res for r in rets), rets
        return mapping_apply(self.layout, outs, res), res
