"""A range ENCODER for tests: the inverse of oracle/oc_range.c, in plain Python, plus frame writers that pin the leading symbols
of a CELT or SILK frame and leave the rest to noise.  TEST INFRASTRUCTURE ONLY (tests/, tests/golden/make_rare_paths.py,
tools/oracle_branches.py).

The coder is the textbook carry-propagating encoder that pairs with the decoder of RFC 6716 section 4.1: 32-bit range, 8-bit output
symbols, raw bits written backwards from the packet's end.  `done(nbytes, fill=...)` closes the coded prefix with the fewest bits that
pin it and puts caller-supplied bytes behind them, so that a frame reads as "these first K symbols, then noise": whatever follows the
closing bits leaves the decoder's value inside the last symbol's interval, so every pinned symbol still comes back.

Every symbol method mirrors one oc_rc_* function:
    encode(fl, fh, ft)   <-> oc_rc_decode(ft) + oc_rc_update(fl, fh, ft)
    encode_bin(fl, fh, b)<-> oc_rc_decode_bin(b) + oc_rc_update(fl, fh, 1 << b)
    bit_logp(v, logp)    <-> oc_rc_bit_logp(logp)
    icdf(s, table, ftb)  <-> oc_rc_icdf(table, ftb)
    uint(v, ft)          <-> oc_rc_uint(ft)
    bits(v, n)           <-> oc_rc_bits(n)
    laplace(v, fs, decay)<-> oc_rc_laplace(fs, decay)
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYM_BITS, CODE_BITS, SYM_MAX = 8, 32, 255
CODE_TOP = 1 << 31
CODE_BOT = CODE_TOP >> SYM_BITS
CODE_SHIFT = CODE_BITS - SYM_BITS - 1


class CraftError(ValueError):
    """The symbols do not fit the requested packet size (or a symbol has probability zero)."""


class Encoder:
    def __init__(self):
        self.low, self.rng, self.rem, self.ext = 0, CODE_TOP, -1, 0
        self.out = bytearray()        # range-coded bytes, from the front
        self.end = bytearray()        # raw-bit bytes, from the back (end[0] is the packet's last byte)
        self.end_window, self.nend_bits = 0, 0
        self.nbits_total = CODE_BITS + 1

    # ---- the coder -------------------------------------------------------------------------------------------------------------
    def _carry_out(self, c):
        if c != SYM_MAX:
            carry = c >> SYM_BITS
            if self.rem >= 0:
                self.out.append((self.rem + carry) & SYM_MAX)
            if self.ext > 0:
                self.out.extend([(SYM_MAX + carry) & SYM_MAX] * self.ext)
                self.ext = 0
            self.rem = c & SYM_MAX
        else:
            self.ext += 1

    def _normalize(self):
        while self.rng <= CODE_BOT:
            self._carry_out(self.low >> CODE_SHIFT)
            self.low = (self.low << SYM_BITS) & (CODE_TOP - 1)
            self.rng <<= SYM_BITS
            self.nbits_total += SYM_BITS

    def _narrow(self, r, fl, fh, ft):
        if not 0 <= fl < fh <= ft:
            raise CraftError(f"symbol with no probability: [{fl}, {fh}) of {ft}")
        if fl > 0:
            self.low += self.rng - r * (ft - fl)
            self.rng = r * (fh - fl)
        else:
            self.rng -= r * (ft - fh)
        self._normalize()

    def encode(self, fl, fh, ft):
        self._narrow(self.rng // ft, fl, fh, ft)

    def encode_bin(self, fl, fh, bits):
        self._narrow(self.rng >> bits, fl, fh, 1 << bits)

    def bit_logp(self, val, logp):
        s = self.rng >> logp
        r = self.rng - s
        if val:
            self.low += r
        self.rng = s if val else r
        self._normalize()

    def icdf(self, s, icdf, ftb=8):
        ft = 1 << ftb
        fl = ft - (icdf[s - 1] if s > 0 else ft)
        self._narrow(self.rng >> ftb, fl, ft - icdf[s], ft)

    def uint(self, val, ft):
        if not 0 <= val < ft:
            raise CraftError(f"{val} is no value below {ft}")
        ft -= 1
        ftb = ft.bit_length()
        if ftb > 8:
            ftb -= 8
            self.encode(val >> ftb, (val >> ftb) + 1, (ft >> ftb) + 1)
            self.bits(val & ((1 << ftb) - 1), ftb)
        else:
            self.encode(val, val + 1, ft + 1)

    def bits(self, val, n):
        """n raw bits (n <= 25), written from the packet's end"""
        if not 0 <= val < (1 << n):
            raise CraftError(f"{val} does not fit {n} bits")
        self.end_window |= val << self.nend_bits
        self.nend_bits += n
        while self.nend_bits >= SYM_BITS:
            self.end.append(self.end_window & SYM_MAX)
            self.end_window >>= SYM_BITS
            self.nend_bits -= SYM_BITS
        self.nbits_total += n

    def laplace(self, val, fs, decay):
        """oc_rc_laplace's inverse (fs: probability of 0 in Q15, decay in Q14).  Values past the modelled tail cannot be coded."""
        fl, v = 0, abs(val)
        if val:
            s = -1 if val < 0 else 0
            fl = fs
            fs = ((32768 - 32 - fs) * (16384 - decay) >> 15)
            i = 1
            while fs > 0 and i < v:
                fs *= 2
                fl += fs + 2
                fs = (fs * decay) >> 15
                i += 1
            if fs == 0:
                ndi_max = (32768 - fl - s) >> 1  # how many values of probability 1 / 32768 are left on this side
                di = v - i
                if di > ndi_max - 1:
                    raise CraftError(f"Laplace value {val} is past the model's tail")
                fl += 2 * di + 1 + s
                fs = min(1, 32768 - fl)
            else:
                fs += 1
                fl += fs & ~s
        self.encode_bin(fl, min(fl + fs, 32768), 15)

    def tell(self):
        return self.nbits_total - self.rng.bit_length()

    # ---- closing the packet ---------------------------------------------------------------------------------------------------
    def done(self, nbytes, fill=None):
        """The packet: exactly `nbytes` bytes.  Behind the bits that close the range-coded prefix, and before the raw bits at the
        end, come the bytes of `fill` (an iterable of ints, cycled if short; zeros if None).  Raises CraftError if the prefix and
        the raw bits do not fit.  The coder stays usable: more symbols may follow and done() may be called again."""
        saved = (self.low, self.rng, self.rem, self.ext, bytearray(self.out))
        l = CODE_BITS - self.rng.bit_length()
        msk = (CODE_TOP - 1) >> l
        end = (self.low + msk) & ~msk
        if (end | msk) >= self.low + self.rng:
            l += 1
            msk >>= 1
            end = (self.low + msk) & ~msk
        while l > 0:
            self._carry_out(end >> CODE_SHIFT)
            end = (end << SYM_BITS) & (CODE_TOP - 1)
            l -= SYM_BITS
        if self.rem >= 0 or self.ext > 0:
            self._carry_out(0)
        front = self.out
        self.low, self.rng, self.rem, self.ext, self.out = saved
        free_low_bits = -l if front else 0  # of front's last byte: the closing bits sit in its high end
        back = bytearray(self.end)          # back[0] is the packet's last byte
        if self.nend_bits:
            back.append(self.end_window & ((1 << self.nend_bits) - 1))
        if len(front) + len(back) == nbytes + 1 and 0 < self.nend_bits <= free_low_bits:
            front[-1] |= back.pop()         # the closing bits and the last raw bits share a byte
        elif len(front) + len(back) > nbytes:
            raise CraftError(f"{len(front)} coded + {len(back)} raw bytes do not fit {nbytes}")
        gap = nbytes - len(front) - len(back)
        src = [v & 0xFF for v in fill] if fill is not None else []
        src = src or [0]
        mid = bytearray(src[i % len(src)] for i in range(gap))
        return bytes(front + mid + back[::-1])


# ---- ROM tables, read from the generated header (data, not restated here) ----------------------------------------------------------
_ROM = {}


def rom(name):
    """integer array `name` of oracle/rom_tables.h"""
    if not _ROM:
        text = open(os.path.join(ROOT, "oracle", "rom_tables.h")).read()
        for m in re.finditer(r"\b(rom_\w+)\s*\[[^\]]*\]\s*=\s*\{([^}]*)\}", text):
            _ROM[m.group(1)] = [int(v, 0) for v in re.findall(r"-?(?:0x[0-9a-fA-F]+|\d+)", m.group(2))]
    return _ROM[name]


# ---- CELT frame writer (oracle/oc_celt.c oc_celt_decode, 20 ms frames: LM = 3) -------------------------------------------------------
TAPSET_ICDF = [2, 1, 0]
SMALL_ENERGY_ICDF = [2, 1, 0]


def celt_frame(nbytes, channels=2, *, silence=0, postfilter=None, transient=0, intra=0, coarse=None, fill=None, LM=3):
    """A CELT frame of `nbytes` bytes (payload only: prepend the TOC) whose leading symbols are pinned (LM 3: a 20 ms frame, the only
    size reference mode decodes; LM 0..2: the 2.5 / 5 / 10 ms frames of RFC mode, whose TOC names that duration):
    the silence flag; postfilter = None (flag 0) or (octave, period_low_bits, gain_index, tapset); transient; intra;
    coarse = list over bands from 0 of the Laplace value qi, or of one qi per channel (bands not listed are left to the
    fill, as is everything after the coarse energies).
    The writer follows the decoder's budget checks; a symbol the decoder would not read at that point raises CraftError."""
    e = Encoder()
    celt_symbols(e, nbytes * 8, channels, silence, postfilter, transient, intra, coarse, LM)
    return e.done(nbytes, fill)


def celt_symbols(e, total, C, silence=0, postfilter=None, transient=0, intra=0, coarse=None, LM=3):
    """the symbols of celt_frame on encoder e (a CELT-only frame of 120 << LM samples, bands from 0)"""
    NB = 21
    if e.tell() >= total:
        return
    if e.tell() == 1:
        e.bit_logp(silence, 15)
    elif silence:
        raise CraftError("the silence flag is only read at the very start of a packet")
    if silence:
        return
    if e.tell() + 16 <= total:
        e.bit_logp(1 if postfilter else 0, 1)
        if postfilter:
            octave, low, qg, tapset = postfilter
            e.uint(octave, 6)
            e.bits(low, 4 + octave)
            e.bits(qg, 3)
            if e.tell() + 2 <= total:
                e.icdf(tapset, TAPSET_ICDF, 2)
            elif tapset:
                raise CraftError("no bits left for the tapset")
    elif postfilter:
        raise CraftError("no post-filter symbols here")
    if LM > 0 and e.tell() + 3 <= total:
        e.bit_logp(transient, 3)
    elif transient:
        raise CraftError("no transient flag here (LM 0, or no bits left)")
    if e.tell() + 3 <= total:
        e.bit_logp(intra, 3)
    elif intra:
        raise CraftError("no bits left for the intra flag")
    pm = rom("rom_eprob")[(LM * 2 + intra) * 42:][:42]
    for i in range(min(NB, len(coarse or ()))):
        for c in range(C):
            qi = coarse[i]
            qi = qi[c] if isinstance(qi, (list, tuple)) else qi
            left = total - e.tell()
            if left >= 15:
                pi = 2 * min(i, 20)
                e.laplace(qi, pm[pi] << 7, pm[pi + 1] << 6)
            elif left >= 2:
                if qi not in (0, -1, 1):
                    raise CraftError("only 0, -1, 1 fit here")
                e.icdf(2 * qi if qi >= 0 else 1, SMALL_ENERGY_ICDF, 2)
            elif left >= 1:
                if qi not in (0, -1):
                    raise CraftError("only 0, -1 fit here")
                e.bit_logp(-qi, 1)
            elif qi != -1:
                raise CraftError("no bits left: the decoder takes -1")


# ---- SILK frame writer (oracle/oc_silk.c oc_silk_decode_ex, decode_indices; 20 ms frames: four subframes) ------------------------
def silk_frame(nbytes, channels=1, fs_khz=8, *, chans, stereo_pred=None, mid_only=None, pulses=None, fill=None):
    """A SILK frame (the payload of a SILK-only packet, or the SILK part of a hybrid one) whose side information is pinned, as
    reference mode reads it: one 20 ms frame per packet, independently coded (oracle/oc_silk.c: condCoding 0).
    chans: one dict per channel of the packet with vad (0/1) and, for the channel that is coded,
        type (0..1 without VAD: signalType * 2 + offset; 2..5 with), gains = [absolute index 0..63, delta, delta, delta] (delta
        symbols 0..40), nlsf1 (stage-1 index 0..31), nlsf_res (order values in -10..10), interp (0..4),
        and for voiced frames (signalType 2): lag = (high, low), contour, per, ltp = [4 indices], ltp_scale; then seed (0..3).
    Stereo: stereo_pred = (joint n 0..24, [ix00, ix01], [ix10, ix11]); the side channel can be pinned only as absent (vad 0 and
    mid_only 1): a coded side would need the mid channel's excitation written in full.
    pulses = None (noise) or {"rate_level": r, "blocks": [symbol lists]}: see silk_pulse_prefix.
    Everything after the last pinned symbol is `fill`."""
    e = Encoder()
    for ch in chans:
        e.bit_logp(ch["vad"], 1)
        e.bit_logp(0, 1)  # no LBRR frame (those are RFC mode's)
    if channels == 2:
        if chans[1]["vad"] or not mid_only:
            raise CraftError("the side channel can only be written as absent")
        n, a, b = stereo_pred
        e.icdf(n, rom("rom_silk_stereo_joint_icdf"))
        for ix in (a, b):
            e.icdf(ix[0], rom("rom_silk_uniform3_icdf"))
            e.icdf(ix[1], rom("rom_silk_uniform5_icdf"))
        e.icdf(1, rom("rom_silk_mid_only_icdf"))
    _silk_indices(e, chans[0], fs_khz, fs_khz == 16)
    if pulses is not None:
        silk_pulse_prefix(e, chans[0]["type"] >> 1, pulses)
    return e.done(nbytes, fill)


def _silk_indices(e, ch, fs_khz, wb):
    order = 16 if wb else 10
    t = ch["type"]
    if ch["vad"]:
        if t < 2:
            raise CraftError("a frame with VAD set has type 2..5")
        e.icdf(t - 2, rom("rom_silk_type_vad_icdf"))
    else:
        if t > 1:
            raise CraftError("a frame without VAD has type 0..1")
        e.icdf(t, rom("rom_silk_type_novad_icdf"))
    sig = t >> 1
    g = ch["gains"]
    e.icdf(g[0] >> 3, rom("rom_silk_gain_icdf")[8 * sig:])
    e.icdf(g[0] & 7, rom("rom_silk_uniform8_icdf"))
    for d in g[1:4]:
        e.icdf(d, rom("rom_silk_delta_gain_icdf"))
    pre = "rom_silk_wb_" if wb else "rom_silk_nb_"
    e.icdf(ch["nlsf1"], rom(pre + "cb1_icdf")[(sig >> 1) * 32:])
    sel = rom(pre + "cb2_select")[ch["nlsf1"] * order // 2:]
    ec = rom(pre + "cb2_icdf")
    ext = rom("rom_silk_nlsf_ext_icdf")
    for i in range(order):
        entry = sel[i // 2]
        ix = 9 * (((entry >> 1) & 7) if i % 2 == 0 else ((entry >> 5) & 7))
        r = ch["nlsf_res"][i]
        if not -10 <= r <= 10:
            raise CraftError("NLSF residual outside -10..10")
        s = max(-4, min(4, r)) + 4
        e.icdf(s, ec[ix:])
        if s == 0:
            e.icdf(-4 - r, ext)
        elif s == 8:
            e.icdf(r - 4, ext)
    e.icdf(ch.get("interp", 4), rom("rom_silk_nlsf_interp_icdf"))
    if sig == 2:
        lag = ch["lag"]
        e.icdf(lag[0], rom("rom_silk_pitch_lag_icdf"))
        e.icdf(lag[1], rom({16: "rom_silk_uniform8_icdf", 12: "rom_silk_uniform6_icdf", 8: "rom_silk_uniform4_icdf"}[fs_khz]))
        e.icdf(ch["contour"], rom("rom_silk_pitch_contour_nb_icdf" if fs_khz == 8 else "rom_silk_pitch_contour_icdf"))
        e.icdf(ch["per"], rom("rom_silk_ltp_per_icdf"))
        for ix in ch["ltp"]:
            e.icdf(ix, rom("rom_silk_ltp_gain_icdf%d" % ch["per"]))
        e.icdf(ch.get("ltp_scale", 0), rom("rom_silk_ltpscale_icdf"))
    e.icdf(ch.get("seed", 0), rom("rom_silk_uniform4_icdf"))


def silk_pulse_prefix(e, sig, pulses):
    """The head of decode_pulses: the rate level, then for each listed block its pulse-count symbols: a list whose every entry but
    the last is 17 (one more LSB shift).  Blocks not listed, and the shells, LSBs and signs, are left to noise."""
    r = pulses["rate_level"]
    e.icdf(r, rom("rom_silk_rate_levels_icdf")[9 * (sig >> 1):])
    ppb = rom("rom_silk_pulses_per_block_icdf")
    for blk in pulses["blocks"]:
        for n, s in enumerate(blk):
            if (s == 17) != (n < len(blk) - 1):
                raise CraftError("a block's symbols are 17, ..., 17, last < 17")
            e.icdf(s, ppb[18 * r:] if n == 0 else ppb[18 * 9 + (1 if n == 10 else 0):])
