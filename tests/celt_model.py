"""A float64 model of the back half of CELT, written from the mathematics of RFC 6716 sections 4.3.6 to 4.3.8 -- NOT from
oracle/oc_celt.c or the kernel headers, and importing neither: an arbiter that shares no code and no reading with them.

It takes what the front half of the decoder hands over -- the normalised spectrum X (Q14), the band energies E (log2 units, Q10), the
frame's size, block layout, band range and post-filter parameters -- and produces the synthesis signal and the PCM:

    denormalise   freq[i] = X[i] * 2^(E[band] + eMeans[band])  over the coded bands, zero elsewhere
    inverse MDCT  y[n] = sum_k freq[k] cos(pi / N (n + 1/2 + N/2)(k + 1/2)),  n = 0 .. 2N - 1, no further scaling; the low-overlap window
                  w(n) = sin(pi/2 sin^2(pi (n + 1/2) / 240)) over the 120 samples at each end of the part that is not zero, and
                  overlap-add with the tail of the frame before.  A transient frame is 2^LM transforms of 120 coefficients, block b
                  owning coefficients b, b + 2^LM, b + 2 * 2^LM, ...
    post-filter   y[n] = x[n] + g * sum_k tap_k (y[n - T - k] + y[n - T + k]), recursive over its own output; over the first 120
                  samples of a span the old parameter set fades out with 1 - w^2 while the new one fades in with w^2.  The first 120
                  samples of a frame go from the set before the last to the last one, the rest of the frame from the last one to the
                  frame's own; a 2.5 ms frame has no rest, and its own set waits for the next frame (section 4.3.7.1).
    de-emphasis   1 / (1 - 0.85000610 z^-1), rounded to the nearest integer and saturated to 16 bits

The signal is in units of one PCM step (the fixed-point decoders carry it in Q12: divide their taps by 4096).

Two things here are not in the RFC's formulas and are stated so that nobody takes them for mathematics:
  * SIG_SAT: the fixed-point decoders bound the synthesis signal at +-300,000,000 / 4096 after the transform and after every comb
    filter output.  The model clips at the same level so that its state stays comparable after a frame that gets there; the tests
    leave such frames out of the comparison all the same.
  * QUIRK_PARTIAL_RESET: see reset().

`slip=` applies ONE deliberate mistake (SLIPS); tests/test_celt_model.py uses them to show that its tolerance tells a decoder that is
right from one that is subtly wrong.  A model with a slip is wrong on purpose and checks nothing.
"""
import numpy as np

import rc_craft

OVERLAP = 120
HIST = 1024            # the comb filter reaches y[n - T - 2] with T <= 1022
MIN_PERIOD = 15
NBANDS = 21
DEEMPH = 0.85000610
SIG_SAT = 300000000 / 4096.0
TAPSETS = ((0.3066406250, 0.2170410156, 0.1296386719), (0.4638671875, 0.2680664062, 0.0), (0.7998046875, 0.1000976562, 0.0))

SLIPS = ("ola_shift", "anchor", "deinterleave", "xfade_unsquared", "period_plus", "period_minus", "tapset_swap", "pf_swap", "emeans",
         "deemph")
EMEANS_SLIP_BAND_FROM_START = 1   # slip "emeans": the band (start + 1) goes without its mean

# Reference mode only.  The reference's OPUS_RESET_STATE of the CELT decoder clears the post-filter parameters and the energy
# histories but leaves the synthesis history, the overlap tail and the de-emphasis memory standing (SURVEY.md appendix A, Q5:
# src/celt.cpp:2479-2498), and its packet layer issues that reset when the mode changes (src/opus_decoder.cpp:255-256).
# reset(partial=True) models exactly that; a reset as RFC 6716 means it clears everything.
QUIRK_PARTIAL_RESET = True


def window():
    n = np.arange(OVERLAP) + 0.5
    return np.sin(0.5 * np.pi * np.sin(np.pi * n / (2 * OVERLAP)) ** 2)


_W = window()
_checked = []


def _self_check():
    """the window of the formula against the ROM table (Q15), once: within one LSB of that table's format"""
    if not _checked:
        rom = np.array(rc_craft.rom("rom_win120"), dtype=np.float64) / 32768.0
        assert rom.shape == (OVERLAP,) and np.abs(rom - _W).max() <= 1.0 / 32768.0, np.abs(rom - _W).max()
        _checked.append(True)


_BASIS = {}


def _imdct_basis(n):
    """rows (n - 120) / 2 .. (n - 120) / 2 + n + 120 of the 2n x n cosine matrix: the part of the output the window leaves standing,
    with the window on its first and last 120 rows"""
    if n not in _BASIS:
        first = (n - OVERLAP) // 2
        t = np.arange(first, first + n + OVERLAP, dtype=np.float64)[:, None]
        k = np.arange(n, dtype=np.float64)[None, :]
        m = np.cos(np.pi / n * (t + 0.5 + n / 2.0) * (k + 0.5))
        m[:OVERLAP] *= _W[:, None]
        m[n:] *= _W[::-1, None]
        _BASIS[n] = m
    return _BASIS[n]


class CeltModel:
    def __init__(self, channels, slip=None):
        assert channels in (1, 2) and (slip is None or slip in SLIPS), (channels, slip)
        _self_check()
        self.channels, self.slip = channels, slip
        self.eband = np.array(rc_craft.rom("rom_eband"), dtype=np.int64)
        self.emeans = np.array(rc_craft.rom("rom_emeans")[:NBANDS], dtype=np.float64) / 16.0   # Q4
        self.reset()

    def reset(self, partial=False):
        """A stream starts from zeros.  partial: QUIRK_PARTIAL_RESET, what the reference's mode switch does instead."""
        zero_pf = (0, 0.0, 0)
        self.pf_old, self.pf_cur = zero_pf, zero_pf
        if partial and QUIRK_PARTIAL_RESET:
            return
        cc = self.channels
        self.tail = np.zeros((cc, OVERLAP))
        self.hist = np.zeros((cc, HIST))
        self.mem = np.zeros(cc)
        self.prev_lm = None
        self.last_peak = 0.0

    # ---- the four steps -------------------------------------------------------------------------------------------------------------
    def _denormalise(self, x_q14, e_q10, lm, start, end):
        m = 1 << lm
        freq = np.zeros(OVERLAP << lm)
        for b in range(start, end):
            mean = self.emeans[b]
            if self.slip == "emeans" and b == start + EMEANS_SLIP_BAND_FROM_START:
                mean = 0.0
            lo, hi = m * self.eband[b], m * self.eband[b + 1]
            freq[lo:hi] = (x_q14[lo:hi] / 16384.0) * 2.0 ** (e_q10[b] / 1024.0 + mean)
        return freq

    def _imdct(self, freq, lm, transient, tail):
        n = OVERLAP << lm
        acc = np.zeros(n + OVERLAP + 1)
        at = 1 if self.slip == "ola_shift" else 0
        acc[at:at + OVERLAP] += tail
        if transient:
            m = 1 << lm
            for b in range(m):
                coef = freq[b * OVERLAP:(b + 1) * OVERLAP] if self.slip == "deinterleave" else freq[b::m]
                acc[b * OVERLAP:b * OVERLAP + 2 * OVERLAP] += _imdct_basis(OVERLAP) @ coef
        else:
            acc[:n + OVERLAP] += _imdct_basis(n) @ freq
        return np.clip(acc[:n], -SIG_SAT, SIG_SAT), acc[n:n + OVERLAP].copy()

    def _comb(self, h, at, count, old, new):
        """h[at : at + count) in place; old / new = (period, gain, tapset); the cross-fade runs over the first 120 samples"""
        if self.slip == "pf_swap":
            old, new = new, old
        (t0, g0, s0), (t1, g1, s1) = old, new
        if g0 == 0.0 and g1 == 0.0:
            return
        shift = {"period_plus": 1, "period_minus": -1}.get(self.slip, 0)
        t0, t1 = max(t0, MIN_PERIOD) + shift, max(t1, MIN_PERIOD) + shift
        if self.slip == "tapset_swap":
            s0, s1 = (1, 0, 2)[s0], (1, 0, 2)[s1]
        fade = np.ones(count)
        k = min(count, OVERLAP)
        fade[:k] = _W[:k] if self.slip == "xfade_unsquared" else _W[:k] ** 2
        a0, a1 = (1.0 - fade) * g0, fade * g1
        step = min(t0, t1) - 2   # what a chunk reads lies before the chunk
        for p in range(0, count, step):
            i = np.arange(at + p, at + min(p + step, count))
            w0, w1 = a0[i - at], a1[i - at]
            y = h[i]
            for (t, w, taps) in ((t0, w0, TAPSETS[s0]), (t1, w1, TAPSETS[s1])):
                y = y + w * (taps[0] * h[i - t] + taps[1] * (h[i - t - 1] + h[i - t + 1]) + taps[2] * (h[i - t - 2] + h[i - t + 2]))
            h[i] = np.clip(y, -SIG_SAT, SIG_SAT)

    def _deemphasis(self, x, c):
        coef = 0.8 if self.slip == "deemph" else DEEMPH
        y, m = np.empty(len(x)), self.mem[c]
        for j, v in enumerate(x.tolist()):
            m = v + coef * m
            y[j] = m
        self.mem[c] = m
        return y

    # ---- one frame ------------------------------------------------------------------------------------------------------------------
    def frame(self, X, E, lm, transient, start, end, postfilter=None, silence=False):
        """X: int16 [C][120 << lm] in Q14, E: int16 [C][21] in Q10, C = the channels the frame codes (1 or 2);
        postfilter = None or (period, gain in Q15, tapset) as the frame codes it.
        -> (synthesis after the post-filter float64 [channels][N], pcm int16 [N][channels])"""
        X, E = np.asarray(X, dtype=np.float64), np.asarray(E, dtype=np.float64)
        C, cc, n = X.shape[0], self.channels, OVERLAP << lm
        assert X.shape == (C, n) and E.shape == (C, NBANDS) and 0 <= lm <= 3 and 0 <= start <= end <= NBANDS
        new = (0, 0.0, 0) if postfilter is None else (int(postfilter[0]), postfilter[1] / 32768.0, int(postfilter[2]))
        if silence:
            freqs = [np.zeros(n) for _ in range(C)]
        else:
            freqs = [self._denormalise(X[c], E[c], lm, start, end) for c in range(C)]
        if C == 1 and cc == 2:
            freqs = [freqs[0], freqs[0]]          # a mono frame in a stereo decoder: both channels get the one spectrum
        elif C == 2 and cc == 1:
            freqs = [0.5 * (freqs[0] + freqs[1])]  # a stereo frame in a mono decoder: the mean
        syn = np.zeros((cc, n))
        pcm = np.zeros((n, cc), dtype=np.int16)
        peak = 0.0
        for c in range(cc):
            pre, self.tail[c] = self._imdct(freqs[c], lm, transient, self.tail[c])
            hist = self.hist[c]
            if self.slip == "anchor" and self.prev_lm is not None and self.prev_lm != lm:
                hist = np.concatenate([[0.0], hist[:-1]])
            h = np.concatenate([hist, pre])
            peak = max(peak, np.abs(h).max(), np.abs(self.tail[c]).max())
            self._comb(h, HIST, OVERLAP, self.pf_old, self.pf_cur)
            if lm != 0:
                self._comb(h, HIST + OVERLAP, n - OVERLAP, self.pf_cur, new)
            syn[c] = h[HIST:]
            self.hist[c] = h[-HIST:]
            y = self._deemphasis(syn[c], c)
            pcm[:, c] = np.clip(np.floor(y + 0.5), -32768, 32767).astype(np.int16)
        self.pf_old, self.pf_cur = self.pf_cur, new
        if lm != 0:
            self.pf_old = self.pf_cur
        self.prev_lm = lm
        self.last_peak = peak   # the largest magnitude among the frame before the post-filter, the history it reads and the new tail
        return syn, pcm
