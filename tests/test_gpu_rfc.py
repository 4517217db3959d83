"""RFC mode on the GPU (include/opusgpu.h OPUSGPU_MODE_RFC) against the oracle's RFC mode
(oc_decoder_set_rfc -- itself parity-UNPINNED: the reference cannot decode these durations and no libopus exists here):
all 32 TOC configurations x frame-count codes 0..3, mono and stereo packets in mono and stereo decoders, every packet at the
duration its TOC names (2.5 ... 60 ms frames, up to 120 ms per packet), state carried over a sequence of packets with
configuration switches (incl. hybrid -> SILK-only: the silence-frame fade-out).  Through the C ABI (opusgpu_decode_packets)."""
import numpy as np
import pytest

import ctypes as C

import rfc_common as rc
from rfc_common import make_packet

pytestmark = pytest.mark.gpu


def _run(pkg, oracle, ctx, channels, name):
    """The plan `name` of rfc_common.rfc_plan: every stream decodes plan["steps"] packets, one per step (rfc_common.draw_step: lost
    packets are empty and concealed for as long as the stream's last packet was; DTX frames carry 0 or 1 bytes; before some
    packets the packet before is recovered from the packet's forward error correction data with decode_packets_fec, after
    which the packet is decoded normally).  Every stream against its own oracle decoder in RFC mode (rfc_common.oracle_step /
    same_step, oracle_fec_step / same_fec_step).  -> packets compared."""
    plan = rc.rfc_plan(name)
    rng = np.random.default_rng(plan["seed"] + channels)
    n, steps = plan["streams"], plan["steps"]
    ctx.set_mode(True)
    try:
        ctx.streams_alloc(n, channels)
        decs = []
        for s in range(n):
            d = oracle.decoder(channels)
            d.init()
            d.set_rfc(True)
            decs.append(d)
        last = [None] * n  # (frame count, frame duration, packet channels, mode) of the stream's last packet that framed
        checked = 0
        for f in range(steps):
            pk, who = rc.draw_step(oracle, plan, rng, f, channels)
            if who:  # the packet before pk[s] was lost: recover it from pk[s]
                pcm, res = ctx.decode_packets_fec(np.array(who), [pk[s] for s in who], frame_capacity=6)
                for j, s in enumerate(who):
                    ref, r, spans, before = rc.oracle_fec_step(oracle, decs[s], pk[s], last[s], channels)
                    bad = rc.same_fec_step(pcm[j], res[j], ref, r, spans, before, channels)
                    assert bad is None, (f, s, hex(pk[s][0]), bad)
                    checked += r > 0
            pcm, res = ctx.decode_packets(np.arange(n), pk, frame_capacity=6)
            for s in range(n):
                ref, r, domain, last[s] = rc.oracle_step(oracle, decs[s], pk[s], last[s], channels)
                bad = rc.same_step(pcm[s], res[s], ref, r, domain, channels)
                assert bad is None, (f, s, "lost" if not pk[s] else hex(pk[s][0]), bad)
                checked += r > 0
        return checked
    finally:
        ctx.set_mode(False)


@pytest.mark.parametrize("channels", [2, 1])
def test_rfc_all_configs_and_codes(pkg, oracle, gpu_ctx, channels):
    """stream s decodes configuration s % 32 with frame-count code (s // 32) % 4, four packets in a row"""
    assert _run(pkg, oracle, gpu_ctx, channels, "all_configs") > 256 * 3


@pytest.mark.parametrize("channels", [2, 1])
def test_rfc_configuration_switches(pkg, oracle, gpu_ctx, channels):
    """every stream walks its own random sequence of configurations and codes (mode, bandwidth and duration switches,
    hybrid -> SILK-only among them); redundant CELT frames (RFC 6716 section 4.5.1): SILK-only frames with random payloads
    carry one almost always, hybrid packets with the flag set are mixed in from tests/golden/rfc_hybrid_redundancy_seeds.json"""
    assert _run(pkg, oracle, gpu_ctx, channels, "switches") > 384 * 5


@pytest.mark.parametrize("channels", [2, 1])
def test_rfc_loss_path(pkg, oracle, gpu_ctx, channels):
    """lost packets (len == 0) and DTX frames conceal on the GPU, bit-exact to the oracle's RFC mode -- SILK PLC +
    comfort noise + the glue to the next decoded frame, CELT's noise-based concealment, hybrid both; random configuration
    walks so that losses follow (and are followed by) every mode, bandwidth and frame duration; several losses in a row."""
    assert _run(pkg, oracle, gpu_ctx, channels, "loss") > 512 * 7


@pytest.mark.parametrize("channels", [2, 1])
def test_rfc_forward_error_correction(pkg, oracle, gpu_ctx, channels):
    """opus_decode(decode_fec = 1): a lost packet recovered from the NEXT packet's LBRR frames (SILK-only and hybrid; per channel
    and internal frame a concealment where the packet carries no copy; hybrid's CELT layer concealed), plain concealment
    around CELT-only packets; mixed with ordinary losses and DTX frames"""
    assert _run(pkg, oracle, gpu_ctx, channels, "fec") > 384 * 9


def test_rfc_loss_before_any_packet_and_after_reset(pkg, oracle, gpu_ctx):
    """a loss with nothing decoded yet is 20 ms of zeros; after a stream reset the same"""
    ctx = gpu_ctx
    ctx.set_mode(True)
    try:
        ctx.streams_alloc(4, 2)
        pcm, res = ctx.decode_packets(np.arange(4), [b""] * 4, frame_capacity=6)
        assert (res == 960).all() and not pcm.any()
        rng = np.random.default_rng(9)
        pk = [make_packet(rng, 31, True, 0, 80) for _ in range(4)]
        pcm, res = ctx.decode_packets(np.arange(4), pk, frame_capacity=6)
        assert (res == 960).all() and pcm.any()
        pcm, res = ctx.decode_packets(np.arange(4), [None] * 4, frame_capacity=6)
        assert (res == 960).all() and pcm[:, :960].any()  # concealed from the CELT state
        ctx.streams_reset(0, 4, True)
        pcm, res = ctx.decode_packets(np.arange(4), [b""] * 4, frame_capacity=6)
        assert (res == 960).all() and not pcm.any()
    finally:
        ctx.set_mode(False)


def test_reference_mode_conceals_nothing(pkg, gpu_ctx):
    """Reference mode has no concealment (Q8) -- an empty packet there is NOT a lost packet but what the reference's own
    empty-packet branch makes of it (src/opus_decoder.cpp:290-308; tests/test_empty_packets.py has the known answers): a frame of
    no bytes in the stream's last mode.  Fresh streams are in mode 0: SILK runs, CELT refuses (src/celt.cpp:2225)."""
    ctx = gpu_ctx
    ctx.streams_alloc(2, 2)
    pcm, res = ctx.decode_packets(np.arange(2), [b"", None])
    assert (res == -18).all()  # ERR_OPUS_CELT_BAD_ARG


def test_reference_mode_unchanged_after_rfc(pkg, oracle, gpu_ctx):
    """switching the mode off again gives the reference-exact decode (every frame 960 samples)"""
    ctx = gpu_ctx
    ctx.set_mode(True)
    ctx.set_mode(False)
    n = 64
    ctx.streams_alloc(n, 2)
    pay = pkg.lcg_payloads(n, 2, 60)
    ref, ok = oracle.batch_decode(2, 0xE4, pay)  # CELT FB 2.5 ms TOC: decodes as 20 ms in reference mode (Q6)
    for f in range(2):
        pk = [bytes([0xE4]) + pay[f, s].tobytes() for s in range(n)]
        pcm, res = ctx.decode_packets(np.arange(n), pk)
        assert (res == 960).all()
        assert (pcm == ref[:, f]).all()


@pytest.mark.parametrize("channels", [2, 1])
def test_rfc_celt_loss_bursts_pitch_then_noise(pkg, oracle, gpu_ctx, channels):
    """CELT-only streams of every bandwidth and frame duration (configurations 16 .. 31) losing half of their packets: bursts of one
    to ten lost frames -- the first five of a burst extrapolated from the pitch period (og_plc.hpp: the search and the LPC analysis at
    the burst's first frame, period and filter kept for the rest), the later ones noise at the decaying band energies -- and the
    first decoded frame behind a burst blending into the concealment's overlap tail.  Every sample against the oracle's RFC mode."""
    assert _run(pkg, oracle, gpu_ctx, channels, "celt_bursts") > 640 * 9
