"""The fill jobs of k_celt_recon_fb's phase-major band loop on the GPU against the oracle: what the kernel of 20 ms frames does
differently from the emulation there -- the lane's noise-generator pair held for the frame (LcgTab::hold / at_lane), the record's
band_w staged in LDS with the kernel's first round trip (also for the CELT layer of hybrid frames, whose bands below 17 have no
words), the stereo merge's band edges requested ahead.  The batches of tests/test_fill_windows_emul.py (stereo CELT fullband
packets of 20, 40, 80, 160 and 400 LCG bytes, 64 streams x 8 frames each: 15 to 1 fill jobs per frame, counted there) and 32
streams x 8 frames of hybrid fullband packets (TOC 0x7C, 120 bytes: start = 17), step by step and as ONE queued window; EVERY
step's PCM and result codes are compared.  The bar is equality."""
import functools

import numpy as np
import pytest

from test_fill_windows_emul import FRAMES, SIZES, STREAMS, TOC, reference
from test_gpu_pipeline import run_queued

HYBRID = (32, 0x7C, 120)


def _pkg():
    from conftest import load_pkg
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _hybrid_reference():
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    n, toc, L = HYBRID
    pay = pkg.lcg_payloads(n, FRAMES, L, seed_base=0xF111B000)
    pcm = np.zeros((n, FRAMES, 960, 2), dtype=np.int16)
    d = oracle.decoder(2)
    for s in range(n):
        d.init()
        for f in range(FRAMES):
            ref, r = d.decode(bytes([toc]) + pay[f, s].tobytes())
            assert r == 960, (s, f, r)
            pcm[s, f] = ref[:960]
    pay.setflags(write=False)
    pcm.setflags(write=False)
    return pay, pcm


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
@pytest.mark.parametrize("batch", [*SIZES, "hybrid"])
def test_every_step_matches_the_oracle(pkg, gpu_ctx, batch, route):
    if batch == "hybrid":
        n, toc, L = HYBRID
        pay, ref = _hybrid_reference()
    else:
        n, toc, L = STREAMS, TOC, batch
        pay, ref = reference(L)
    ref = ref.transpose(1, 0, 2, 3).reshape(FRAMES, n, 960 * 2)
    pk = np.empty((FRAMES, n, L + 1), dtype=np.uint8)
    pk[:, :, 0] = toc
    pk[:, :, 1:] = pay
    arena = np.concatenate([pk.reshape(-1), np.zeros(16, dtype=np.uint8)])
    offs = (np.arange(FRAMES * n, dtype=np.int64) * (L + 1)).reshape(FRAMES, n)
    lens = np.full((FRAMES, n), L, dtype=np.int64)
    tocs = np.full((FRAMES, n), toc, dtype=np.uint8)
    if route == "in_order":
        pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens, tocs, pipeline=False)
    else:
        pcm, res = run_queued(pkg, gpu_ctx, 2, arena, offs, lens, tocs, pipeline=True, window=True, modes=pkg.toc_modes(toc))
    assert (res == 960).all(), (batch, route, "result codes of (frame, stream)", np.argwhere(res != 960)[:4].tolist())
    bad = (pcm != ref).any(axis=-1)
    assert not bad.any(), (batch, route, "PCM of (frame, stream)", np.argwhere(bad)[:8].tolist(), "frames that differ per step",
                           bad.sum(axis=1).tolist())
