"""The parse kernels' LDS layout on the GPU against the oracle: a band's dynalloc boost rests as a count in the band's fine_quant
byte (LaneArr::boost, og_celt_parse.hpp), and a 64-frame parse wave's rows are 8,064 bytes apart, the tables behind the second
wave's (og_parse64.hip).  What only the GPU can show: the two waves of a k_celt_parse64 workgroup must not share rows, and the
rows must not reach into the tables.  The batches of tests/parse_alloc_batches.py (stereo CELT fullband payloads of 20, 40, 80, 160
and 400 bytes with the directed frames: a boost stopped by its cap, silent frames) at 165 streams -- one full 128-frame workgroup of
k_celt_parse64 and a ragged second one, five full and a ragged workgroup of the 32-frame k_celt_parse -- six frames, in order
(k_celt_parse) and as ONE queued pipelined window (k_celt_parse64); and 32 hybrid fullband streams (TOC 0x7C, 120 bytes), whose
CELT layer starts at band 17: the bands below keep a zero count.  EVERY step's PCM and result codes are compared.  The bar is equality."""
import functools

import numpy as np
import pytest

from parse_alloc_batches import SIZES, TOC, reference
from test_gpu_pipeline import run_queued

STREAMS, FRAMES = 165, 6
HYBRID = (32, 0x7C, 120)


def _pkg():
    from conftest import load_pkg
    return load_pkg()


@functools.lru_cache(maxsize=None)
def _hybrid_reference():
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    n, toc, L = HYBRID
    pay = pkg.lcg_payloads(n, FRAMES, L, seed_base=0xA110B000)
    pcm, ok = oracle.batch_decode_threads(2, toc, pay)
    assert ok == n * FRAMES, ok
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
        pay, ref = reference(L, STREAMS, FRAMES)
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
