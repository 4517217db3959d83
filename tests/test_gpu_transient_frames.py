"""What only transient frames run in k_celt_recon_fb -- anti-collapse in whole-wave passes (anti_collapse_pm), the eight short
blocks of the inverse MDCT -- on the GPU, against the oracle: the batches of tests/test_anti_collapse_cells.py (3,072 stereo
frames of the bench's payloads with 360 transient frames, 179 of them with anti-collapse; 64 streams x 12 frames each of mono
packets in a mono decoder, mono packets in a stereo decoder and hybrid fullband packets, whose CELT layer starts at band 17),
step by step and as ONE queued window.  EVERY step's PCM and result codes are compared.  That each batch holds every class is
test_anti_collapse_cells.py::test_every_class_occurs (no GPU)."""
import numpy as np
import pytest

from test_anti_collapse_cells import BATCHES, FRAMES, reference
from test_gpu_pipeline import run_queued


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["in_order", "window"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_every_step_matches_the_oracle(pkg, gpu_ctx, name, route):
    n, channels, toc, L, _ = BATCHES[name]
    pay, ref, count = reference(name)
    assert count["transient"] > count["anti_collapse"] > 0
    ref = ref.transpose(1, 0, 2, 3).reshape(FRAMES, n, 960 * channels)
    # packets back to back, frame-major: TOC byte + payload
    pk = np.empty((FRAMES, n, L + 1), dtype=np.uint8)
    pk[:, :, 0] = toc
    pk[:, :, 1:] = pay
    arena = np.concatenate([pk.reshape(-1), np.zeros(16, dtype=np.uint8)])
    offs = (np.arange(FRAMES * n, dtype=np.int64) * (L + 1)).reshape(FRAMES, n)
    lens = np.full((FRAMES, n), L, dtype=np.int64)
    tocs = np.full((FRAMES, n), toc, dtype=np.uint8)
    if route == "in_order":
        pcm, res = run_queued(pkg, gpu_ctx, channels, arena, offs, lens, tocs, pipeline=False)
    else:
        pcm, res = run_queued(pkg, gpu_ctx, channels, arena, offs, lens, tocs, pipeline=True, window=True, modes=pkg.toc_modes(toc))
    assert (res == 960).all(), (name, route, "result codes of (frame, stream)", np.argwhere(res != 960)[:4].tolist())
    bad = (pcm != ref).any(axis=-1)
    assert not bad.any(), (name, route, "PCM of (frame, stream)", np.argwhere(bad)[:8].tolist(), "frames that differ per step",
                           bad.sum(axis=1).tolist())
