"""Batches for the parse kernel's allocation scratch (tests/test_parse_alloc_layout_emul.py, tests/test_gpu_parse_layout.py): stereo
CELT fullband payloads of 20, 40, 80, 160 and 400 bytes, and their oracle PCM.  LCG payloads, which reach a dynalloc boost in a
quarter of the frames and a band boosted three times or more in a tenth -- and two directed kinds for what random bytes never reach:
  * a boost stopped by the band's cap takes 23 or more `1` flags in a row: one 160-byte payload that has them
    (tests/golden/parse_alloc_directed.json), in two frames of the last stream of the 160-byte batch;
  * a frame whose budget went negative is a silent one (the silence flag spends every bit of the frame, and the allocation starts
    from -1): four 0xFF bytes in front, in two frames of the last stream but one of every batch.
The header's symbols are decoded without reference to the stream's state, so a directed frame does the same in any frame of any stream."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOC = 0xFC
SIZES = (20, 40, 80, 160, 400)


def _pkg():
    from conftest import load_pkg
    return load_pkg()


@functools.lru_cache(maxsize=None)
def reference(L, n, frames):
    """-> payloads uint8 [frames, n, L], oracle PCM int16 [n, frames, 960, 2].  Computed once, read-only."""
    import oracle_py
    oracle, pkg = oracle_py.load(), _pkg()
    pay = pkg.lcg_payloads(n, frames, L, seed_base=0xA110C000 + L).copy()
    pay[2:4, n - 2, :4] = 0xFF
    if L == 160:
        cap = json.load(open(os.path.join(ROOT, "tests", "golden", "parse_alloc_directed.json")))["cap_stop_160"]
        pay[0, n - 1] = pay[frames - 1, n - 1] = np.frombuffer(bytes.fromhex(cap), dtype=np.uint8)
    pcm, ok = oracle.batch_decode_threads(2, TOC, pay)
    assert ok == n * frames, (L, ok)
    pcm = np.ascontiguousarray(pcm).reshape(n, frames, 960, 2)
    pay.setflags(write=False)
    pcm.setflags(write=False)
    return pay, pcm
