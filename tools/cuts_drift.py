#!/usr/bin/env python3
"""How far a cut lies from the slice of the continuous decode, per mode and pre-roll (include/opusgpu.h WHOLE FILES / CUTS; DESIGN
13j).  CPU only, oracle only: files of one mode each (CELT-only, SILK-only, hybrid; stereo, 20 ms packets of random payload, as the
tests' corpora are made), decoded whole by the oracle and as cuts by the model of the device path on the oracle (tests/files_util.py:
model_decode), whose decoder starts from reset state at the cut's first packet.  For pre-rolls of 0, 20, 40, 80 and 160 ms and
--starts cut starts per file: the largest |cut - slice| over the cuts, how many cuts agree with the slice exactly from some sample
on, and the latest such sample.  Information for choosing `preroll`, not a test threshold: nothing asserts these figures.
usage: python3 tools/cuts_drift.py [--packets P] [--starts N] [--seconds S]"""
import argparse
import importlib.util
import os
import sys

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(here, "..", "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=200, help="packets of 20 ms per file")
ap.add_argument("--starts", type=int, default=12, help="cuts per file and pre-roll")
ap.add_argument("--seconds", type=float, default=2.0, help="length of a cut")
ap.add_argument("--channels", type=int, default=2)
args = ap.parse_args()

spec = importlib.util.spec_from_file_location("esp32_opus_player_amd", os.path.join(here, "..", "esp32-opus-player_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pkg)
import files_util as fu  # noqa: E402
import oracle_py  # noqa: E402

oracle = oracle_py.load()
rng = np.random.default_rng(2)
silk, hyb, celt = fu.TOCS20[args.channels]
modes = [("CELT", celt, 100), ("SILK", silk, 35), ("hybrid", hyb, 90)]
files = [fu.opus_file([[fu.packet(rng, toc, n) for _ in range(5)] for _ in range(args.packets // 5)], args.channels, 312)[0] for _, toc, n in modes]
whole = pkg.FileBatch(files, channels=args.channels)
tracks = fu.model_decode(pkg, oracle, whole)[0]
count = int(args.seconds * 48000)
prerolls = [0, 960, 1920, 3840, 7680]
print("| mode | pre-roll | lead got | largest abs(cut - slice) | cuts equal from some sample on | latest such sample |")
print("|---|---|---|---|---|---|")
for i, (name, _, _) in enumerate(modes):
    length = int(whole.info["track_samples"][i])
    starts = [int(s) for s in rng.integers(8000, length - count, args.starts)]  # (behind the first 160 ms: no cut is exact)
    for pre in prerolls:
        b = pkg.FileBatch(files, channels=args.channels, cuts=[(i, s, count, pre) for s in starts])
        assert not b.cut_info["exact"].any()
        got = fu.model_decode(pkg, oracle, b)[0]
        worst, agree, latest = 0, 0, 0
        for s, g in zip(starts, got):
            d = np.abs(g.astype(np.int64) - tracks[i][s:s + count].astype(np.int64)).max(axis=1)
            worst = max(worst, int(d.max()))
            bad = np.nonzero(d)[0]
            if not len(bad) or bad[-1] < count - 960:  # equal over at least the last frame of the cut
                agree += 1
                latest = max(latest, int(bad[-1]) + 1 if len(bad) else 0)
        lead = b.cut_info["lead"]
        print(f"| {name} | {pre} ({pre / 48:.0f} ms) | {int(lead.min())} - {int(lead.max())} | {worst} | {agree} of {len(starts)} | "
              f"{latest if agree else '-'} |")
        b.close()
whole.close()
