#!/usr/bin/env python3
"""Digests of the feature kernels' outputs, for comparing two builds of the library bit by bit: the crafted tracks of
tests/test_gpu_tracks_mel.py, test_gpu_tracks_melspec.py, test_gpu_tracks_stft.py and test_gpu_tracks_fbank.py -- every set, both
layouts, laid out in guard-filled buffers as those tests lay them out -- through opusgpu_tracks_{mel,melspec,stft,fbank}_device of
whichever library OPUSGPU_LIB names (the tree's own without it), in one process.  One line per (kernel, set, layout): the SHA-256
of the WHOLE output buffer, guard words included.  Two builds compute the same bits exactly when every line is the same.
usage (GPU box): [OPUSGPU_LIB=build_ab/lib_<name>.so] python3 tools/feat_digest.py"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402  (the package loader of the tests)
import test_gpu_tracks_fbank as g_fbank  # noqa: E402
import test_gpu_tracks_mel as g_mel  # noqa: E402
import test_gpu_tracks_melspec as g_spec  # noqa: E402
import test_gpu_tracks_stft as g_stft  # noqa: E402
import test_tracks_fbank as c_fbank  # noqa: E402
import test_tracks_stft as c_stft  # noqa: E402


def main():
    pkg = conftest.load_pkg()
    g_spec._PKG[:] = [pkg]
    c_stft._PKG[:] = [pkg]
    ctx = pkg.Context(0)

    def line(kernel, name, layout, words):
        print(f"{kernel:8s} {name:12s} {layout:6s} {words.size:9d} words  {hashlib.sha256(words.tobytes()).hexdigest()}", flush=True)

    try:
        for n_mels in (80, 128):
            for layout in ("bands", "frames"):
                tracks, scales = g_mel.crafted_tracks()
                frames_major = layout == "frames"
                buf, spans, total = g_mel.lay_out(pkg, np.random.default_rng(n_mels + frames_major), tracks, scales, n_mels, frames_major)
                line("mel", str(n_mels), layout, g_mel.run_kernel(pkg, ctx, buf, spans, total, n_mels, layout)[0])
        for name in g_spec.ALL_SETS:
            for layout in ("bands", "frames"):
                tracks, scales = g_spec.crafted_tracks(name)
                rec = g_spec.spec_of(pkg, name, layout)
                buf, spans, total = g_spec.lay_out(pkg, np.random.default_rng(len(name) + (layout == "frames")), tracks, scales, rec)
                line("melspec", name, layout, g_spec.run_kernel(ctx, buf, spans, total, rec)[0])
        for name in c_stft.SETS:
            for layout in c_stft.LAYOUTS[name]:
                tracks, scales = c_stft.crafted_tracks(name)
                rec = c_stft.stft_of(pkg, name, layout)
                buf, spans, total = g_stft.lay_out(pkg, np.random.default_rng(len(name) + (layout == "frames")), tracks, scales,
                                                   lambda n: c_stft.frame_count(rec, n), g_stft.width_of(rec))
                line("stft", name, layout, g_stft.run_kernel(ctx, buf, spans, total, rec)[0])
        for name in c_fbank.SETS:
            for layout in ("bands", "frames"):
                rec = c_fbank.spec_of(pkg, name, layout)
                c_fbank.crafted_tracks.dtype = rec.dtype
                tracks, scales = c_fbank.crafted_tracks(name, c_fbank.spec_of(pkg, name).tobytes())
                buf, spans, total = g_fbank.lay_out(pkg, np.random.default_rng(len(name) + (layout == "frames")), tracks, scales, rec)
                line("fbank", name, layout, g_fbank.run_kernel(ctx, buf, spans, total, rec)[0])
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
