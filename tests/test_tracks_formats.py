"""Track formats of the whole-file path (include/opusgpu.h, TRACK FORMATS), what needs no GPU: the exported symbols and the place
record, opusgpu_head_gain_scale, and the refusals that decode_files raises before any device work."""
import os
import re

import numpy as np
import pytest

import files_util as fu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["opusgpu_head_gain_scale", "opusgpu_tracks_assemble_device_as", "opusgpu_files_decode_as", "opusgpu_ms_tracks_assemble_device_as",
       "opusgpu_ms_files_decode_as"]


def test_symbols_and_place_record(pkg):
    lib = pkg.load_lib()
    hdr = open(os.path.join(ROOT, "include", "opusgpu.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in pkg.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert (pkg.TRACKS_S16, pkg.TRACKS_F32, pkg.TRACKS_F32_PLANAR) == (0, 1, 2)
    for name, value in (("S16", 0), ("F32", 1), ("F32_PLANAR", 2)):
        assert re.search(rf"#define OPUSGPU_TRACKS_{name} {value}\b", hdr), name
    d = pkg.TRACK_PLACE_DTYPE
    assert d.itemsize == 24 and "opusgpu_track_place { /* 24 bytes" in hdr
    assert [(n, d.fields[n][1], d.fields[n][0]) for n in d.names] == [
        ("track_offset", 0, np.dtype("<i8")), ("plane_samples", 8, np.dtype("<i8")), ("scale", 16, np.dtype("<f4")), ("reserved", 20, np.dtype("<i4"))]


def test_head_gain_scale(pkg):
    assert pkg.head_gain_scale(0) == np.float32(2.0 ** -15) and float(pkg.head_gain_scale(0)) == 2.0 ** -15
    for q8 in (-32768, -1541, -256, 1, 256, 1541, 32767):
        want = np.float32(10.0 ** (q8 / 5120.0) / 32768.0)
        got = pkg.head_gain_scale(q8)
        print(q8, float(got), float(want))
        assert abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1, q8  # positive floats: adjacent bit patterns are one ulp apart


@pytest.fixture(scope="module")
def batch(pkg):
    files = [c[1] for c in fu.corpus20(2, channel_switches=False)[:4]]
    b = pkg.FileBatch(files, channels=2)
    yield b
    b.close()


def test_format_and_scale_refusals(pkg, batch):
    n = batch.n_files
    assert pkg.track_format_args(batch) == (pkg.TRACKS_S16, None, None)
    fmt, scale, out = pkg.track_format_args(batch, "f32_planar", np.arange(1, n + 1) / 7.0)
    assert fmt == pkg.TRACKS_F32_PLANAR and scale.dtype == np.float32 and scale.shape == (n,) and out is None
    fmt, scale, _ = pkg.track_format_args(batch, "f32", "head_gain")
    assert (scale == np.float32(2.0 ** -15)).all()  # these heads carry no gain
    for kw in (dict(format="f64"), dict(format=1), dict(format="s16", scale=np.ones(n)), dict(format="s16", scale="head_gain"),
               dict(format="f32", scale=np.ones(n + 1)), dict(format="f32", scale="gain"),
               dict(format="f32", scale=[1.0] * (n - 1) + [np.nan]), dict(format="f32_planar", scale=[np.inf] + [1.0] * (n - 1)),
               dict(format="f32", scale=[-np.inf] * n)):
        with pytest.raises(ValueError):
            pkg.track_format_args(batch, **kw)
    lib = pkg.load_lib()
    for fn in (lib.opusgpu_files_decode_as, lib.opusgpu_ms_files_decode_as):  # no decoder: refused, nothing touched
        assert fn(None, batch.h, pkg.TRACKS_F32, None, None, None, None) == pkg.OPUSGPU_BAD_ARG


class Tensor:
    """What track_format_args looks at of a torch tensor.  (torch itself stays out of this process: it brings a HIP runtime of its
    own, see test_abi.py; tests/test_gpu_tracks_formats.py hands over real tensors.)"""

    def __init__(self, n, dtype="torch.float32", device=("cuda", 0), contiguous=True, ptr=4096):
        self.n, self.dtype, self.contiguous, self.ptr = n, dtype, contiguous, ptr
        self.is_cuda = device[0] == "cuda"
        self.device = type("Device", (), {"type": device[0], "index": device[1], "__str__": lambda d: f"{d.type}:{d.index}"})()

    def numel(self):
        return self.n

    def is_contiguous(self):
        return self.contiguous

    def data_ptr(self):
        return self.ptr

    def view(self, *_):
        return self


def test_out_refusals_need_no_device(pkg, batch):
    need = int(batch.track_samples) * batch.channels
    ok = Tensor(need)
    assert pkg.track_format_args(batch, "f32", None, ok, 0)[2] is ok
    assert pkg.track_format_args(batch, "s16", None, Tensor(need + 5, dtype="torch.int16"), 0)[0] == pkg.TRACKS_S16
    for fmt, t, dev in (("f32", Tensor(need, device=("cpu", None)), 0),       # a CPU tensor
                        ("f32", Tensor(need), 1),                             # another GPU's
                        ("f32", Tensor(need, dtype="torch.int16"), 0),        # the wrong dtype, both ways
                        ("s16", Tensor(need), 0),
                        ("f32_planar", Tensor(need, dtype="torch.float64"), 0),
                        ("f32_planar", Tensor(need - 1), 0),                  # too small
                        ("f32", Tensor(need, contiguous=False), 0),
                        ("f32", Tensor(need, ptr=4096 + 64), 0),              # not 128-byte aligned
                        ("f32", np.zeros(need, dtype=np.float32), 0)):        # not a tensor at all
        with pytest.raises(ValueError):
            pkg.track_format_args(batch, fmt, None, t, dev)
    # decode_files raises before it touches its decoder: an object without one is enough to see it
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.h, ctx.device, ctx.channels, ctx.n_streams = None, 0, 2, 0
    with pytest.raises(ValueError):
        ctx.decode_files(None, batch=batch, format="f32", out=Tensor(need, device=("cpu", None)))
    with pytest.raises(ValueError):
        ctx.decode_files(None, batch=batch, format="s16", scale=np.ones(batch.n_files))
