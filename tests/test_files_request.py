"""files_request: the keywords of decode_files -> the one C call they mean, for a stereo batch and a six-channel multistream one,
with no decoder anywhere.  The table holds what the two decode_files ladders that files_request replaced handed to the library.
Then the six track_*_args helpers, which keep the tuples they returned."""
import numpy as np
import pytest

from test_tracks_formats import Tensor
from test_tracks_melspec import spec_of
from test_tracks_resample import batch, ms_batch  # noqa: F401 (fixtures)

MIX, PARAMS = "mix record", "params record"
REFUSED = None
# keywords -> (entry, arguments between the batch and the format: scalars, records by kind), output channels, result kind),
# for the stereo batch and for the multistream one; entries without their opusgpu_ / opusgpu_ms_ prefix
TABLE = [
    (dict(),
     ("files_decode", (), 2, "tracks"), ("files_decode", (), 6, "tracks")),
    (dict(format="f32_planar", scale="head_gain"),
     ("files_decode_as", (), 2, "tracks"), ("files_decode_as", (), 6, "tracks")),
    (dict(rate=16000),
     ("files_decode_resampled", (16000, 0), 2, "resampled"), ("files_decode_resampled", (16000,), 6, "resampled")),
    (dict(rate=48000, mono=True),
     ("files_decode_resampled", (48000, 1), 1, "resampled"), REFUSED),
    (dict(mix="mono"),
     ("files_decode_mixed", (48000, MIX), 1, "resampled"), ("files_decode_mixed", (48000, MIX), 1, "resampled")),
    (dict(mix="stereo", rate=24000),
     ("files_decode_mixed", (24000, MIX), 2, "resampled"), ("files_decode_mixed", (24000, MIX), 2, "resampled")),
    (dict(resample=44100),
     ("files_decode_ratio", (147, 160, 0, None), 2, "resampled"), ("files_decode_ratio", (147, 160, None), 6, "resampled")),
    (dict(resample=(4, 6), mono=True),
     ("files_decode_ratio", (2, 3, 1, None), 1, "resampled"), REFUSED),
    (dict(resample=32000, mix="mono"),
     ("files_decode_ratio", (2, 3, 0, MIX), 1, "resampled"), ("files_decode_ratio", (2, 3, MIX), 1, "resampled")),
    (dict(features="logmel", mono=True),
     ("files_decode_mel", (1, None, PARAMS), 1, "features"), REFUSED),
    (dict(features="logmel", mix="mono", n_mels=128, feature_layout="frames", rate=16000),
     ("files_decode_mel", (0, MIX, PARAMS), 1, "features"), ("files_decode_mel", (MIX, PARAMS), 1, "features")),
    (dict(features="kaldi", mono=True),
     ("files_decode_melspec", (16000, 0, 0, 1, None, PARAMS), 1, "features"), REFUSED),
    (dict(features="tts", mono=True),
     ("files_decode_melspec", (0, 147, 320, 1, None, PARAMS), 1, "features"), REFUSED),
    (dict(features="kaldi", resample=16000, mix="mono"),
     ("files_decode_melspec", (0, 1, 3, 0, MIX, PARAMS), 1, "features"), ("files_decode_melspec", (0, 1, 3, MIX, PARAMS), 1, "features")),
]


def keywords(pkg, kw):
    kw = dict(kw)
    if kw.get("features") in ("kaldi", "tts"):
        kw["features"] = spec_of(pkg, kw["features"])
    return kw


def shown(pkg, a):
    if isinstance(a, np.ndarray):
        assert a.shape == (1,) and a.dtype in (pkg.MIX_MATRIX_DTYPE, pkg.MEL_PARAMS_DTYPE, pkg.SPEC_PARAMS_DTYPE)
        return MIX if a.dtype == pkg.MIX_MATRIX_DTYPE else PARAMS
    assert a is None or type(a) is int
    return a


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_the_table(pkg, batch, ms_batch, row):
    kw, *want = TABLE[row]
    for b, multistream, expected in ((batch, False, want[0]), (ms_batch, True, want[1])):
        if expected is REFUSED:
            assert kw.get("mono")  # a multistream decoder has no mono downmix, and its decode_files no such argument
            with pytest.raises(ValueError):
                pkg.files_request(b, multistream, 0, **keywords(pkg, kw))
            continue
        req = pkg.files_request(b, multistream, 0, **keywords(pkg, kw))  # no decoder anywhere
        assert (req.entry, tuple(shown(pkg, a) for a in req.args), req.channels, req.kind) == expected
        assert hasattr(pkg.load_lib(), ("opusgpu_ms_" if multistream else "opusgpu_") + req.entry)
        assert (req.mix is not None) == (MIX in expected[1]) and (req.params is not None) == (PARAMS in expected[1])
        assert req.out is None and len(req.offsets) == len(req.planes) == b.n_files
        planar = kw.get("format") == "f32_planar"
        assert req.fmt == (pkg.TRACKS_F32_PLANAR if planar else pkg.TRACKS_F32 if req.kind == "features" else pkg.TRACKS_S16)
        assert (req.scale is not None) == ("scale" in kw) and (req.scale is None or req.scale.dtype == np.float32)
        if req.mix is not None:
            assert int(req.mix["in_channels"][0]) == b.channels and int(req.mix["out_channels"][0]) == req.channels


def test_an_out_tensor_is_held_against_the_requests_size(pkg, batch):
    req = pkg.files_request(batch, rate=16000, mono=True, format="f32")
    ok = Tensor(req.total)
    assert pkg.files_request(batch, rate=16000, mono=True, format="f32", out=ok).out is ok
    plain = pkg.files_request(batch, format="f32")
    assert plain.total == int(batch.track_samples) and (plain.offsets == batch.info["track_offset"]).all()
    for kw in (dict(rate=16000, mono=True, format="f32", out=Tensor(req.total - 1)), dict(format="f32", out=Tensor(2 * plain.total - 1)),
               dict(mix="mono", mono=True), dict(rate=44100), dict(features="logmel")):
        with pytest.raises(ValueError):
            pkg.files_request(batch, **kw)


def test_the_helpers_return_what_they_returned(pkg, batch):
    """Their tuples are indexed by position elsewhere in the suite; files_request is made of them."""
    planned, n = batch.info["track_samples"], batch.n_files
    assert pkg.track_format_args(batch) == (pkg.TRACKS_S16, None, None)
    fmt, scale, out = pkg.track_format_args(batch, "f32", np.ones(n))
    assert (fmt, out) == (pkg.TRACKS_F32, None) and scale.dtype == np.float32 and scale.shape == (n,)

    assert pkg.track_rate_args(batch) is None
    D, ch, offs, total, out = pkg.track_rate_args(batch, 16000, True, "f32")
    want_offs, want_total = pkg.resample_layout(planned, 16000)
    assert (D, ch, total, out) == (3, 1, want_total, None) and (offs == want_offs).all()

    ratio, ch, offs, total, out, rec = pkg.track_ratio_args(batch, 44100)
    want_offs, want_total = pkg.resample_ratio_layout(planned, 147, 160)
    assert (ratio, ch, total, out, rec) == ((147, 160), 2, want_total, None, None) and (offs == want_offs).all()
    assert int(pkg.track_ratio_args(batch, (2, 3), mix="mono")[5]["out_channels"][0]) == 1

    D, ch, offs, total, out, rec = pkg.track_mix_args(batch, "mono", 24000)
    want_offs, want_total = pkg.resample_layout(planned, 24000)
    assert (D, ch, total, out) == (2, 1, want_total, None) and (offs == want_offs).all() and rec.dtype == pkg.MIX_MATRIX_DTYPE

    assert pkg.track_feature_args(batch) is None
    rec, mrec, scale, offs, planes, total, out = pkg.track_feature_args(batch, "logmel", 128, "frames", mono=True)
    want = pkg.mel_layout(planned, 128, "frames")
    assert (mrec, scale, out, total) == (None, None, None, want[2]) and (offs == want[0]).all() and (planes == want[1]).all()
    assert np.array_equal(rec, pkg.mel_params(128, "frames"))

    kaldi = spec_of(pkg, "kaldi")
    rec, mrec, scale, offs, planes, total, out, how = pkg.track_spectrogram_args(batch, kaldi, mono=True)
    want = pkg.spec_layout(planned, 1, 3, kaldi)
    assert (mrec, scale, out, how, total) == (None, None, None, (16000, 0, 0), want[2]) and (offs == want[0]).all() and (planes == want[1]).all()
    assert np.array_equal(rec, kaldi)
    req = pkg.files_request(batch, features=kaldi, mono=True)
    assert (req.total, req.args[:3]) == (total, how) and (req.offsets == offs).all() and (req.planes == planes).all()
