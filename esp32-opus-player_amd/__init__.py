"""ctypes binding of libopusgpu.so (the MI355X batched Opus decoder) for tests and bench.py.

This module is plumbing only: every decode goes through the C ABI declared in include/opusgpu.h and
runs on the GPU.  There is no CPU fallback -- if the HIP library is missing or no GPU is usable the
calls raise.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)

The directory name has a hyphen, so import it with `importlib` (see tests/conftest.py: load_pkg()).
"""
import ctypes as C
import os
import typing

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OPUSGPU_LIB", os.path.join(HERE, "libopusgpu.so"))  # override: experiments only

OPUSGPU_ERR_NO_DEVICE = -100
FRAME = 960

EXPORTS = [
    "opusgpu_version", "opusgpu_ctx_create", "opusgpu_ctx_destroy", "opusgpu_last_error",
    "opusgpu_streams_alloc", "opusgpu_streams_reset", "opusgpu_stream_count", "opusgpu_stream_channels",
    "opusgpu_stream_state_bytes", "opusgpu_debug_stage_taps", "opusgpu_decode_packets", "opusgpu_decode_packets_fec", "opusgpu_packet_to_frames",
    "opusgpu_dev_alloc", "opusgpu_dev_free", "opusgpu_memcpy_h2d", "opusgpu_memcpy_d2h",
    "opusgpu_decode_step_device", "opusgpu_decode_step_device_modes", "opusgpu_decode_steps_device", "opusgpu_synchronize", "opusgpu_event_create", "opusgpu_event_record",
    "opusgpu_event_elapsed_ms", "opusgpu_event_destroy", "opusgpu_event_synchronize", "opusgpu_stream_state_get", "opusgpu_stream_pitch_get",
    "opusgpu_upload_async", "opusgpu_upload_fence", "opusgpu_stream_wait_event", "opusgpu_host_register", "opusgpu_host_unregister",
    "opusgpu_pages_demux", "opusgpu_pages_demux_into", "opusgpu_page_batch_arena_offset", "opusgpu_page_batch_steps", "opusgpu_page_batch_step", "opusgpu_page_batch_arena",
    "opusgpu_page_batch_free", "opusgpu_pages_crc_device", "opusgpu_output_stage_device",
    "opusgpu_set_mode", "opusgpu_get_mode", "opusgpu_set_pipeline", "opusgpu_get_pipeline", "opusgpu_packet_to_frames_mode",
    "opusgpu_empty_packet_to_frames",
    "opusgpu_ms_create", "opusgpu_ms_destroy", "opusgpu_ms_last_error", "opusgpu_ms_set_mode", "opusgpu_ms_reset",
    "opusgpu_ms_packet_to_frames", "opusgpu_ms_decode_packets", "opusgpu_ms_decode_step_device", "opusgpu_ms_synchronize",
    "opusgpu_files_plan", "opusgpu_file_batch_steps", "opusgpu_file_batch_step", "opusgpu_file_batch_segments", "opusgpu_file_batch_arena",
    "opusgpu_file_batch_track_samples", "opusgpu_file_batch_packet_start", "opusgpu_file_batch_free", "opusgpu_tracks_assemble_device",
    "opusgpu_files_decode", "opusgpu_head_gain_scale", "opusgpu_tracks_assemble_device_as", "opusgpu_files_decode_as",
    "opusgpu_file_layout", "opusgpu_ms_files_plan", "opusgpu_ms_file_batch_steps", "opusgpu_ms_file_batch_step", "opusgpu_ms_file_batch_segments",
    "opusgpu_ms_file_batch_arena", "opusgpu_ms_file_batch_track_samples", "opusgpu_ms_file_batch_packet_start", "opusgpu_ms_file_batch_free",
    "opusgpu_ms_tracks_assemble_device", "opusgpu_ms_files_decode", "opusgpu_ms_files_last_steps_ms",
    "opusgpu_ms_tracks_assemble_device_as", "opusgpu_ms_files_decode_as",
    "opusgpu_resample_taps", "opusgpu_resample_layout", "opusgpu_tracks_resample_device", "opusgpu_files_decode_resampled",
    "opusgpu_ms_files_decode_resampled",
    "opusgpu_downmix_matrix", "opusgpu_tracks_resample_mixed_device", "opusgpu_files_decode_mixed", "opusgpu_ms_files_decode_mixed",
    "opusgpu_mel_basis", "opusgpu_mel_filterbank", "opusgpu_mel_layout", "opusgpu_tracks_mel_device", "opusgpu_files_decode_mel",
    "opusgpu_ms_files_decode_mel",
    "opusgpu_resample_ratio_taps", "opusgpu_resample_ratio_layout", "opusgpu_tracks_resample_ratio_device", "opusgpu_files_decode_ratio",
    "opusgpu_ms_files_decode_ratio",
    "opusgpu_spec_basis", "opusgpu_spec_filterbank", "opusgpu_spec_fft_tables", "opusgpu_spec_tile", "opusgpu_spec_layout", "opusgpu_tracks_melspec_device", "opusgpu_files_decode_melspec",
    "opusgpu_ms_files_decode_melspec",
    "opusgpu_stft_basis", "opusgpu_stft_fft_tables", "opusgpu_stft_tile", "opusgpu_stft_layout", "opusgpu_tracks_stft_device", "opusgpu_files_decode_stft",
    "opusgpu_ms_files_decode_stft",
    "opusgpu_fbank_window", "opusgpu_fbank_filterbank", "opusgpu_fbank_dct", "opusgpu_fbank_layout", "opusgpu_tracks_fbank_device",
    "opusgpu_files_decode_fbank", "opusgpu_ms_files_decode_fbank",
    "opusgpu_loudness_weights", "opusgpu_loudness_gain", "opusgpu_tracks_loudness_device", "opusgpu_set_loudness", "opusgpu_last_loudness",
    "opusgpu_ms_set_loudness", "opusgpu_ms_last_loudness",
    "opusgpu_files_plan_cuts", "opusgpu_ms_files_plan_cuts", "opusgpu_file_batch_track_stride", "opusgpu_ms_file_batch_track_stride",
    "opusgpu_tracks_fill_tail_device",
    "opusgpu_set_feature_batch", "opusgpu_ms_set_feature_batch", "opusgpu_feat_batch_layout", "opusgpu_tracks_feature_batch_device",
    "opusgpu_set_wave_batch", "opusgpu_ms_set_wave_batch", "opusgpu_last_wave_stats", "opusgpu_ms_last_wave_stats",
    "opusgpu_wave_batch_layout", "opusgpu_tracks_wave_batch_device",
    "opusgpu_set_wave_trim", "opusgpu_ms_set_wave_trim", "opusgpu_last_wave_trim", "opusgpu_ms_last_wave_trim",
    "opusgpu_last_wave_trim_flags", "opusgpu_ms_last_wave_trim_flags", "opusgpu_tracks_wave_trim_device",
    "opusgpu_set_stft_batch", "opusgpu_ms_set_stft_batch", "opusgpu_stft_batch_layout", "opusgpu_tracks_stft_batch_device",
]


class MsLayout(C.Structure):
    """opusgpu_ms_layout (include/opusgpu.h, MULTISTREAM)."""
    _fields_ = [("channels", C.c_int32), ("streams", C.c_int32), ("coupled", C.c_int32), ("mapping", C.c_uint8 * 256)]


def ms_layout(channels, streams, coupled, mapping=None):
    """An MsLayout; mapping defaults to the identity (output channel c <- decoded channel c)."""
    lay = MsLayout()
    lay.channels, lay.streams, lay.coupled = channels, streams, coupled
    m = list(range(channels)) if mapping is None else list(mapping)
    for c in range(256):
        lay.mapping[c] = m[c] if c < len(m) else 255
    return lay


class OutputCfg(C.Structure):
    """opusgpu_output_cfg (include/opusgpu.h): the player's output settings, src/main.cpp m_vol / m_f_forceMono /
    m_bitsPerSample / m_channels."""
    _fields_ = [("volume", C.c_uint8), ("force_mono", C.c_uint8), ("bits", C.c_uint8), ("channels", C.c_uint8)]


OUTPUT_CFG_DTYPE = np.dtype([("volume", "u1"), ("force_mono", "u1"), ("bits", "u1"), ("channels", "u1")])


class _SilkChTaps(C.Structure):
    _fields_ = [("pitchL", C.c_int32 * 4), ("Gains_Q16", C.c_int32 * 4), ("PredCoef_Q12", (C.c_int16 * 16) * 2),
                ("LTPCoef_Q14", C.c_int16 * 20), ("LTP_scale_Q14", C.c_int32), ("signalType", C.c_int32), ("quantOffsetType", C.c_int32)]


class StageTaps(C.Structure):
    """opusgpu_stage_taps (include/opusgpu.h): what the kernels of the last decode step left between the stages."""
    _fields_ = [("celt_valid", C.c_int32), ("celt_ret", C.c_int32), ("silence", C.c_int32), ("transient", C.c_int32), ("lm", C.c_int32),
                ("spread", C.c_int32), ("dual_stereo", C.c_int32), ("anti_collapse_on", C.c_int32), ("intensity", C.c_int32),
                ("pf_pitch", C.c_int32), ("pf_gain", C.c_int32), ("pf_tapset", C.c_int32), ("n_leaves", C.c_int32),
                ("celt_rng_final", C.c_uint32), ("bandE", C.c_int16 * 42), ("pulses", C.c_int16 * 21), ("tf_res", C.c_int8 * 21),
                ("pad0", C.c_int8 * 3), ("syn_post", (C.c_int32 * 960) * 2), ("overlap_tail", (C.c_int32 * 60) * 2),
                ("state_bandE", C.c_int16 * 42), ("state_logE1", C.c_int16 * 42), ("state_logE2", C.c_int16 * 42), ("pad1", C.c_int16),
                ("state_rng", C.c_uint32), ("pf_period", C.c_int32), ("pf_gain_state", C.c_int32), ("pf_tapset_state", C.c_int32),
                ("silk_valid", C.c_int32), ("silk_ret", C.c_int32), ("decode_only_middle", C.c_int32), ("ms_pred_q13", C.c_int32 * 2),
                ("silk_ch", _SilkChTaps * 2), ("silk_out", (C.c_int16 * 320) * 2), ("silk_sLPC_Q14", (C.c_int32 * 16) * 2),
                ("silk_fs_kHz", C.c_int32 * 2)]


class FrameDesc(C.Structure):
    _fields_ = [("stream", C.c_int32), ("offset", C.c_int32), ("len", C.c_int32), ("flags", C.c_int32)]


HAS_SILK, HAS_HYBRID, HAS_CELT = 1, 2, 4  # opusgpu_decode_step_device_modes
STEP_KEEPS_MODE = 8  # OPUSGPU_STEP_KEEPS_MODE: no stream of the step has decoded a frame of another mode since its last reset


def toc_modes(toc):
    """The mode mask of a step whose frames all carry this TOC byte."""
    return HAS_CELT if toc & 0x80 else (HAS_HYBRID if (toc & 0x60) == 0x60 else HAS_SILK)


DESC_DTYPE = np.dtype([("stream", "<i4"), ("offset", "<i4"), ("len", "<i4"), ("flags", "<i4")])
# opusgpu_page_info (include/opusgpu.h)
PAGE_INFO_DTYPE = np.dtype([("status", "<i4"), ("packets", "<i4"), ("first_step", "<i4"), ("header_type", "<i4"),
                            ("serial", "<u4"), ("seqno", "<u4"), ("granulepos", "<i8")])
PAGE_BAD_CAPTURE, PAGE_BAD_CRC, PAGE_SPANS, PAGE_BAD_PACKET, PAGE_BAD_STREAM = -200, -201, -202, -203, -204
PAGES_VERIFY_CRC, PAGES_GROUP_BY_MODE, PAGES_ORDER_BY_HEADER = 1, 2, 4

# opusgpu_track_seg / opusgpu_track_state / opusgpu_file_info (include/opusgpu.h, WHOLE FILES)
TRACK_SEG_DTYPE = np.dtype([("slot", "<i4"), ("src_first", "<i4"), ("count", "<i4"), ("track", "<i4"), ("dst_first", "<i8"),
                            ("packet_seq", "<i4"), ("reserved", "<i4")])
TRACK_STATE_DTYPE = np.dtype([("first_bad", "<i4"), ("code", "<i4")])
FILE_INFO_DTYPE = np.dtype([("status", "<i4"), ("channels", "<i4"), ("pre_skip", "<i4"), ("output_gain", "<i4"), ("mapping_family", "<i4"),
                            ("packets", "<i4"), ("frames", "<i4"), ("holes", "<i4"), ("track_samples", "<i8"), ("track_offset", "<i8")])
# opusgpu_track_place and the OPUSGPU_TRACKS_* formats (include/opusgpu.h, TRACK FORMATS)
TRACK_PLACE_DTYPE = np.dtype([("track_offset", "<i8"), ("plane_samples", "<i8"), ("scale", "<f4"), ("reserved", "<i4")])
# opusgpu_cut / opusgpu_cut_info / opusgpu_tail_span (include/opusgpu.h, WHOLE FILES / CUTS)
CUT_DTYPE = np.dtype([("file", "<i4"), ("preroll", "<i4"), ("start", "<i8"), ("count", "<i8")])
CUT_INFO_DTYPE = np.dtype([("first_packet", "<i4"), ("packets", "<i4"), ("lead", "<i4"), ("exact", "<i4"), ("start", "<i8")])
TAIL_SPAN_DTYPE = np.dtype([("track_offset", "<i8"), ("plane_samples", "<i8"), ("first", "<i8"), ("end", "<i8")])
CUT_PREROLL = 3840  # OPUSGPU_CUT_PREROLL: 80 ms, RFC 7845 section 4.6
TRACKS_S16, TRACKS_F32, TRACKS_F32_PLANAR = 0, 1, 2
TRACK_FORMATS = {"s16": TRACKS_S16, "f32": TRACKS_F32, "f32_planar": TRACKS_F32_PLANAR}
# opusgpu_resample_span and the rates of the resampled tracks (include/opusgpu.h, TRACK RATES): rate -> D = 48000 / rate
RESAMPLE_SPAN_DTYPE = np.dtype([("in_offset", "<i8"), ("in_samples", "<i8"), ("out_offset", "<i8"), ("out_plane", "<i8"), ("scale", "<f4"),
                                ("reserved", "<i4")])
TRACK_RATES = {48000: 1, 24000: 2, 16000: 3, 12000: 4, 8000: 6}
# opusgpu_mix_matrix (include/opusgpu.h, CHANNEL MIX): m[o][c] in Q14
MIX_MATRIX_DTYPE = np.dtype([("out_channels", "<i4"), ("in_channels", "<i4"), ("m", "<i2", (8, 8))])
# opusgpu_mel_params / opusgpu_mel_span and the constants of the log-mel features (include/opusgpu.h, TRACK FEATURES)
MEL_PARAMS_DTYPE = np.dtype([("n_mels", "<i4"), ("layout", "<i4"), ("reserved", "<i4", (6,))])
MEL_SPAN_DTYPE = np.dtype([("in_offset", "<i8"), ("in_samples", "<i8"), ("out_offset", "<i8"), ("plane", "<i8"), ("scale", "<f4"),
                           ("reserved", "<i4")])
MEL_NFFT, MEL_HOP, MEL_SR, MEL_BINS = 400, 160, 16000, 201
MEL_BANDS_MAJOR, MEL_FRAMES_MAJOR = 0, 1
MEL_LAYOUTS = {"bands": MEL_BANDS_MAJOR, "frames": MEL_FRAMES_MAJOR}
# opusgpu_spec_params and its enums (include/opusgpu.h, TRACK SPECTROGRAMS)
SPEC_PARAMS_DTYPE = np.dtype([("sample_rate", "<i4"), ("n_fft", "<i4"), ("win_length", "<i4"), ("hop", "<i4"), ("n_mels", "<i4"),
                              ("mel_scale", "<i4"), ("norm", "<i4"), ("power", "<i4"), ("log", "<i4"), ("frames", "<i4"), ("layout", "<i4"),
                              ("fmin", "<f4"), ("fmax", "<f4"), ("floor", "<f4"), ("reserved", "<i4", (2,))])
SPEC_SCALES = {"slaney": 0, "htk": 1}
SPEC_NORMS = {"slaney": 0, None: 1, "none": 1}
SPEC_LOGS = {None: 0, "none": 0, "log10": 1, "ln": 2}
SPEC_FRAMES = {"torch": 0, "whisper": 1}
SPEC_ALGO_DENSE, SPEC_ALGO_FFT = 0, 1  # OPUSGPU_SPEC_ALGO_*: reserved[1] of the record
SPEC_ALGOS = {"dense": SPEC_ALGO_DENSE, "fft": SPEC_ALGO_FFT}
# opusgpu_stft_params (include/opusgpu.h, TRACK STFT); log, frames and layout take TRACK SPECTROGRAMS' and TRACK FEATURES' values
STFT_PARAMS_DTYPE = np.dtype([("sample_rate", "<i4"), ("n_fft", "<i4"), ("win_length", "<i4"), ("hop", "<i4"), ("power", "<i4"), ("log", "<i4"),
                              ("frames", "<i4"), ("layout", "<i4"), ("floor", "<f4"), ("reserved", "<i4", (7,))])
STFT_COMPLEX = 0  # OPUSGPU_STFT_COMPLEX: power=None
STFT_ALGO_DENSE, STFT_ALGO_FFT = 0, 1  # OPUSGPU_STFT_ALGO_*: reserved[1] of the record
STFT_ALGOS = {"dense": STFT_ALGO_DENSE, "fft": STFT_ALGO_FFT}
# opusgpu_fbank_params and its enums (include/opusgpu.h, TRACK KALDI FEATURES)
FBANK_PARAMS_DTYPE = np.dtype([("sample_rate", "<i4"), ("frame_length", "<i4"), ("frame_shift", "<i4"), ("n_fft", "<i4"), ("n_mels", "<i4"),
                               ("n_ceps", "<i4"), ("window", "<i4"), ("snip_edges", "u1"), ("remove_dc", "u1"), ("power", "u1"), ("log", "u1"),
                               ("layout", "<i4"), ("preemphasis", "<f4"), ("low_freq", "<f4"), ("high_freq", "<f4"), ("floor", "<f4"),
                               ("cepstral_lifter", "<f4"), ("reserved", "<i4", (2,))])
FBANK_WINDOWS = {"povey": 0, "hanning": 1, "hamming": 2, "rectangular": 3, "blackman": 4}
FBANK_LOG_NONE, FBANK_LOG_LN = 0, 1
FBANK_FLOOR = 1.1920929e-07  # FLT_EPSILON, Kaldi's floor under the log
# opusgpu_loudness_span / opusgpu_loudness / opusgpu_loudness_req and the request's modes (include/opusgpu.h, TRACK LOUDNESS)
LOUDNESS_SPAN_DTYPE = np.dtype([("in_offset", "<i8"), ("in_samples", "<i8")])
LOUDNESS_DTYPE = np.dtype([("lufs", "<f4"), ("peak", "<f4"), ("blocks", "<i4"), ("gated", "<i4")])
LOUDNESS_REQ_DTYPE = np.dtype([("mode", "<i4"), ("target_lufs", "<f4"), ("peak_limit", "<f4"), ("n_weights", "<i4"), ("weights", "<f4", (8,))])
FEAT_BATCH_REQ_DTYPE = np.dtype([("stride_frames", "<i8"), ("var_floor", "<f8"), ("enabled", "<i4"), ("norm", "<i4"), ("pad_mode", "<i4"),
                                 ("pad_value", "<f4"), ("range", "<f4"), ("add", "<f4"), ("mul", "<f4"), ("reserved", "<i4", (5,))])
FEAT_SPAN_DTYPE = np.dtype([("grid_offset", "<i8"), ("plane", "<i8"), ("frames", "<i8")])
FEAT_NORMS = {None: 0, "none": 0, "whisper": 1, "cmn": 2, "cmvn": 3, "affine": 4}
FEAT_NORM_NONE, FEAT_NORM_WHISPER, FEAT_NORM_CMN, FEAT_NORM_CMVN, FEAT_NORM_AFFINE = range(5)
FEAT_PAD_VALUE, FEAT_PAD_NORMALIZED = 0, 1
FEAT_SEG = 1024  # OPUSGPU_FEAT_SEG: frames per segment of the statistics
STFT_BATCH_REQ_DTYPE = np.dtype(FEAT_BATCH_REQ_DTYPE.descr)  # opusgpu_stft_batch_req: the fields of opusgpu_feat_batch_req
STFT_BATCH_SPAN_DTYPE = np.dtype(FEAT_SPAN_DTYPE.descr)      # opusgpu_stft_batch_span
STFT_NORM_REFMAX = 5  # OPUSGPU_STFT_NORM_REFMAX
STFT_NORMS = dict(FEAT_NORMS, refmax=STFT_NORM_REFMAX)
STFT_BATCH_MAX_BINS = 1025
WAVE_BATCH_REQ_DTYPE = np.dtype([("stride_samples", "<i8"), ("eps", "<f8"), ("target", "<f8"), ("enabled", "<i4"), ("norm", "<i4"),
                                 ("pad_value", "<f4"), ("mask", "<i4"), ("reserved", "<i4", (6,))])
WAVE_SPAN_DTYPE = np.dtype([("in_offset", "<i8"), ("samples", "<i8"), ("scale", "<f4"), ("reserved", "<i4")])
WAVE_STAT_DTYPE = np.dtype([("count", "<i8"), ("sum", "<i8"), ("sumsq", "<u8"), ("sub", "<f8"), ("mul", "<f8"), ("peak", "<i4"), ("reserved", "<i4")])
WAVE_NORMS = {None: 0, "none": 0, "zmuv": 1, "peak": 2}
WAVE_NORM_NONE, WAVE_NORM_ZMUV, WAVE_NORM_PEAK = range(3)
WAVE_EPS = 1e-7  # Wav2Vec2FeatureExtractor's
WAVE_TRIM_REQ_DTYPE = np.dtype([("ratio", "<f8"), ("threshold", "<u8"), ("enabled", "<i4"), ("mode", "<i4"), ("frame_length", "<i4"),
                                ("hop", "<i4"), ("margin", "<i4"), ("flags", "<i4"), ("reserved", "<i4", (6,))])
WAVE_TRIM_STAT_DTYPE = np.dtype([("start", "<i8"), ("count", "<i8"), ("full", "<i8"), ("emax", "<u8"), ("thr", "<u8"), ("frames", "<i4"),
                                 ("first", "<i4"), ("last", "<i4"), ("active", "<i4"), ("reserved", "<i4", (2,))])
WAVE_TRIM_REL, WAVE_TRIM_ABS = 0, 1
LOUDNESS_OFF, LOUDNESS_MEASURE, LOUDNESS_NORMALIZE = 0, 1, 2
OPUSGPU_BAD_ARG, OPUSGPU_UNIMPLEMENTED, OPUSGPU_CELT_BAD_ARG = -1, -5, -18
RFC_FRAME = 2880

_lib = None


def load_lib():
    """Load libopusgpu.so; raises (loudly) if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the decode path.")
    lib = C.CDLL(LIB_PATH)
    vp, i32p, u8pp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_char_p)
    lib.opusgpu_version.restype = C.c_int
    lib.opusgpu_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.opusgpu_ctx_destroy.argtypes = [vp]
    lib.opusgpu_ctx_destroy.restype = None
    lib.opusgpu_last_error.argtypes = [vp]
    lib.opusgpu_last_error.restype = C.c_char_p
    lib.opusgpu_streams_alloc.argtypes = [vp, C.c_int, C.c_int]
    lib.opusgpu_streams_reset.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.opusgpu_stream_count.argtypes = [vp]
    lib.opusgpu_stream_channels.argtypes = [vp]
    lib.opusgpu_stream_state_bytes.restype = C.c_size_t
    lib.opusgpu_decode_packets.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.opusgpu_decode_packets_fec.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.opusgpu_packet_to_frames.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(FrameDesc)]
    lib.opusgpu_packet_to_frames_mode.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int, C.POINTER(FrameDesc)]
    lib.opusgpu_empty_packet_to_frames.argtypes = [C.c_int32, C.c_int32, C.c_int, C.c_int, C.POINTER(FrameDesc)]
    lib.opusgpu_set_mode.argtypes = [vp, C.c_int]
    lib.opusgpu_get_mode.argtypes = [vp]
    lib.opusgpu_set_pipeline.argtypes = [vp, C.c_int]
    lib.opusgpu_get_pipeline.argtypes = [vp]
    lib.opusgpu_dev_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.opusgpu_dev_free.argtypes = [vp, vp]
    lib.opusgpu_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    lib.opusgpu_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    lib.opusgpu_decode_step_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_decode_step_device_modes.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int]
    lib.opusgpu_decode_steps_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int]
    lib.opusgpu_synchronize.argtypes = [vp]
    lib.opusgpu_event_create.argtypes = [vp, C.POINTER(vp)]
    lib.opusgpu_event_record.argtypes = [vp, vp]
    lib.opusgpu_event_elapsed_ms.argtypes = [vp, vp, vp, C.POINTER(C.c_float)]
    lib.opusgpu_event_destroy.argtypes = [vp, vp]
    lib.opusgpu_event_synchronize.argtypes = [vp, vp]
    lib.opusgpu_upload_async.argtypes = [vp, vp, vp, C.c_size_t]
    lib.opusgpu_upload_fence.argtypes = [vp, vp]
    lib.opusgpu_stream_wait_event.argtypes = [vp, vp, vp]
    lib.opusgpu_host_register.argtypes = [vp, vp, C.c_size_t]
    lib.opusgpu_host_unregister.argtypes = [vp, vp]
    lib.opusgpu_stream_state_get.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.opusgpu_stream_pitch_get.argtypes = [vp, C.c_int, vp]
    lib.opusgpu_debug_stage_taps.argtypes = [vp, C.c_int, vp]
    lib.opusgpu_pages_demux.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.opusgpu_pages_demux_into.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(vp)]
    lib.opusgpu_page_batch_arena_offset.argtypes = [vp]
    lib.opusgpu_page_batch_arena_offset.restype = C.c_size_t
    lib.opusgpu_page_batch_steps.argtypes = [vp]
    lib.opusgpu_page_batch_step.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    lib.opusgpu_page_batch_arena.argtypes = [vp, C.POINTER(C.c_size_t)]
    lib.opusgpu_page_batch_arena.restype = vp
    lib.opusgpu_page_batch_free.argtypes = [vp]
    lib.opusgpu_page_batch_free.restype = None
    lib.opusgpu_pages_crc_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_output_stage_device.argtypes = [vp, C.c_int, C.c_int, vp, C.c_longlong, vp, C.c_int, vp, OutputCfg, vp,
                                                C.c_longlong, vp]
    lib.opusgpu_ms_create.argtypes = [C.c_int, C.POINTER(MsLayout), C.c_int, C.POINTER(vp)]
    lib.opusgpu_ms_destroy.argtypes = [vp]
    lib.opusgpu_ms_destroy.restype = None
    lib.opusgpu_ms_last_error.argtypes = [vp]
    lib.opusgpu_ms_last_error.restype = C.c_char_p
    lib.opusgpu_ms_set_mode.argtypes = [vp, C.c_int]
    lib.opusgpu_ms_reset.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.opusgpu_ms_packet_to_frames.argtypes = [C.POINTER(MsLayout), C.c_char_p, C.c_int32, C.c_int32, C.c_int, C.POINTER(FrameDesc), vp]
    lib.opusgpu_ms_decode_packets.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.opusgpu_ms_decode_step_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_synchronize.argtypes = [vp]
    lib.opusgpu_files_plan.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    lib.opusgpu_tracks_assemble_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.opusgpu_files_decode.argtypes = [vp, vp, vp, vp, vp]
    lib.opusgpu_head_gain_scale.argtypes = [C.c_int32]
    lib.opusgpu_head_gain_scale.restype = C.c_float
    lib.opusgpu_tracks_assemble_device_as.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    lib.opusgpu_files_decode_as.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    lib.opusgpu_file_layout.argtypes = [vp, C.c_int64, C.POINTER(MsLayout), vp]
    lib.opusgpu_ms_files_plan.argtypes = [C.c_int, vp, vp, C.POINTER(MsLayout), C.c_int, C.c_int, vp, C.POINTER(vp)]
    for prefix, step_more in (("opusgpu_file_batch", [C.POINTER(C.c_int)]), ("opusgpu_ms_file_batch", [])):
        def f(name):
            return getattr(lib, f"{prefix}_{name}")
        f("steps").argtypes = [vp]
        f("step").argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)] + step_more
        f("segments").argtypes = [vp, C.c_int, C.POINTER(vp)]
        f("arena").argtypes = [vp, C.POINTER(C.c_size_t)]
        f("arena").restype = vp
        f("track_samples").argtypes = [vp]
        f("track_samples").restype = C.c_int64
        f("packet_start").argtypes = [vp, C.c_int, C.c_int]
        f("packet_start").restype = C.c_int64
        f("free").argtypes = [vp]
        f("free").restype = None
        f("track_stride").argtypes = [vp]
        f("track_stride").restype = C.c_int64
    lib.opusgpu_files_plan_cuts.argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(vp)]
    lib.opusgpu_ms_files_plan_cuts.argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_int64, C.POINTER(MsLayout), C.c_int, C.c_int, vp, vp,
                                               C.POINTER(vp)]
    lib.opusgpu_tracks_fill_tail_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp]
    lib.opusgpu_ms_tracks_assemble_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode.argtypes = [vp, vp, vp, vp, vp]
    lib.opusgpu_ms_tracks_assemble_device_as.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_as.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    lib.opusgpu_ms_files_last_steps_ms.restype = C.c_float
    lib.opusgpu_resample_taps.argtypes = [C.c_int, C.POINTER(vp)]
    lib.opusgpu_resample_layout.argtypes = [C.c_int, vp, C.c_int, vp]
    lib.opusgpu_resample_layout.restype = C.c_int64
    lib.opusgpu_tracks_resample_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.opusgpu_files_decode_resampled.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_resampled.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_downmix_matrix.argtypes = [C.c_int, C.c_int, vp]
    lib.opusgpu_resample_ratio_taps.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    lib.opusgpu_resample_ratio_layout.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp]
    lib.opusgpu_resample_ratio_layout.restype = C.c_int64
    lib.opusgpu_tracks_resample_ratio_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    lib.opusgpu_files_decode_ratio.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_ratio.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_tracks_resample_mixed_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    lib.opusgpu_files_decode_mixed.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_mixed.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_mel_basis.argtypes = [C.POINTER(vp), C.POINTER(vp)]
    lib.opusgpu_mel_filterbank.argtypes = [C.c_int, C.POINTER(vp)]
    lib.opusgpu_mel_layout.argtypes = [C.c_int, vp, vp, vp]
    lib.opusgpu_mel_layout.restype = C.c_int64
    lib.opusgpu_tracks_mel_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_files_decode_mel.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_mel.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_spec_basis.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.opusgpu_spec_filterbank.argtypes = [vp, C.POINTER(vp)]
    lib.opusgpu_spec_fft_tables.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.opusgpu_spec_tile.argtypes = [vp]
    lib.opusgpu_spec_layout.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, vp]
    lib.opusgpu_spec_layout.restype = C.c_int64
    lib.opusgpu_tracks_melspec_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_files_decode_melspec.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_melspec.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_stft_basis.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.opusgpu_stft_fft_tables.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.opusgpu_stft_tile.argtypes = [vp]
    lib.opusgpu_stft_layout.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, vp]
    lib.opusgpu_stft_layout.restype = C.c_int64
    lib.opusgpu_tracks_stft_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_files_decode_stft.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_stft.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_fbank_window.argtypes = [vp, C.POINTER(vp)]
    lib.opusgpu_fbank_filterbank.argtypes = [vp, C.POINTER(vp)]
    lib.opusgpu_fbank_dct.argtypes = [vp, C.POINTER(vp)]
    lib.opusgpu_fbank_layout.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, vp]
    lib.opusgpu_fbank_layout.restype = C.c_int64
    lib.opusgpu_tracks_fbank_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
    lib.opusgpu_files_decode_fbank.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_ms_files_decode_fbank.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.opusgpu_loudness_weights.argtypes = [C.c_int, vp]
    lib.opusgpu_loudness_gain.argtypes = [vp, C.c_double, C.c_double]
    lib.opusgpu_loudness_gain.restype = C.c_double
    lib.opusgpu_tracks_loudness_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    for name in ("opusgpu_set_loudness", "opusgpu_ms_set_loudness"):
        getattr(lib, name).argtypes = [vp, vp]
    for name in ("opusgpu_last_loudness", "opusgpu_ms_last_loudness"):
        getattr(lib, name).argtypes = [vp, C.c_int, vp, vp]
    for name in ("opusgpu_set_feature_batch", "opusgpu_ms_set_feature_batch"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, C.c_int]
    lib.opusgpu_feat_batch_layout.argtypes = [C.c_int, C.c_int, C.c_int64, vp]
    lib.opusgpu_feat_batch_layout.restype = C.c_int64
    lib.opusgpu_tracks_feature_batch_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    for name in ("opusgpu_set_wave_batch", "opusgpu_ms_set_wave_batch"):
        getattr(lib, name).argtypes = [vp, vp]
    for name in ("opusgpu_last_wave_stats", "opusgpu_ms_last_wave_stats"):
        getattr(lib, name).argtypes = [vp, C.c_int, vp]
    lib.opusgpu_wave_batch_layout.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, vp]
    lib.opusgpu_wave_batch_layout.restype = C.c_int64
    lib.opusgpu_tracks_wave_batch_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    for name in ("opusgpu_set_wave_trim", "opusgpu_ms_set_wave_trim"):
        getattr(lib, name).argtypes = [vp, vp]
    for name in ("opusgpu_last_wave_trim", "opusgpu_ms_last_wave_trim"):
        getattr(lib, name).argtypes = [vp, C.c_int, vp]
    for name in ("opusgpu_last_wave_trim_flags", "opusgpu_ms_last_wave_trim_flags"):
        getattr(lib, name).argtypes = [vp, C.c_int64, vp]
        getattr(lib, name).restype = C.c_int64
    lib.opusgpu_tracks_wave_trim_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
    for name in ("opusgpu_set_stft_batch", "opusgpu_ms_set_stft_batch"):
        getattr(lib, name).argtypes = [vp, vp, vp, vp, C.c_int]
    lib.opusgpu_stft_batch_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, vp]
    lib.opusgpu_stft_batch_layout.restype = C.c_int64
    lib.opusgpu_tracks_stft_batch_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    _lib = lib
    return lib


class OpusGpuError(RuntimeError):
    code = 0  # the negative OPUSGPU_* value the call returned


class BufferTooSmall(OpusGpuError):
    def __init__(self, need):
        super().__init__(f"output memory too small: {need} bytes needed")
        self.need = need


def packet_to_frames(packet: bytes, stream: int = 0):
    """Host-only: frame descriptors of one packet (list of (offset, len, flags)) or a negative code."""
    lib = load_lib()
    d = (FrameDesc * 48)()
    n = lib.opusgpu_packet_to_frames(packet, len(packet), stream, d)
    if n < 0:
        return n
    return [(d[i].offset, d[i].len, d[i].flags) for i in range(n)]


def empty_packet_to_frames(last_flags, decoder_channels, frame_size, stream: int = 0):
    """Host-only: the frames of an EMPTY packet in reference mode (opusgpu_empty_packet_to_frames): `last_flags` the flags of the
    stream's last accepted packet, negative when it has had none since its reset.  List of (offset, len, flags) or a negative code."""
    lib = load_lib()
    d = (FrameDesc * 48)()
    n = lib.opusgpu_empty_packet_to_frames(stream, last_flags, decoder_channels, frame_size, d)
    if n < 0:
        return n
    return [(d[i].offset, d[i].len, d[i].flags) for i in range(n)]


def ms_packet_to_frames(layout, packet: bytes, decoder: int = 0, rfc=False):
    """Host-only: one multistream packet -> (duration in samples, [per elementary stream: list of (offset, len, flags)]), or a
    negative code (opusgpu_ms_packet_to_frames).  `layout`: an MsLayout (ms_layout())."""
    lib = load_lib()
    S = max(int(layout.streams), 1)
    d = (FrameDesc * (48 * S))()
    counts = np.zeros(S, dtype=np.int32)
    r = lib.opusgpu_ms_packet_to_frames(C.byref(layout), packet, len(packet), decoder, 1 if rfc else 0, d, counts.ctypes.data)
    if r < 0:
        return r
    return r, [[(d[s * 48 + k].offset, d[s * 48 + k].len, d[s * 48 + k].flags) for k in range(counts[s])] for s in range(S)]


class PageBatch:
    """Decode steps made from a batch of Ogg pages by opusgpu_pages_demux (host only, include/opusgpu.h).
    `blob` holds the pages back to back, page i = blob[offsets[i] : offsets[i] + lens[i]]; stream_ids[i] is the decoder
    stream page i belongs to.  info: one PAGE_INFO_DTYPE record per page (status = frames contributed or PAGE_*)."""

    def __init__(self, blob, offsets, lens, stream_ids, flags=PAGES_VERIFY_CRC | PAGES_GROUP_BY_MODE, threads=1, out_mem=None):
        """out_mem: a uint8 array (16-byte aligned, e.g. page-locked by Context.host_register) that receives the step tables and the
        arena (opusgpu_pages_demux_into); raises BufferTooSmall(need) when it is too small.  Then `self.image` is the part of out_mem
        that holds [tables | arena] and `self.arena_offset` where the arena begins in it: one upload carries the whole batch."""
        lib = load_lib()
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        offsets = np.asarray(offsets, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        n = len(offsets)
        if not (len(lens) == n and len(ids) == n):
            raise ValueError("offsets, lens and stream_ids must have one entry per page")
        if n and (offsets.min() < 0 or (offsets + lens).max() > blob.size):
            raise ValueError("a page lies outside the blob")
        ptrs = (np.uint64(blob.ctypes.data) + offsets.astype(np.uint64)).astype(np.uint64)
        self.info = np.zeros(n, dtype=PAGE_INFO_DTYPE)
        h = C.c_void_p()
        self.image, self.arena_offset = None, 0
        if out_mem is None:
            r = lib.opusgpu_pages_demux(n, ptrs.ctypes.data, lens.ctypes.data, ids.ctypes.data, flags, threads,
                                        self.info.ctypes.data, C.byref(h))
        else:
            need = C.c_size_t()
            r = lib.opusgpu_pages_demux_into(n, ptrs.ctypes.data, lens.ctypes.data, ids.ctypes.data, flags, threads,
                                             self.info.ctypes.data, out_mem.ctypes.data, out_mem.nbytes, C.byref(need), C.byref(h))
            if r == -2:
                raise BufferTooSmall(need.value)
        if r != 0:
            raise OpusGpuError(f"opusgpu_pages_demux failed: {r}")
        self.lib, self.h = lib, h
        self.n_steps = lib.opusgpu_page_batch_steps(h)
        nbytes = C.c_size_t()
        a = lib.opusgpu_page_batch_arena(h, C.byref(nbytes))
        self.arena = np.ctypeslib.as_array((C.c_uint8 * nbytes.value).from_address(a)) if nbytes.value else np.zeros(0, np.uint8)
        if out_mem is not None:
            self.arena_offset = lib.opusgpu_page_batch_arena_offset(h)
            self.image = out_mem[:self.arena_offset + nbytes.value]
            self._out_mem = out_mem

    @classmethod
    def with_gpu_crc(cls, ctx, d_blob, blob, offsets, lens, stream_ids, flags=PAGES_GROUP_BY_MODE, threads=1):
        """The steps PageBatch(..., flags | PAGES_VERIFY_CRC) makes, with the checksums computed on the GPU
        (opusgpu_pages_crc_device) from the copy of the pages that lies in HBM at `d_blob` (same offsets as in `blob`,
        e.g. raw pages delivered by the work-queue scatter); the host demux then skips its own CRC pass.  Pages whose
        checksum does not match are kept out of the demux and reported as PAGE_BAD_CRC."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = len(offsets)
        st = np.zeros(n, dtype=np.int32)
        if n:
            bufs = [ctx.dev_alloc(8 * n), ctx.dev_alloc(4 * n), ctx.dev_alloc(4 * n)]
            try:
                ctx.h2d(bufs[0], offsets)
                ctx.h2d(bufs[1], lens)
                ctx.pages_crc_device(n, d_blob, bufs[0], bufs[1], bufs[2])
                ctx.synchronize()
                ctx.d2h(st, bufs[2])
            finally:
                for b in bufs:
                    ctx.dev_free(b)
        batch = cls(blob, offsets, np.where(st == 1, lens, 0), stream_ids, flags & ~PAGES_VERIFY_CRC, threads)
        bad_crc = (st == 0) & (batch.info["status"] != PAGE_BAD_STREAM)  # (the demux looks at the stream id first)
        batch.info["status"][bad_crc] = PAGE_BAD_CRC
        hdr = np.ascontiguousarray(blob, dtype=np.uint8)
        for i in np.nonzero(bad_crc)[0]:  # the header fields the demux reports for such a page
            h = hdr[offsets[i]:offsets[i] + 27]
            batch.info[i]["header_type"] = h[5]
            batch.info[i]["granulepos"] = h[6:14].view("<i8")[0]
            batch.info[i]["serial"], batch.info[i]["seqno"] = h[14:18].view("<u4")[0], h[18:22].view("<u4")[0]
        return batch

    def step(self, k):
        """-> (descriptors [DESC_DTYPE], page index of every slot [int32]); views into the batch, valid until close()."""
        d, sp = C.c_void_p(), C.c_void_p()
        n = self.lib.opusgpu_page_batch_step(self.h, k, C.byref(d), C.byref(sp))
        if n < 0:
            raise IndexError(k)
        if n == 0:
            return np.zeros(0, dtype=DESC_DTYPE), np.zeros(0, dtype=np.int32)
        descs = np.frombuffer((C.c_uint8 * (16 * n)).from_address(d.value), dtype=DESC_DTYPE)
        pages = np.frombuffer((C.c_uint8 * (4 * n)).from_address(sp.value), dtype=np.int32)
        return descs, pages

    def close(self):
        if self.h:
            self.lib.opusgpu_page_batch_free(self.h)
            self.h = None
            self.arena = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cut_seconds(file, start_s, duration_s):
    """A cut of file `file` given in seconds -> (file, start, count) in samples at 48 kHz, each rounded as round(s * 48000)."""
    return int(file), int(round(start_s * 48000)), int(round(duration_s * 48000))


def cut_records(cuts, preroll=CUT_PREROLL):
    """cuts: a sequence of (file, start, count) or (file, start, count, preroll), in samples at 48 kHz on the axis of the file's
    whole-file track; count None or negative: to the end; preroll: decoded samples wanted in front of `start` where the cut names
    none (negative: 3840, 80 ms) -> CUT_DTYPE records (opusgpu_cut)."""
    cuts = [tuple(c) for c in cuts]
    rec = np.zeros(len(cuts), dtype=CUT_DTYPE)
    for t, c in enumerate(cuts):
        if len(c) not in (3, 4):
            raise ValueError(f"a cut is (file, start, count) or (file, start, count, preroll), not {c!r}")
        rec[t] = (int(c[0]), int(c[3] if len(c) == 4 else preroll), int(c[1]), -1 if c[2] is None else int(c[2]))
    return rec


class _PlannedFiles:
    """What FileBatch and MsFileBatch share: the plan call, the batch's accessors (the C family `_prefix`: opusgpu_file_batch /
    opusgpu_ms_file_batch) and its lifetime.  A slot of a step has `_width` descriptors."""
    _prefix, _width = None, 1

    def _plan(self, files, rfc, name, call, cuts=None, preroll=CUT_PREROLL, stride=None):
        """call(n, file pointers, lengths, info, out handle, cut arguments) -> the code of the plan function `name` (cut arguments
        None), or of its _cuts twin: (n_cuts, cut records, track_stride, cut info).  With cuts the batch's tracks are the cuts:
        n_files and info count them, `cut_info` holds their CUT_INFO_DTYPE records and n_sources the files."""
        self.lib = load_lib()
        self._files = [np.frombuffer(bytes(f) + b"\0", dtype=np.uint8) for f in files]  # (kept alive; + 1: never an empty buffer)
        n = len(self._files)
        ptrs = np.array([a.ctypes.data for a in self._files], dtype=np.uint64)
        lens = np.array([a.size - 1 for a in self._files], dtype=np.int64)
        if cuts is None:
            if stride:
                raise ValueError("stride needs cuts")
            self.cuts, self.cut_info, cut_args, n_tracks = None, None, None, n
        else:
            self.cuts = cut_records(cuts, preroll)
            n_tracks = self.cuts.size
            self.cut_info = np.zeros(n_tracks, dtype=CUT_INFO_DTYPE)
            cut_args = (n_tracks, self.cuts.ctypes.data, int(stride or 0), self.cut_info.ctypes.data)
        self.info = np.zeros(n_tracks, dtype=FILE_INFO_DTYPE)
        h = C.c_void_p()
        r = call(n, ptrs.ctypes.data, lens.ctypes.data, self.info.ctypes.data, C.byref(h), cut_args)
        if r != 0:
            e = OpusGpuError(f"{name}{'_cuts' if cut_args else ''} failed: {r}")
            e.code = r
            raise e
        self.h = h
        self.n_files, self.n_sources, self.rfc = n_tracks, n, bool(rfc)
        self.stride = int(stride or 0)
        self.row_samples = RFC_FRAME if rfc else FRAME
        self.n_steps = self._c("steps")(h)
        self.track_samples = self._c("track_samples")(h)
        nbytes = C.c_size_t()
        a = self._c("arena")(h, C.byref(nbytes))
        self.arena = np.ctypeslib.as_array((C.c_uint8 * nbytes.value).from_address(a)) if nbytes.value else np.zeros(0, np.uint8)

    def _c(self, name):
        return getattr(self.lib, f"{self._prefix}_{name}")

    def _step_tables(self, k, *more):
        """-> (descriptors, flat; file of every slot; segments): views, valid until close().  more: what the step call takes
        behind slot_files."""
        d, sf, sg = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = self._c("step")(self.h, k, C.byref(d), C.byref(sf), *more)
        if n < 0:
            raise IndexError(k)
        if n == 0:
            return np.zeros(0, DESC_DTYPE), np.zeros(0, np.int32), np.zeros(0, TRACK_SEG_DTYPE)
        self._c("segments")(self.h, k, C.byref(sg))
        descs = np.frombuffer((C.c_uint8 * (16 * n * self._width)).from_address(d.value), dtype=DESC_DTYPE)
        files = np.frombuffer((C.c_uint8 * (4 * n)).from_address(sf.value), dtype=np.int32)
        segs = np.frombuffer((C.c_uint8 * (32 * n)).from_address(sg.value), dtype=TRACK_SEG_DTYPE)
        return descs, files, segs

    def packet_start(self, file, packet_seq):
        """Planned start (track-relative sample) of a file's packet; packet_seq == its packet count: the planned length."""
        return self._c("packet_start")(self.h, file, packet_seq)

    def close(self):
        if self.h:
            self._c("free")(self.h)
            self.h = None
            self.arena = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FileBatch(_PlannedFiles):
    """Decode steps, packet arena and track segments planned from whole Ogg Opus files by opusgpu_files_plan (host only,
    include/opusgpu.h WHOLE FILES).  files: a list of bytes-like objects, file i = decoder stream i.  info: one FILE_INFO_DTYPE
    record per file (status, OpusHead fields, packets, frames, holes, planned track length and offset).
    cuts: None, or pieces of the files as the batch's tracks (cut_records says what they may be; include/opusgpu.h WHOLE FILES /
    CUTS): cut t = decoder stream t, n_files and info count the cuts, cut_info holds their CUT_INFO_DTYPE records, and the files are
    read once each.  preroll: for cuts that name none.  stride: None / 0 for packed tracks, else every track's distance."""
    _prefix = "opusgpu_file_batch"

    def __init__(self, files, channels=2, rfc=False, flags=0, threads=1, cuts=None, preroll=CUT_PREROLL, stride=None):
        self.channels = channels
        mode = 1 if rfc else 0

        def call(n, ptrs, lens, info, out, cut_args):
            if cut_args is None:
                return load_lib().opusgpu_files_plan(n, ptrs, lens, channels, mode, flags, threads, info, out)
            n_cuts, recs, track_stride, cut_info = cut_args
            return load_lib().opusgpu_files_plan_cuts(n, ptrs, lens, n_cuts, recs, track_stride, channels, mode, flags, threads, info, cut_info, out)
        self._plan(files, rfc, "opusgpu_files_plan", call, cuts, preroll, stride)

    def step(self, k):
        """-> (descriptors [DESC_DTYPE], file of every slot [int32], segments [TRACK_SEG_DTYPE], modes); views, valid until close()."""
        modes = C.c_int()
        return self._step_tables(k, C.byref(modes)) + (modes.value,)


def file_layout(data):
    """Host-only: the layout of one Ogg Opus file, read from its OpusHead (opusgpu_file_layout) -> ((channels, streams, coupled,
    mapping list), info [FILE_INFO_DTYPE record]).  Family 0 gives one stream and the identity mapping.  Raises OpusGpuError with
    the reader's code (or OPUSGPU_UNIMPLEMENTED for mapping family 255) when the file has no usable header."""
    lib = load_lib()
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    lay = MsLayout()
    info = np.zeros(1, dtype=FILE_INFO_DTYPE)
    r = lib.opusgpu_file_layout(buf.ctypes.data, buf.size - 1, C.byref(lay), info.ctypes.data)
    if r != 0:
        e = OpusGpuError(f"opusgpu_file_layout failed: {r}")
        e.code = r
        raise e
    return (lay.channels, lay.streams, lay.coupled, [lay.mapping[c] for c in range(lay.channels)]), info[0]


class MsFileBatch(_PlannedFiles):
    """Decode steps, packet arena and track segments planned from whole Ogg Opus files of ONE multistream layout by
    opusgpu_ms_files_plan (host only, include/opusgpu.h WHOLE FILES / MULTISTREAM).  files: a list of bytes-like objects, file i =
    decoder i; layout: (channels, streams, coupled, mapping) or an MsLayout.  A step is rows of `streams` descriptors, one row and
    one segment per file that has a frame in it.  cuts, preroll, stride: as for FileBatch."""
    _prefix = "opusgpu_ms_file_batch"

    def __init__(self, files, layout, rfc=False, threads=1, cuts=None, preroll=CUT_PREROLL, stride=None):
        self.layout = layout if isinstance(layout, MsLayout) else ms_layout(*layout)
        self.channels, self.streams = int(self.layout.channels), int(self.layout.streams)
        self._width = self.streams
        mode = 1 if rfc else 0

        def call(n, ptrs, lens, info, out, cut_args):
            if cut_args is None:
                return load_lib().opusgpu_ms_files_plan(n, ptrs, lens, C.byref(self.layout), mode, threads, info, out)
            n_cuts, recs, track_stride, cut_info = cut_args
            return load_lib().opusgpu_ms_files_plan_cuts(n, ptrs, lens, n_cuts, recs, track_stride, C.byref(self.layout), mode, threads, info,
                                                         cut_info, out)
        self._plan(files, rfc, "opusgpu_ms_files_plan", call, cuts, preroll, stride)

    def step(self, k):
        """-> (descriptors [rows, streams] of DESC_DTYPE, file of every row [int32], segments [TRACK_SEG_DTYPE]); views, valid
        until close()."""
        descs, files, segs = self._step_tables(k)
        return descs.reshape(-1, self.streams), files, segs


def head_gain_scale(output_gain_q8):
    """opusgpu_head_gain_scale: an OpusHead output gain (Q7.8 dB) as the linear factor of the float track formats, 1 / 32768 folded in."""
    return np.float32(load_lib().opusgpu_head_gain_scale(int(output_gain_q8)))


def track_format_args(batch, format="s16", scale=None, out=None, device=0):
    """What decode_files makes of its format=, scale= and out= for a planned batch, before any device work: -> (OPUSGPU_TRACKS_*
    value, float32 scale array or None, out flattened or None).  Raises ValueError for a format that does not exist, a scale with
    "s16" or of the wrong length or not finite, and an `out` that is not a contiguous torch tensor on GPU `device`, of the format's
    dtype, 128-byte aligned, with at least track_samples * channels elements."""
    if format not in TRACK_FORMATS:
        raise ValueError(f"format must be one of {sorted(TRACK_FORMATS)}, not {format!r}")
    fmt = TRACK_FORMATS[format]
    if scale is not None:
        if fmt == TRACKS_S16:
            raise ValueError("scale needs a float format: int16 tracks are not scaled")
        if isinstance(scale, str):
            if scale != "head_gain":
                raise ValueError(f"scale must be None, 'head_gain' or an array, not {scale!r}")
            scale = [head_gain_scale(g) for g in batch.info["output_gain"]]
        scale = np.ascontiguousarray(scale, dtype=np.float32)
        if scale.shape != (batch.n_files,):
            raise ValueError(f"scale must have one entry per file ({batch.n_files}), not shape {scale.shape}")
        if not np.isfinite(scale).all():
            raise ValueError("scale entries must be finite")
    if out is not None:
        out = _out_flat(out, max(int(batch.track_samples), 1) * batch.channels, format, device)
    return fmt, scale, out


def _out_flat(out, need, format, device):
    """decode_files' `out` for tracks of `format` that take `need` elements, flattened; ValueError if it does not fit."""
    dtype = "torch.int16" if TRACK_FORMATS[format] == TRACKS_S16 else "torch.float32"
    if not hasattr(out, "data_ptr") or not hasattr(out, "is_cuda"):
        raise ValueError("out must be a torch tensor")
    if not out.is_cuda or out.device.index != device:
        raise ValueError(f"out must be on GPU {device}, not on {out.device}")
    if str(out.dtype) != dtype:
        raise ValueError(f"out must be of dtype {dtype} for format {format!r}, not {out.dtype}")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")
    if out.numel() < need:
        raise ValueError(f"out is too small: {out.numel()} elements, {need} needed")
    if out.data_ptr() % 128:
        raise ValueError("out must be 128-byte aligned")
    return out.view(-1)


def _tables(name, ctype, args, count, refused):
    """What a table accessor of the library hands out: `name`(*args, `count` pointers out) -> copies of the `count` arrays of
    `ctype`, flat; ValueError(refused) where the call refuses."""
    ptrs = [C.c_void_p() for _ in range(count)]
    n = getattr(load_lib(), name)(*args, *(C.byref(p) for p in ptrs))
    if n < 0:
        raise ValueError(refused)
    return [np.ctypeslib.as_array((ctype * n).from_address(p.value)).copy() for p in ptrs]


def _layout(name, planned_samples, args, refused):
    """A layout call of the library: `name`(n, planned, *args, offsets out) -> (planned [int64], offsets [int64], total);
    ValueError where the call refuses."""
    planned = np.ascontiguousarray(planned_samples, dtype=np.int64)
    offsets = np.zeros(planned.size, dtype=np.int64)
    total = getattr(load_lib(), name)(planned.size, planned.ctypes.data, *args, offsets.ctypes.data)
    if total < 0:
        raise ValueError(f"{name} refused {refused}")
    return planned, offsets, int(total)


def resample_taps(rate):
    """opusgpu_resample_taps: the Q15 decimation taps of `rate` (24000, 16000, 12000, 8000) as an int16 array of 24 D + 1."""
    return _tables("opusgpu_resample_taps", C.c_int16, (int(rate),), 1, f"no taps for rate {rate!r}")[0]


def resample_layout(planned_samples, rate):
    """opusgpu_resample_layout: the grid of the resampled tracks -> (out_offsets [int64], total samples per channel)."""
    return _layout("opusgpu_resample_layout", planned_samples, (int(rate),), f"rate {rate!r} or a negative length")[1:]


def track_rate_args(batch, rate=48000, mono=False, format="s16", out=None, device=0, allow_mono=True):
    """What decode_files makes of its rate= and mono= for a planned batch, before any device work: None for the defaults (today's
    path), else (D, output channels, out_offsets, total samples per channel, out flattened or None).  Raises ValueError for a rate
    that does not exist, 48000 without mono, mono with more than 2 channels (or where there is no mono: allow_mono False), and an
    `out` that does not fit the RESAMPLED tracks: total * output channels elements, otherwise as track_format_args says."""
    if mono and not allow_mono:
        raise ValueError("there is no mono downmix of multistream tracks")
    if rate == 48000 and not mono:
        return None
    if rate not in TRACK_RATES:
        raise ValueError(f"rate must be one of {sorted(TRACK_RATES)}, not {rate!r}")
    if mono and batch.channels > 2:
        raise ValueError(f"mono needs 1 or 2 channels, not {batch.channels}")
    if format not in TRACK_FORMATS:
        raise ValueError(f"format must be one of {sorted(TRACK_FORMATS)}, not {format!r}")
    ch_out = 1 if mono else batch.channels
    offsets, total = resample_layout(batch.info["track_samples"], rate)
    if out is not None:
        out = _out_flat(out, max(total, 1) * ch_out, format, device)
    return TRACK_RATES[rate], ch_out, offsets, total, out


def track_ratio(resample):
    """A resample= argument as its reduced (up, down) (include/opusgpu.h TRACK RATIOS): a pair (up, down) as for
    scipy.signal.resample_poly, or the output rate as an int, which is reduced against 48000 -- 44100 is (147, 160).  Raises
    ValueError for anything else and for a ratio outside 1 <= up <= 160, up < down <= min(8 up, 640)."""
    import math
    import numbers
    if isinstance(resample, numbers.Integral) and not isinstance(resample, bool):
        pair = (int(resample), 48000)
    else:
        try:
            pair = tuple(resample)
        except TypeError:
            pair = ()
        if len(pair) != 2 or not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in pair):
            raise ValueError(f"resample must be (up, down) or an output rate in Hz as an int, not {resample!r}")
    up, down = int(pair[0]), int(pair[1])
    if up < 1 or down < 1:
        raise ValueError(f"resample must be positive, not {resample!r}")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if not (up <= 160 and up < down <= min(8 * up, 640)):
        raise ValueError(f"resample {resample!r} is {up}/{down}: outside 1 <= up <= 160, up < down <= min(8 up, 640)")
    return up, down


def resample_ratio_taps(up, down):
    """opusgpu_resample_ratio_taps: the Q15 taps of up / down as an int16 array of 24 down' + 1, down' the reduced down."""
    return _tables("opusgpu_resample_ratio_taps", C.c_int16, (int(up), int(down)), 1, f"no taps for the ratio {up!r}/{down!r}")[0]


def resample_ratio_layout(planned_samples, up, down):
    """opusgpu_resample_ratio_layout: the grid of the tracks at up / down -> (out_offsets [int64], total samples per channel)."""
    return _layout("opusgpu_resample_ratio_layout", planned_samples, (int(up), int(down)),
                   f"the ratio {up!r}/{down!r} or a negative length")[1:]


def _channel_mix(batch, mono, mix, allow_mono, one=False):
    """What mono= and mix= make of the channels of a planned batch: the matrix record of a mix, None for mono or all channels.
    one: the result must be ONE channel (features).  Raises ValueError for mono where there is none (allow_mono False) or on more
    than 2 channels, mono together with a mix, what mix_matrix refuses, and with `one` for neither and for a mix of more rows."""
    if mono and not allow_mono:
        raise ValueError("there is no mono downmix of multistream tracks: use mix='mono'")
    if mix is not None and mono:
        raise ValueError("mix and mono=True exclude each other: the row {8192, 8192} is mono")
    if one and mix is None and not mono:
        raise ValueError("features are made of ONE channel: pass mono=True or a mix of one row (mix='mono')")
    rec = None if mix is None else mix_matrix(mix, batch.channels)
    if one and rec is not None and int(rec["out_channels"][0]) != 1:
        raise ValueError(f"features are made of ONE channel: the mix has {int(rec['out_channels'][0])} rows")
    if mono and batch.channels > 2:
        raise ValueError(f"mono needs 1 or 2 channels, not {batch.channels}")
    return rec


def track_ratio_args(batch, resample, mono=False, mix=None, format="s16", out=None, device=0, allow_mono=True, rate=None, features=None):
    """What decode_files makes of its resample= for a planned batch, before any device work: ((up, down) reduced, output channels,
    out_offsets, total samples per channel, out flattened or None, the matrix record or None).  Raises ValueError for what
    track_ratio and mix_matrix refuse, resample= together with a rate= (other than None) or with features=, mono together with a mix,
    mono with more than 2 channels (or where there is no mono: allow_mono False), a format that does not exist, and an `out` that
    does not fit the RESAMPLED tracks: total * output channels elements, otherwise as track_format_args says."""
    if rate is not None:
        raise ValueError("resample= and rate= exclude each other")
    if features is not None:
        raise ValueError("features are made of the track at 16000 Hz: there is no resample= with them")
    up, down = track_ratio(resample)
    rec = _channel_mix(batch, mono, mix, allow_mono)
    if format not in TRACK_FORMATS:
        raise ValueError(f"format must be one of {sorted(TRACK_FORMATS)}, not {format!r}")
    ch_out = int(rec["out_channels"][0]) if rec is not None else 1 if mono else batch.channels
    offsets, total = resample_ratio_layout(batch.info["track_samples"], up, down)
    if out is not None:
        out = _out_flat(out, max(total, 1) * ch_out, format, device)
    return (up, down), ch_out, offsets, total, out, rec


def downmix_matrix(channels, out_channels):
    """opusgpu_downmix_matrix: the default table that takes `channels` (1 - 8, Vorbis order) to 2 or 1 -> int16 [out, in], Q14."""
    rec = np.zeros(1, dtype=MIX_MATRIX_DTYPE)
    if load_lib().opusgpu_downmix_matrix(int(channels), int(out_channels), rec.ctypes.data) != 0:
        raise ValueError(f"there is no default downmix of {channels!r} channels to {out_channels!r}")
    return rec["m"][0, :out_channels, :channels].copy()


def mix_matrix(mix, channels):
    """A `mix` argument for tracks of `channels` channels as its opusgpu_mix_matrix record (a MIX_MATRIX_DTYPE array of one).
    mix: "mono" or "stereo" (the default table), an integer array [out, in] taken as Q14, or a float array converted by
    np.rint(a * 16384).  Raises ValueError for what CHANNEL MIX refuses and for a float array that leaves int16."""
    if isinstance(mix, str):
        if mix not in ("mono", "stereo"):
            raise ValueError(f"mix must be 'mono', 'stereo' or a matrix, not {mix!r}")
        m = downmix_matrix(channels, 1 if mix == "mono" else 2)
    else:
        m = np.asarray(mix)
        if m.ndim != 2 or m.dtype.kind not in "iuf":
            raise ValueError(f"mix must be a matrix [out_channels, in_channels] of numbers, not shape {m.shape} of {m.dtype}")
        if m.dtype.kind == "f":
            if not np.isfinite(m).all():
                raise ValueError("mix entries must be finite")
            m = np.rint(m.astype(np.float64) * 16384)
        if m.size and (m.min() < -32768 or m.max() > 32767):
            raise ValueError("mix entries must fit int16 in Q14: [-2, 2)")
        m = m.astype(np.int16)
    co, ci = m.shape
    if not 1 <= co <= 8 or not 1 <= ci <= 8:
        raise ValueError(f"mix must have 1 - 8 rows and columns, not {m.shape}")
    if ci != channels:
        raise ValueError(f"mix has {ci} columns for tracks of {channels} channels")
    if np.abs(m.astype(np.int64)).sum(axis=1).max() > 65535:
        raise ValueError("a row of mix has sum |M| > 65535 in Q14: the int32 sum would not be exact")
    rec = np.zeros(1, dtype=MIX_MATRIX_DTYPE)
    rec["out_channels"], rec["in_channels"] = co, ci
    rec["m"][0, :co, :ci] = m
    return rec


def track_mix_args(batch, mix, rate=48000, format="s16", out=None, device=0):
    """What decode_files makes of its mix= (and rate=) for a planned batch, before any device work: (D, output channels, out_offsets,
    total samples per channel, out flattened or None, the matrix record).  Raises ValueError for what mix_matrix refuses, a rate or
    format that does not exist, and an `out` that does not fit the MIXED tracks: total * out_channels elements."""
    rec = mix_matrix(mix, batch.channels)
    if rate not in TRACK_RATES:
        raise ValueError(f"rate must be one of {sorted(TRACK_RATES)}, not {rate!r}")
    if format not in TRACK_FORMATS:
        raise ValueError(f"format must be one of {sorted(TRACK_FORMATS)}, not {format!r}")
    ch_out = int(rec["out_channels"][0])
    offsets, total = resample_layout(batch.info["track_samples"], rate)
    if out is not None:
        out = _out_flat(out, max(total, 1) * ch_out, format, device)
    return TRACK_RATES[rate], ch_out, offsets, total, out, rec


def mel_params(n_mels=80, feature_layout="bands"):
    """An opusgpu_mel_params record (a MEL_PARAMS_DTYPE array of one).  feature_layout: "bands" ([n_mels, frames]) or "frames"
    ([frames, n_mels]), or the OPUSGPU_MEL_* value.  Raises ValueError for an n_mels other than 80 or 128 and an unknown layout."""
    if n_mels not in (80, 128):
        raise ValueError(f"n_mels must be 80 or 128, not {n_mels!r}")
    lay = MEL_LAYOUTS.get(feature_layout, feature_layout) if isinstance(feature_layout, str) else feature_layout
    if lay not in (MEL_BANDS_MAJOR, MEL_FRAMES_MAJOR) or isinstance(lay, bool):
        raise ValueError(f"feature_layout must be one of {sorted(MEL_LAYOUTS)}, not {feature_layout!r}")
    rec = np.zeros(1, dtype=MEL_PARAMS_DTYPE)
    rec["n_mels"], rec["layout"] = n_mels, lay
    return rec


def mel_basis():
    """opusgpu_mel_basis: the windowed DFT basis the kernel multiplies -> (Wc, Ws), float32 [400, 201] each."""
    return tuple(a.reshape(MEL_NFFT, MEL_BINS) for a in _tables("opusgpu_mel_basis", C.c_float, (), 2, None))


def mel_filterbank(n_mels):
    """opusgpu_mel_filterbank: the Slaney filterbank of 80 or 128 bands -> float32 [n_mels, 201]."""
    bank = _tables("opusgpu_mel_filterbank", C.c_float, (int(n_mels),), 1, f"n_mels must be 80 or 128, not {n_mels!r}")[0]
    return bank.reshape(int(n_mels), MEL_BINS)


def mel_layout(planned_48k_samples, n_mels=80, feature_layout="bands"):
    """opusgpu_mel_layout: the grid of the feature tracks -> (feat_offsets [int64], planes [int64], total floats)."""
    rec = mel_params(n_mels, feature_layout)
    planned, offsets, total = _layout("opusgpu_mel_layout", planned_48k_samples, (rec.ctypes.data,), "a negative length")
    return offsets, ((planned + 2) // 3 // MEL_HOP + 63) // 64 * 64, total


def track_feature_args(batch, features=None, n_mels=80, feature_layout="bands", rate=None, mono=False, mix=None, format=None, scale=None,
                       out=None, device=0, allow_mono=True):
    """What decode_files makes of its features= for a planned batch, before any device work: None for features=None (today's
    paths), else (params record, mix record or None, float32 scale array or None, feat_offsets, planes, total floats, out flattened
    or None).  Raises ValueError for a feature other than "logmel", what mel_params refuses, a rate other than 16000 (or None), a
    format other than "f32" (or None), a result of more than one channel -- neither mono=True nor a mix, both, a mix of more than
    one row, mono on more than 2 channels or where there is none (allow_mono False) --, a scale of the wrong length or not finite,
    and an `out` that does not fit the feature tracks: total floats, otherwise as track_format_args says."""
    if features is None:
        return None
    if features != "logmel":
        raise ValueError(f"features must be None or 'logmel', not {features!r}")
    rec = mel_params(n_mels, feature_layout)
    if rate not in (None, MEL_SR):
        raise ValueError(f"features are made of the track at {MEL_SR} Hz: rate must be absent or {MEL_SR}, not {rate!r}")
    if format not in (None, "f32"):
        raise ValueError(f"features are float32: format must be absent or 'f32', not {format!r}")
    mrec = _channel_mix(batch, mono, mix, allow_mono, one=True)
    _, scale, _ = track_format_args(batch, "f32", scale, None, device)
    offsets, planes, total = mel_layout(batch.info["track_samples"], n_mels, feature_layout)
    if out is not None:
        out = _out_flat(out, max(total, 1), "f32", device)
    return rec, mrec, scale, offsets, planes, total, out


def mel_spec(sample_rate, n_fft, hop, win_length=None, n_mels=80, fmin=0.0, fmax=None, mel_scale="slaney", norm="slaney", power=2,
             log="log10", floor=1e-10, frames="torch", feature_layout="bands", algo="dense"):
    """An opusgpu_spec_params record (a SPEC_PARAMS_DTYPE array of one; include/opusgpu.h TRACK SPECTROGRAMS): the numbers that
    torchaudio's MelSpectrogram and librosa's melspectrogram take.  win_length None is n_fft, fmax None is sample_rate / 2; mel_scale
    "slaney" or "htk"; norm "slaney" or None; power 1 or 2; log "log10", "ln" or None; frames "torch" (n // hop + 1) or "whisper"
    (n // hop); feature_layout as for mel_params; algo "dense" (the DFT on the matrix cores, n_fft up to 2048) or "fft" (n_fft a
    power of two in [64, 8192], any hop in [1, n_fft]).  Raises ValueError for what the record's rules refuse."""
    import numbers

    def whole(name, v):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool):
            raise ValueError(f"{name} must be an int, not {v!r}")
        return int(v)
    sample_rate, n_fft, hop, n_mels = whole("sample_rate", sample_rate), whole("n_fft", n_fft), whole("hop", hop), whole("n_mels", n_mels)
    win = n_fft if win_length is None else whole("win_length", win_length)
    if not isinstance(algo, str) or algo not in SPEC_ALGOS:
        raise ValueError(f"algo must be one of {sorted(SPEC_ALGOS)}, not {algo!r}")
    if not 1 <= sample_rate <= 1048576:
        raise ValueError(f"sample_rate must be in [1, 1048576], not {sample_rate}")
    if algo == "fft":
        if not 64 <= n_fft <= 8192 or n_fft & (n_fft - 1):
            raise ValueError(f"n_fft must be a power of two in [64, 8192] with algo='fft', not {n_fft}")
    elif not 64 <= n_fft <= 2048 or n_fft % 16:
        raise ValueError(f"n_fft must be a multiple of 16 in [64, 2048], not {n_fft}")
    if not 16 <= win <= n_fft or win % 2:
        raise ValueError(f"win_length must be even and in [16, n_fft], not {win}")
    if algo == "fft":
        if not 1 <= hop <= n_fft:
            raise ValueError(f"hop must be in [1, n_fft] with algo='fft', not {hop}")
    elif not 1 <= hop <= n_fft or 31 * hop + n_fft > 32768:
        raise ValueError(f"hop must be in [1, n_fft] with 31 * hop + n_fft <= 32768, not {hop}")
    if not 1 <= n_mels <= 128:
        raise ValueError(f"n_mels must be in [1, 128], not {n_mels}")
    for name, v, table in (("mel_scale", mel_scale, SPEC_SCALES), ("norm", norm, SPEC_NORMS), ("log", log, SPEC_LOGS), ("frames", frames, SPEC_FRAMES),
                           ("feature_layout", feature_layout, MEL_LAYOUTS)):
        if not isinstance(v, (str, type(None))) or v not in table:
            raise ValueError(f"{name} must be one of {sorted(table, key=str)}, not {v!r}")
    if power not in (1, 2) or isinstance(power, bool):
        raise ValueError(f"power must be 1 or 2, not {power!r}")
    rec = np.zeros(1, dtype=SPEC_PARAMS_DTYPE)
    rec["sample_rate"], rec["n_fft"], rec["win_length"], rec["hop"], rec["n_mels"] = sample_rate, n_fft, win, hop, n_mels
    rec["mel_scale"], rec["norm"], rec["power"], rec["log"] = SPEC_SCALES[mel_scale], SPEC_NORMS[norm], int(power), SPEC_LOGS[log]
    rec["frames"], rec["layout"] = SPEC_FRAMES[frames], MEL_LAYOUTS[feature_layout]
    rec["reserved"][0, 1] = SPEC_ALGOS[algo]
    try:
        rec["fmin"], rec["fmax"], rec["floor"] = float(fmin), sample_rate / 2 if fmax is None else float(fmax), float(floor)
    except (TypeError, ValueError):
        raise ValueError(f"fmin, fmax and floor must be numbers, not {fmin!r}, {fmax!r}, {floor!r}") from None
    fmin32, fmax32, floor32 = float(rec["fmin"][0]), float(rec["fmax"][0]), float(rec["floor"][0])
    if not (0 <= fmin32 < fmax32 <= sample_rate / 2):
        raise ValueError(f"0 <= fmin < fmax <= sample_rate / 2 must hold, not fmin {fmin!r}, fmax {fmax!r}")
    if not np.isfinite(floor32) or floor32 < 0 or (rec["log"][0] and not floor32 > 0):
        raise ValueError(f"floor must be finite and >= 0, and > 0 with a log, not {floor!r}")
    return rec


def _record(rec, dtype, what):
    """A parameter record as the library takes it: one contiguous element of `dtype`; ValueError(what) for anything else."""
    if getattr(rec, "dtype", None) != dtype or np.size(rec) != 1:
        raise ValueError(what)
    return np.ascontiguousarray(rec).reshape(1)


# (dtype, what) of the three records, as _record takes them
_SPEC = (SPEC_PARAMS_DTYPE, "a spectrogram's parameters are a mel_spec() record")
_STFT = (STFT_PARAMS_DTYPE, "an STFT's parameters are a stft_spec() record")
_FBANK = (FBANK_PARAMS_DTYPE, "Kaldi features' parameters are a kaldi_fbank() or kaldi_mfcc() record")


# The calls that mel_spec and stft_spec records share, keyed by the C symbol, for a checked record.
def _record_basis(name, rec):
    tables = _tables(name, C.c_float, (rec.ctypes.data,), 2, f"{name} refused the record")
    return tuple(a.reshape(int(rec["n_fft"][0]), -1) for a in tables)


def _record_fft_tables(name, rec):
    window, twiddle = _tables(name, C.c_float, (rec.ctypes.data,), 2, f"{name} refused the record")
    return window, twiddle.reshape(-1, 2)


def _record_tile(name, rec):
    T = getattr(load_lib(), name)(rec.ctypes.data)
    if T < 0:
        raise ValueError(f"{name} refused the record")
    return int(T)


def _centered_frames(rec, samples):
    n, hop = np.asarray(samples, dtype=np.int64), int(rec["hop"][0])
    return n // hop if int(rec["frames"][0]) == SPEC_FRAMES["whisper"] else np.where(n > 0, n // hop + 1, 0)


def _record_layout(name, planned_48k_samples, up, down, rec, frames):
    """opusgpu_spec_layout / opusgpu_stft_layout / opusgpu_fbank_layout for a checked record whose F is frames(rec, samples)."""
    planned, offsets, total = _layout(name, planned_48k_samples, (int(up), int(down), rec.ctypes.data),
                                      f"the record, the ratio {up!r}/{down!r} or a negative length")
    return offsets, (frames(rec, -(-planned * int(up) // int(down))) + 63) // 64 * 64, total


def spec_basis(rec):
    """opusgpu_spec_basis: the windowed DFT basis of a mel_spec record -> (Wc, Ws), float32 [n_fft, n_fft / 2 + 1] each.  Raises
    ValueError for an algo="fft" record: there is no dense basis behind one (spec_fft_tables has its tables)."""
    return _record_basis("opusgpu_spec_basis", _record(rec, *_SPEC))


def spec_filterbank(rec):
    """opusgpu_spec_filterbank: the filterbank of a mel_spec record -> float32 [n_mels, n_fft / 2 + 1]."""
    rec = _record(rec, *_SPEC)
    bank = _tables("opusgpu_spec_filterbank", C.c_float, (rec.ctypes.data,), 1, "opusgpu_spec_filterbank refused the record")[0]
    return bank.reshape(int(rec["n_mels"][0]), -1)


def spec_fft_tables(rec):
    """opusgpu_spec_fft_tables: the tables of a mel_spec(algo="fft") record, which are stft_fft_tables' for the same n_fft and
    win_length -> (window [n_fft], twiddle [n_fft / 2, 2]: cos and sin of 2 pi j / n_fft), float32."""
    return _record_fft_tables("opusgpu_spec_fft_tables", _record(rec, *_SPEC))


def spec_tile(rec):
    """opusgpu_spec_tile: the frames of a tile for a mel_spec record: of k_tracks_melspec 128, 64 or 32, of k_tracks_melfft
    (algo="fft") the larger of 32 and 8192 / n_fft."""
    return _record_tile("opusgpu_spec_tile", _record(rec, *_SPEC))


def spec_frames(rec, samples):
    """F of TRACK SPECTROGRAMS for tracks of `samples` samples at the record's rate."""
    return _centered_frames(_record(rec, *_SPEC), samples)


def spec_layout(planned_48k_samples, up, down, rec):
    """opusgpu_spec_layout: the grid of the spectrograms of tracks at up / down of 48 kHz -> (feat_offsets [int64], planes [int64],
    total floats)."""
    return _record_layout("opusgpu_spec_layout", planned_48k_samples, up, down, _record(rec, *_SPEC), _centered_frames)


def track_spectrogram_args(batch, features, rate=None, resample=None, mono=False, mix=None, format=None, scale=None, out=None, device=0,
                           allow_mono=True):
    """What decode_files makes of a mel_spec record as its features= for a planned batch, before any device work: (record, mix record
    or None, float32 scale array or None, feat_offsets, planes, total floats, out flattened or None, (rate or 0, up, down) as the C
    call takes them).  rate= names a rate of TRACK RATES, resample= a ratio of TRACK RATIOS; with neither, the record's sample_rate
    is taken as the one or the other.  Raises ValueError for a record that breaks a rule, both rate= and resample=, a rate or ratio
    that does not exist or is not the record's sample_rate, and for what track_feature_args refuses of format, mono, mix, scale and
    out."""
    return _record_feature_args(batch, _record(features, *_SPEC), spec_layout, rate, resample, mono, mix, format, scale, out, device, allow_mono)


def _record_feature_args(batch, rec, layout, rate, resample, mono, mix, format, scale, out, device, allow_mono):
    """track_spectrogram_args and track_kaldi_args behind their record checks: layout(planned, up, down, rec) is the record's grid."""
    sr = int(rec["sample_rate"][0])
    if rate is not None and resample is not None:
        raise ValueError("resample= and rate= exclude each other")
    if rate is None and resample is None:
        rate, resample = (sr, None) if sr in TRACK_RATES else (None, sr)
    if rate is not None:
        if rate not in TRACK_RATES:
            raise ValueError(f"rate must be one of {sorted(TRACK_RATES)}, not {rate!r}")
        how, up, down = (int(rate), 0, 0), 1, TRACK_RATES[rate]
    else:
        up, down = track_ratio(resample)
        how = (0, up, down)
    if sr * down != 48000 * up:
        raise ValueError(f"the record's sample_rate {sr} is not the track's rate, 48000 * {up} / {down}")
    if format not in (None, "f32"):
        raise ValueError(f"features are float32: format must be absent or 'f32', not {format!r}")
    mrec = _channel_mix(batch, mono, mix, allow_mono, one=True)
    _, scale, _ = track_format_args(batch, "f32", scale, None, device)
    offsets, planes, total = layout(batch.info["track_samples"], up, down, rec)
    if out is not None:
        out = _out_flat(out, max(total, 1), "f32", device)
    return rec, mrec, scale, offsets, planes, total, out, how


def stft_spec(sample_rate, n_fft, hop, win_length=None, power=2, log=None, floor=0.0, frames="torch", feature_layout="bands", algo="dense"):
    """An opusgpu_stft_params record (an STFT_PARAMS_DTYPE array of one; include/opusgpu.h TRACK STFT): the numbers that
    torchaudio's Spectrogram and torch.stft take.  win_length None is n_fft; power 2 (Re^2 + Im^2), 1 (its square root) or None: the
    complex STFT, with torch.stft's sign; log "log10", "ln" or None, over `floor`; frames "torch" (n // hop + 1) or "whisper"
    (n // hop); feature_layout "bands" ([bins, frames]) or "frames" ([frames, bins]); algo "dense" (the DFT on the matrix cores,
    n_fft up to 2048) or "fft" (n_fft a power of two in [64, 8192], any hop in [1, n_fft]).  Raises ValueError for what the record's
    rules refuse."""
    import numbers

    def whole(name, v):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool):
            raise ValueError(f"{name} must be an int, not {v!r}")
        return int(v)
    sample_rate, n_fft, hop = whole("sample_rate", sample_rate), whole("n_fft", n_fft), whole("hop", hop)
    win = n_fft if win_length is None else whole("win_length", win_length)
    if not isinstance(algo, str) or algo not in STFT_ALGOS:
        raise ValueError(f"algo must be one of {sorted(STFT_ALGOS)}, not {algo!r}")
    if not 1 <= sample_rate <= 1048576:
        raise ValueError(f"sample_rate must be in [1, 1048576], not {sample_rate}")
    if algo == "fft":
        if not 64 <= n_fft <= 8192 or n_fft & (n_fft - 1):
            raise ValueError(f"n_fft must be a power of two in [64, 8192] with algo='fft', not {n_fft}")
    elif not 64 <= n_fft <= 2048 or n_fft % 16:
        raise ValueError(f"n_fft must be a multiple of 16 in [64, 2048], not {n_fft}")
    if not 16 <= win <= n_fft or win % 2:
        raise ValueError(f"win_length must be even and in [16, n_fft], not {win}")
    if algo == "fft":
        if not 1 <= hop <= n_fft:
            raise ValueError(f"hop must be in [1, n_fft] with algo='fft', not {hop}")
    elif not 1 <= hop <= n_fft or 31 * hop + n_fft > 32768:
        raise ValueError(f"hop must be in [1, n_fft] with 31 * hop + n_fft <= 32768, not {hop}")
    for name, v, table in (("log", log, SPEC_LOGS), ("frames", frames, SPEC_FRAMES), ("feature_layout", feature_layout, MEL_LAYOUTS)):
        if not isinstance(v, (str, type(None))) or v not in table:
            raise ValueError(f"{name} must be one of {sorted(table, key=str)}, not {v!r}")
    if power is not None and (power not in (1, 2) or isinstance(power, bool)):
        raise ValueError(f"power must be 1, 2 or None (complex), not {power!r}")
    if power is None and SPEC_LOGS[log]:
        raise ValueError("a complex STFT (power=None) has no log")
    rec = np.zeros(1, dtype=STFT_PARAMS_DTYPE)
    rec["sample_rate"], rec["n_fft"], rec["win_length"], rec["hop"] = sample_rate, n_fft, win, hop
    rec["power"], rec["log"] = STFT_COMPLEX if power is None else int(power), SPEC_LOGS[log]
    rec["frames"], rec["layout"] = SPEC_FRAMES[frames], MEL_LAYOUTS[feature_layout]
    rec["reserved"][0, 1] = STFT_ALGOS[algo]
    try:
        rec["floor"] = float(floor)
    except (TypeError, ValueError):
        raise ValueError(f"floor must be a number, not {floor!r}") from None
    floor32 = float(rec["floor"][0])
    if not np.isfinite(floor32) or floor32 < 0 or (rec["log"][0] and not floor32 > 0):
        raise ValueError(f"floor must be finite and >= 0, and > 0 with a log, not {floor!r}")
    return rec


def stft_basis(rec):
    """opusgpu_stft_basis: the windowed DFT basis of a stft_spec record -> (Wc, Ws), float32 [n_fft, n_fft / 2 + 1] each;
    Im = -(frame @ Ws)."""
    return _record_basis("opusgpu_stft_basis", _record(rec, *_STFT))


def stft_fft_tables(rec):
    """opusgpu_stft_fft_tables: the tables of a stft_spec(algo="fft") record -> (window [n_fft], twiddle [n_fft / 2, 2]: cos and sin
    of 2 pi j / n_fft), float32."""
    return _record_fft_tables("opusgpu_stft_fft_tables", _record(rec, *_STFT))


def stft_tile(rec):
    """opusgpu_stft_tile: the frames of a tile for a stft_spec record: of k_tracks_stft 128, 64 or 32, of k_tracks_fft (algo="fft")
    the larger of 16 and 8192 / n_fft."""
    return _record_tile("opusgpu_stft_tile", _record(rec, *_STFT))


def stft_width(rec):
    """The floats of one frame of a stft_spec record: n_fft / 2 + 1 bins, twice that for the complex STFT."""
    rec = _record(rec, *_STFT)
    return (int(rec["n_fft"][0]) // 2 + 1) * (2 if int(rec["power"][0]) == STFT_COMPLEX else 1)


def stft_frames(rec, samples):
    """F of TRACK STFT for tracks of `samples` samples at the record's rate."""
    return _centered_frames(_record(rec, *_STFT), samples)


def stft_layout(planned_48k_samples, up, down, rec):
    """opusgpu_stft_layout: the grid of the STFT spectrograms of tracks at up / down of 48 kHz -> (feat_offsets [int64], planes
    [int64], total floats)."""
    return _record_layout("opusgpu_stft_layout", planned_48k_samples, up, down, _record(rec, *_STFT), _centered_frames)


def track_stft_args(batch, features, rate=None, resample=None, mono=False, mix=None, format=None, scale=None, out=None, device=0,
                    allow_mono=True):
    """track_spectrogram_args for a stft_spec record as decode_files' features=: the same tuple, the same refusals, with
    stft_layout's grid (total and the out= size are in floats: a complex cell is two)."""
    return _record_feature_args(batch, _record(features, *_STFT), stft_layout, rate, resample, mono, mix, format, scale, out, device, allow_mono)


def _kaldi_record(sample_rate, frame_length, frame_shift, num_mel_bins, low_freq, high_freq, preemphasis_coefficient, remove_dc_offset,
                  window_type, round_to_power_of_two, snip_edges, use_power, use_log_fbank, feature_layout, n_ceps, cepstral_lifter, rejected):
    import numbers
    not_offered = {  # keyword -> (the values that change nothing, why no other is taken)
        "dither": ((0,), "the features are a function of the track: there is no dither"),
        "use_energy": ((False,), "the energy coefficient is not offered"),
        "raw_energy": ((True,), "the energy coefficient is not offered"),
        "energy_floor": ((0, 1), "the energy coefficient is not offered"),
        "htk_compat": ((False,), "HTK's coefficient order is not offered"),
        "vtln_warp": ((1,), "VTLN warping is not offered"),
        "vtln_low": ((100,), "VTLN warping is not offered"),
        "vtln_high": ((-500,), "VTLN warping is not offered"),
        "subtract_mean": ((False,), "subtract_mean is one torch operation on the result"),
        "blackman_coeff": ((0.42,), "the Blackman window's coefficient is 0.42"),
        "channel": ((-1, 0), "the track is mono"),
        "min_duration": ((0,), "every track has its F frames"),
    }
    for name, v in rejected.items():
        if name not in not_offered:
            raise TypeError(f"unexpected keyword argument {name!r}")
        same, why = not_offered[name]
        if not isinstance(v, numbers.Real) or v not in same:
            raise ValueError(f"{name}={v!r}: {why}")

    def number(name, v):
        if not isinstance(v, numbers.Real) or isinstance(v, bool) or not np.isfinite(v):
            raise ValueError(f"{name} must be a finite number, not {v!r}")
        return float(v)

    def flag(name, v):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False, not {v!r}")
        return int(v)
    if not isinstance(sample_rate, numbers.Real) or isinstance(sample_rate, bool) or sample_rate != int(sample_rate):
        raise ValueError(f"sample_rate must be a whole number of Hz, not {sample_rate!r}")
    sr = int(sample_rate)
    if not 1 <= sr <= 1048576:
        raise ValueError(f"sample_rate must be in [1, 1048576], not {sr}")
    L, H = int(sr * 0.001 * number("frame_length", frame_length)), int(sr * 0.001 * number("frame_shift", frame_shift))  # as Kaldi does
    if not 2 <= L <= 2048:
        raise ValueError(f"frame_length must come to 2 .. 2048 samples, not {L}")
    if H < 1 or 31 * H + L > 32768:
        raise ValueError(f"frame_shift must come to >= 1 sample with 31 * frame_shift + frame_length <= 32768 samples, not {H}")
    N = 64
    while N < L:
        N *= 2
    if not flag("round_to_power_of_two", round_to_power_of_two):
        if L < 64 or L % 16:  # the frame itself is the FFT's length: taken where the kernel has that length
            raise ValueError(f"round_to_power_of_two=False needs a frame_length that is a multiple of 16 and >= 64 samples, not {L}")
        N = L
    if not isinstance(num_mel_bins, numbers.Integral) or isinstance(num_mel_bins, bool) or not 3 <= num_mel_bins <= 128:
        raise ValueError(f"num_mel_bins must be an int in [3, 128], not {num_mel_bins!r}")
    if not isinstance(n_ceps, numbers.Integral) or isinstance(n_ceps, bool) or not 0 <= n_ceps <= num_mel_bins:
        raise ValueError(f"num_ceps must be an int in [1, num_mel_bins], not {n_ceps!r}")
    if not isinstance(window_type, str) or window_type not in FBANK_WINDOWS:
        raise ValueError(f"window_type must be one of {sorted(FBANK_WINDOWS)}, not {window_type!r}")
    if not isinstance(feature_layout, str) or feature_layout not in MEL_LAYOUTS:
        raise ValueError(f"feature_layout must be one of {sorted(MEL_LAYOUTS)}, not {feature_layout!r}")
    rec = np.zeros(1, dtype=FBANK_PARAMS_DTYPE)
    rec["sample_rate"], rec["frame_length"], rec["frame_shift"], rec["n_fft"], rec["n_mels"], rec["n_ceps"] = sr, L, H, N, num_mel_bins, n_ceps
    rec["window"], rec["snip_edges"], rec["remove_dc"] = FBANK_WINDOWS[window_type], flag("snip_edges", snip_edges), flag("remove_dc_offset", remove_dc_offset)
    rec["power"], rec["log"] = 2 if flag("use_power", use_power) else 1, FBANK_LOG_LN if flag("use_log_fbank", use_log_fbank) else FBANK_LOG_NONE
    rec["layout"], rec["floor"] = MEL_LAYOUTS[feature_layout], FBANK_FLOOR
    rec["preemphasis"], rec["low_freq"], rec["high_freq"] = (number("preemphasis_coefficient", preemphasis_coefficient), number("low_freq", low_freq),
                                                             number("high_freq", high_freq))
    rec["cepstral_lifter"] = number("cepstral_lifter", cepstral_lifter)
    if not 0 <= float(rec["preemphasis"][0]) <= 1:
        raise ValueError(f"preemphasis_coefficient must be in [0, 1], not {preemphasis_coefficient!r}")
    low, high = float(rec["low_freq"][0]), float(rec["high_freq"][0])
    high = high if high > 0 else sr / 2 + high
    if not 0 <= low < high <= sr / 2:
        raise ValueError(f"0 <= low_freq < high_freq <= sample_rate / 2 must hold (high_freq <= 0 counts from there), not {low_freq!r}, {high_freq!r}")
    if float(rec["cepstral_lifter"][0]) < 0:
        raise ValueError(f"cepstral_lifter must be >= 0, not {cepstral_lifter!r}")
    return rec


def kaldi_fbank(sample_rate=16000, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0, high_freq=0.0,
                preemphasis_coefficient=0.97, remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, snip_edges=True,
                use_power=True, use_log_fbank=True, feature_layout="frames", **rejected):
    """An opusgpu_fbank_params record (a FBANK_PARAMS_DTYPE array of one; include/opusgpu.h TRACK KALDI FEATURES) from the arguments
    of Kaldi's compute-fbank-feats and torchaudio.compliance.kaldi.fbank, with their defaults.  frame_length and frame_shift are
    milliseconds and become samples as Kaldi does, int(sample_rate * 0.001 * ms); the floor is FLT_EPSILON.  Raises ValueError, with
    the reason, for what the record's rules refuse and for what is not offered: dither other than 0, use_energy=True, htk_compat=True,
    a vtln_warp other than 1, subtract_mean=True, another blackman_coeff."""
    return _kaldi_record(sample_rate, frame_length, frame_shift, num_mel_bins, low_freq, high_freq, preemphasis_coefficient, remove_dc_offset,
                         window_type, round_to_power_of_two, snip_edges, use_power, use_log_fbank, feature_layout, 0, 0.0, rejected)


def kaldi_mfcc(sample_rate=16000, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, low_freq=20.0, high_freq=0.0,
               preemphasis_coefficient=0.97, remove_dc_offset=True, window_type="povey", round_to_power_of_two=True, snip_edges=True,
               use_power=True, feature_layout="frames", num_ceps=13, cepstral_lifter=22.0, **rejected):
    """kaldi_fbank's record with n_ceps = num_ceps (1 .. num_mel_bins) and the lifter: Kaldi's compute-mfcc-feats and
    torchaudio.compliance.kaldi.mfcc without the energy coefficient (use_energy=False)."""
    import numbers
    if not isinstance(num_ceps, numbers.Integral) or isinstance(num_ceps, bool) or num_ceps < 1:
        raise ValueError(f"num_ceps must be an int in [1, num_mel_bins], not {num_ceps!r}")
    return _kaldi_record(sample_rate, frame_length, frame_shift, num_mel_bins, low_freq, high_freq, preemphasis_coefficient, remove_dc_offset,
                         window_type, round_to_power_of_two, snip_edges, use_power, True, feature_layout, num_ceps, cepstral_lifter, rejected)


def fbank_width(rec):
    """The feature width of a kaldi_fbank / kaldi_mfcc record: n_ceps when it is > 0, else n_mels."""
    rec = _record(rec, *_FBANK)
    return int(rec["n_ceps"][0]) or int(rec["n_mels"][0])


def fbank_window(rec):
    """opusgpu_fbank_window: the window of a kaldi_fbank / kaldi_mfcc record -> float32 [frame_length]."""
    rec = _record(rec, *_FBANK)
    return _tables("opusgpu_fbank_window", C.c_float, (rec.ctypes.data,), 1, "opusgpu_fbank_window refused the record")[0]


def fbank_filterbank(rec):
    """opusgpu_fbank_filterbank: the filterbank of a kaldi_fbank / kaldi_mfcc record -> float32 [n_mels, n_fft / 2]."""
    rec = _record(rec, *_FBANK)
    bank = _tables("opusgpu_fbank_filterbank", C.c_float, (rec.ctypes.data,), 1, "opusgpu_fbank_filterbank refused the record")[0]
    return bank.reshape(int(rec["n_mels"][0]), -1)


def fbank_dct(rec):
    """opusgpu_fbank_dct: the lifted DCT of a kaldi_mfcc record -> float32 [n_ceps, n_mels] ([0, n_mels] for a kaldi_fbank record)."""
    rec = _record(rec, *_FBANK)
    n = load_lib().opusgpu_fbank_dct(rec.ctypes.data, None)
    if n < 0:
        raise ValueError("opusgpu_fbank_dct refused the record")
    n_mels = int(rec["n_mels"][0])
    if n == 0:
        return np.zeros((0, n_mels), dtype=np.float32)
    return _tables("opusgpu_fbank_dct", C.c_float, (rec.ctypes.data,), 1, "opusgpu_fbank_dct refused the record")[0].reshape(-1, n_mels)


def fbank_frames(rec, samples):
    """F of TRACK KALDI FEATURES for tracks of `samples` samples at the record's rate."""
    rec = _record(rec, *_FBANK)
    n, L, H = np.asarray(samples, dtype=np.int64), int(rec["frame_length"][0]), int(rec["frame_shift"][0])
    if int(rec["snip_edges"][0]):
        return np.where(n < L, 0, 1 + (n - L) // H)
    return (n + H // 2) // H


def fbank_layout(planned_48k_samples, up, down, rec):
    """opusgpu_fbank_layout: the grid of the Kaldi features of tracks at up / down of 48 kHz -> (feat_offsets [int64], planes [int64],
    total floats)."""
    return _record_layout("opusgpu_fbank_layout", planned_48k_samples, up, down, _record(rec, *_FBANK), fbank_frames)


def track_kaldi_args(batch, features, rate=None, resample=None, mono=False, mix=None, format=None, scale=None, out=None, device=0,
                     allow_mono=True):
    """track_spectrogram_args for a kaldi_fbank / kaldi_mfcc record as decode_files' features=: the same tuple, the same refusals,
    with the record checked by the library (opusgpu_fbank_layout) and fbank_layout's grid.  scale= may also be one number for every
    track: scale=1.0 is Kaldi's convention of samples in the int16 range."""
    import numbers
    if isinstance(scale, numbers.Real) and not isinstance(scale, bool):
        scale = np.full(batch.n_files, scale, dtype=np.float32)
    return _record_feature_args(batch, _record(features, *_FBANK), fbank_layout, rate, resample, mono, mix, format, scale, out, device, allow_mono)


def loudness_weights(channels):
    """opusgpu_loudness_weights: the default BS.1770-4 channel weights of `channels` (1 - 8, Vorbis order) channels, float32."""
    w = np.zeros(8, dtype=np.float32)
    if load_lib().opusgpu_loudness_weights(int(channels), w.ctypes.data) != 0:
        raise ValueError(f"there are no loudness weights for {channels!r} channels")
    return w[:channels].copy()


def loudness_gain(record, target_lufs, peak_limit=1.0):
    """opusgpu_loudness_gain: the linear gain that takes a track with this LOUDNESS_DTYPE record to target_lufs, held to
    peak * gain <= peak_limit when peak_limit > 0; 1 for a track without loudness (lufs -inf).  A double."""
    rec = np.zeros(1, dtype=LOUDNESS_DTYPE)
    rec[0] = record
    return float(load_lib().opusgpu_loudness_gain(rec.ctypes.data, float(target_lufs), float(peak_limit)))


def loudness_request(batch, loudness=None, peak_limit=1.0, channel_weights=None):
    """What decode_files makes of its loudness=, peak_limit= and channel_weights= for a planned batch, before any device work: None
    for loudness=None (today's calls), else the opusgpu_loudness_req record (a LOUDNESS_REQ_DTYPE array of one).  Raises ValueError
    for a loudness that is neither "measure" nor a finite number, a peak_limit that is not finite, and weights that are not one
    finite number >= 0 per channel of the batch (or given without loudness=)."""
    import numbers
    if loudness is None:
        if channel_weights is not None:
            raise ValueError("channel_weights needs loudness=")
        return None
    rec = np.zeros(1, dtype=LOUDNESS_REQ_DTYPE)
    if isinstance(loudness, str):
        if loudness != "measure":
            raise ValueError(f"loudness must be None, 'measure' or a target in LUFS, not {loudness!r}")
        rec["mode"] = LOUDNESS_MEASURE
    else:
        if not isinstance(loudness, numbers.Real) or isinstance(loudness, bool) or not np.isfinite(loudness):
            raise ValueError(f"loudness must be None, 'measure' or a finite target in LUFS, not {loudness!r}")
        if not isinstance(peak_limit, numbers.Real) or isinstance(peak_limit, bool) or not np.isfinite(peak_limit):
            raise ValueError(f"peak_limit must be a finite number (<= 0: none), not {peak_limit!r}")
        rec["mode"], rec["target_lufs"], rec["peak_limit"] = LOUDNESS_NORMALIZE, loudness, peak_limit
    if channel_weights is not None:
        w = np.asarray(channel_weights, dtype=np.float64)
        if w.shape != (batch.channels,):
            raise ValueError(f"channel_weights must have one entry per channel ({batch.channels}), not shape {w.shape}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("channel_weights must be finite and >= 0")
        rec["n_weights"] = batch.channels
        rec["weights"][0, :batch.channels] = w
    return rec


class FeatureNorm(typing.NamedTuple):
    """feature_norm's record: a normalisation of FEATURE BATCHES with its numbers."""
    norm: int           # FEAT_NORM_*
    range: float = 8.0  # WHISPER: (max(x, m - range) + add) * mul
    add: float = 4.0
    mul: float = 0.25
    var_floor: float = 1e-20  # CMVN: the floor under the variance (Kaldi's)
    sub_vec: object = None    # AFFINE: (x - sub_vec[j]) * mul_vec[j], float32 arrays
    mul_vec: object = None


def feature_norm(kind, range=8.0, add=4.0, mul=0.25, var_floor=1e-20, sub=None, mul_vec=None):
    """A normalisation for decode_files' normalize= with numbers of its own (include/opusgpu.h FEATURE BATCHES): kind is None / "none",
    "whisper" (range, add, mul), "cmn", "cmvn" (var_floor) or "affine" (sub and mul_vec, one finite number per feature bin).  Raises
    ValueError for an unknown kind, a number that is not finite, var_floor <= 0 and affine vectors that are absent, not finite or of
    different lengths."""
    if isinstance(kind, FeatureNorm):
        return kind
    if not isinstance(kind, (str, type(None))) or kind not in FEAT_NORMS:
        raise ValueError(f"normalize must be None, 'whisper', 'cmn', 'cmvn', ('affine', sub, mul) or a feature_norm() record, not {kind!r}")
    nums = [float(v) for v in (range, add, mul, var_floor)]
    if not np.isfinite(nums).all() or nums[3] <= 0:
        raise ValueError("range, add, mul and var_floor must be finite, and var_floor > 0")
    norm = FEAT_NORMS[kind]
    if norm != FEAT_NORM_AFFINE:
        if sub is not None or mul_vec is not None:
            raise ValueError("sub and mul_vec go with 'affine' only")
        return FeatureNorm(norm, *nums)
    if sub is None or mul_vec is None:
        raise ValueError("'affine' needs sub and mul_vec, one number per feature bin each")
    s, m = (np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1)) for v in (sub, mul_vec))
    if s.shape != m.shape or not 1 <= s.size <= 128 or not (np.isfinite(s).all() and np.isfinite(m).all()):
        raise ValueError("the affine vectors must be finite and of one length, 1 - 128")
    return FeatureNorm(norm, *nums, s, m)


class FeatureBatch(typing.NamedTuple):
    """The feature-batch request of one decode_files call: the opusgpu_feat_batch_req record (a FEAT_BATCH_REQ_DTYPE array of one), the
    AFFINE vectors (float32 arrays or None), the features' width W and the stride S."""
    rec: object
    sub: object
    mul: object
    width: int
    stride: int


def feat_batch_layout(n, width, stride_frames):
    """opusgpu_feat_batch_layout: the dense tensor of n tracks of stride_frames frames of `width` bins -> (feat_offsets [int64], total
    floats)."""
    offsets = np.zeros(max(int(n), 0), dtype=np.int64)
    total = int(load_lib().opusgpu_feat_batch_layout(int(n), int(width), int(stride_frames), offsets.ctypes.data))
    if total < 0:
        raise ValueError(f"there is no feature batch of {n!r} tracks of {stride_frames!r} frames of {width!r} bins (stride * width <= 2^31 - 1)")
    return offsets, total


def feature_batch_request(planned_frames, width, feature_stride=None, normalize=None, feature_pad=None):
    """What decode_files makes of feature_stride=, normalize= and feature_pad= for features of `width` bins whose tracks have
    planned_frames[t] frames at their PLANNED lengths: a FeatureBatch.  feature_stride None: the largest planned F (at least 1).
    normalize: None, "whisper", "cmn", "cmvn", ("affine", sub, mul) or a feature_norm() record.  feature_pad: None -- -10 normalised
    under "whisper" (zero audio, as Whisper pads), else 0 verbatim --, a number (verbatim), or (number, "value" | "normalized").
    Raises ValueError for an unknown normalize, affine vectors of the wrong width or not finite, a stride below a planned F and a
    pad that is not finite."""
    import numbers
    planned_frames = np.asarray(planned_frames, dtype=np.int64)
    if isinstance(normalize, tuple) and not isinstance(normalize, FeatureNorm):
        if len(normalize) != 3 or normalize[0] != "affine":
            raise ValueError(f"a normalize tuple must be ('affine', sub, mul), not {normalize!r}")
        normalize = feature_norm("affine", sub=normalize[1], mul_vec=normalize[2])
    fn = feature_norm(normalize)
    if fn.norm == FEAT_NORM_AFFINE and fn.sub_vec.size != width:
        raise ValueError(f"the affine vectors have {fn.sub_vec.size} entries, the features {width} bins")
    most = int(planned_frames.max()) if planned_frames.size else 0
    if feature_stride is None:
        feature_stride = max(most, 1)
    if not isinstance(feature_stride, numbers.Integral) or isinstance(feature_stride, bool) or feature_stride < 1:
        raise ValueError(f"feature_stride must be an integer >= 1, not {feature_stride!r}")
    if feature_stride < most:
        raise ValueError(f"feature_stride {feature_stride} is below the {most} frames of the longest planned track")
    if feature_pad is None:
        feature_pad = (-10.0, "normalized") if fn.norm == FEAT_NORM_WHISPER else (0.0, "value")
    if not isinstance(feature_pad, tuple):
        feature_pad = (feature_pad, "value")
    if (len(feature_pad) != 2 or feature_pad[1] not in ("value", "normalized") or not isinstance(feature_pad[0], numbers.Real) or
            isinstance(feature_pad[0], bool) or not np.isfinite(feature_pad[0])):
        raise ValueError(f"feature_pad must be a finite number or (number, 'value' | 'normalized'), not {feature_pad!r}")
    feat_batch_layout(0, width, feature_stride)  # (stride * width must fit)
    rec = np.zeros(1, dtype=FEAT_BATCH_REQ_DTYPE)
    rec["enabled"], rec["stride_frames"], rec["norm"], rec["var_floor"] = 1, int(feature_stride), fn.norm, fn.var_floor
    rec["pad_mode"], rec["pad_value"] = FEAT_PAD_NORMALIZED if feature_pad[1] == "normalized" else FEAT_PAD_VALUE, feature_pad[0]
    rec["range"], rec["add"], rec["mul"] = fn.range, fn.add, fn.mul
    return FeatureBatch(rec, fn.sub_vec, fn.mul_vec, int(width), int(feature_stride))


def _planned_feature_frames(batch, req):
    """The frames of every track of a "features" request at its PLANNED length."""
    planned = np.asarray(batch.info["track_samples"], dtype=np.int64)
    if req.entry == "files_decode_mel":
        return -(-planned // 3) // MEL_HOP
    rate, up, down = req.args[:3]
    if rate:
        up, down = 1, TRACK_RATES[rate]
    frames = fbank_frames if req.params.dtype == FBANK_PARAMS_DTYPE else stft_frames if req.params.dtype == STFT_PARAMS_DTYPE else spec_frames
    return frames(req.params, -(-planned * up // down))


def _feature_width(params):
    return fbank_width(params) if params.dtype == FBANK_PARAMS_DTYPE else int(params["n_mels"][0])


def stft_norm(kind, range=8.0, add=4.0, mul=None, var_floor=1e-20, sub=None, mul_vec=None):
    """A normalisation for decode_files' stft_normalize= with numbers of its own (include/opusgpu.h STFT BATCHES): feature_norm's
    kinds -- None / "none", "whisper" (range, add, mul; mul None is 0.25), "cmn", "cmvn" (var_floor), "affine" (sub and mul_vec, one
    finite number per bin, 1 - 1025 of them) -- and "refmax" (range, mul; mul None is 10: dB under the track's maximum for a log10 power
    spectrogram, top_db = 10 * range).  -> a FeatureNorm.  Raises ValueError as feature_norm does."""
    if isinstance(kind, FeatureNorm):
        return kind
    if not isinstance(kind, (str, type(None))) or kind not in STFT_NORMS:
        raise ValueError("stft_normalize must be None, 'whisper', 'refmax', 'cmn', 'cmvn', ('affine', sub, mul) or a stft_norm() record, "
                         f"not {kind!r}")
    norm = STFT_NORMS[kind]
    if mul is None:
        mul = 10.0 if norm == STFT_NORM_REFMAX else 0.25
    nums = [float(v) for v in (range, add, mul, var_floor)]
    if not np.isfinite(nums).all() or nums[3] <= 0:
        raise ValueError("range, add, mul and var_floor must be finite, and var_floor > 0")
    if norm != FEAT_NORM_AFFINE:
        if sub is not None or mul_vec is not None:
            raise ValueError("sub and mul_vec go with 'affine' only")
        return FeatureNorm(norm, *nums)
    if sub is None or mul_vec is None:
        raise ValueError("'affine' needs sub and mul_vec, one number per bin each")
    s, m = (np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1)) for v in (sub, mul_vec))
    if s.shape != m.shape or not 1 <= s.size <= STFT_BATCH_MAX_BINS or not (np.isfinite(s).all() and np.isfinite(m).all()):
        raise ValueError("the affine vectors must be finite and of one length, 1 - 1025")
    return FeatureNorm(norm, *nums, s, m)


class StftBatch(typing.NamedTuple):
    """The STFT-batch request of one decode_files call: the opusgpu_stft_batch_req record (a STFT_BATCH_REQ_DTYPE array of one), the
    AFFINE vectors (float32 arrays or None), the spectrogram's bins, c (1: real cells, 2: pairs) and the stride S."""
    rec: object
    sub: object
    mul: object
    bins: int
    c: int
    stride: int


def stft_batch_layout(n, bins, c, stride_frames):
    """opusgpu_stft_batch_layout: the dense tensor of n tracks of stride_frames frames of `bins` bins of c floats -> (feat_offsets
    [int64], total floats)."""
    offsets = np.zeros(max(int(n), 0), dtype=np.int64)
    total = int(load_lib().opusgpu_stft_batch_layout(int(n), int(bins), int(c), int(stride_frames), offsets.ctypes.data))
    if total < 0:
        raise ValueError(f"there is no STFT batch of {n!r} tracks of {stride_frames!r} frames of {bins!r} bins of {c!r} floats "
                         "(bins 1 - 1025, c 1 or 2, stride * bins * c <= 2^31 - 1)")
    return offsets, total


def stft_batch_request(planned_frames, bins, c, stft_stride=None, stft_normalize=None, stft_pad=None):
    """What decode_files makes of stft_stride=, stft_normalize= and stft_pad= for spectrograms of `bins` bins of c floats (2: pairs)
    whose tracks have planned_frames[t] frames at their PLANNED lengths: a StftBatch.  stft_stride None: the largest planned F (at
    least 1).  stft_normalize: None, "whisper", "refmax", "cmn", "cmvn", ("affine", sub, mul) or a stft_norm() record; pairs take
    None and affine only.  stft_pad: None -- -10 normalised under "whisper", else 0 verbatim --, a number (verbatim), or (number,
    "value" | "normalized").  Raises ValueError for an unknown stft_normalize, a norm that pairs do not take, affine vectors of the
    wrong length or not finite, a stride below a planned F and a pad that is not finite."""
    import numbers
    planned_frames = np.asarray(planned_frames, dtype=np.int64)
    if c not in (1, 2):
        raise ValueError(f"c must be 1 (real cells) or 2 (pairs), not {c!r}")
    if isinstance(stft_normalize, tuple) and not isinstance(stft_normalize, FeatureNorm):
        if len(stft_normalize) != 3 or stft_normalize[0] != "affine":
            raise ValueError(f"a stft_normalize tuple must be ('affine', sub, mul), not {stft_normalize!r}")
        stft_normalize = stft_norm("affine", sub=stft_normalize[1], mul_vec=stft_normalize[2])
    fn = stft_norm(stft_normalize)
    if c == 2 and fn.norm not in (FEAT_NORM_NONE, FEAT_NORM_AFFINE):
        raise ValueError("complex spectrograms (pairs) take stft_normalize None and ('affine', sub, mul) only")
    if fn.norm == FEAT_NORM_AFFINE and fn.sub_vec.size != bins:
        raise ValueError(f"the affine vectors have {fn.sub_vec.size} entries, the spectrogram {bins} bins")
    most = int(planned_frames.max()) if planned_frames.size else 0
    if stft_stride is None:
        stft_stride = max(most, 1)
    if not isinstance(stft_stride, numbers.Integral) or isinstance(stft_stride, bool) or stft_stride < 1:
        raise ValueError(f"stft_stride must be an integer >= 1, not {stft_stride!r}")
    if stft_stride < most:
        raise ValueError(f"stft_stride {stft_stride} is below the {most} frames of the longest planned track")
    if stft_pad is None:
        stft_pad = (-10.0, "normalized") if fn.norm == FEAT_NORM_WHISPER else (0.0, "value")
    if not isinstance(stft_pad, tuple):
        stft_pad = (stft_pad, "value")
    if (len(stft_pad) != 2 or stft_pad[1] not in ("value", "normalized") or not isinstance(stft_pad[0], numbers.Real) or
            isinstance(stft_pad[0], bool) or not np.isfinite(stft_pad[0])):
        raise ValueError(f"stft_pad must be a finite number or (number, 'value' | 'normalized'), not {stft_pad!r}")
    stft_batch_layout(0, bins, c, stft_stride)  # (stride * bins * c must fit)
    rec = np.zeros(1, dtype=STFT_BATCH_REQ_DTYPE)
    rec["enabled"], rec["stride_frames"], rec["norm"], rec["var_floor"] = 1, int(stft_stride), fn.norm, fn.var_floor
    rec["pad_mode"], rec["pad_value"] = FEAT_PAD_NORMALIZED if stft_pad[1] == "normalized" else FEAT_PAD_VALUE, stft_pad[0]
    rec["range"], rec["add"], rec["mul"] = fn.range, fn.add, fn.mul
    return StftBatch(rec, fn.sub_vec, fn.mul_vec, int(bins), int(c), int(stft_stride))


class WaveBatch(typing.NamedTuple):
    """The wave-batch request of one decode_files call: the opusgpu_wave_batch_req record (a WAVE_BATCH_REQ_DTYPE array of one), the
    tracks' channels C, the stride S, whether a mask is written, and the buffer as opusgpu_wave_batch_layout lays it out for the
    `n` tracks the request was made for: `floats` in all, the mask `mask_offset` bytes in."""
    rec: object
    channels: int
    stride: int
    mask: bool
    n: int
    floats: int
    mask_offset: int


def wave_batch_layout(n, channels, stride_samples, mask=False):
    """opusgpu_wave_batch_layout: the dense tensor of n tracks of stride_samples samples of `channels` channels, and the mask behind
    it -> (total floats of the buffer, the mask's byte offset or None)."""
    at = C.c_int64(0)
    total = int(load_lib().opusgpu_wave_batch_layout(int(n), int(channels), int(stride_samples), 1 if mask else 0, C.byref(at)))
    if total < 0:
        raise ValueError(f"there is no wave batch of {n!r} tracks of {stride_samples!r} samples of {channels!r} channels "
                         "(stride * channels <= 2^31 - 1)")
    return total, (int(at.value) if mask else None)


def wave_batch_request(planned_out_samples, channels, wave_stride=None, wave_normalize=None, wave_pad=None, wave_mask=False):
    """What decode_files makes of wave_stride=, wave_normalize=, wave_pad= and wave_mask= for tracks of `channels` channels whose
    PLANNED lengths at the output's rate are planned_out_samples[t] (include/opusgpu.h WAVE BATCHES): a WaveBatch.  wave_stride None:
    the longest planned track (at least 1).  wave_normalize: None / "none", "zmuv" (eps 1e-7, Wav2Vec2FeatureExtractor's), ("zmuv",
    eps) or ("peak", target).  wave_pad: the pad cells' value, None is 0.  Raises ValueError for an unknown wave_normalize, an eps
    or target that is not finite and > 0, a stride that is no integer >= 1 or lies below a planned length, stride * channels above
    2^31 - 1, a pad that is not finite and a wave_mask that is no bool."""
    import numbers

    def number(v):
        return isinstance(v, numbers.Real) and not isinstance(v, bool) and np.isfinite(v)
    planned = np.asarray(planned_out_samples, dtype=np.int64)
    norm, value = wave_normalize if isinstance(wave_normalize, tuple) and len(wave_normalize) == 2 else (wave_normalize, None)
    if not isinstance(norm, (str, type(None))) or norm not in WAVE_NORMS or (value is not None and WAVE_NORMS[norm] == WAVE_NORM_NONE):
        raise ValueError(f"wave_normalize must be None, 'zmuv', ('zmuv', eps) or ('peak', target), not {wave_normalize!r}")
    norm = WAVE_NORMS[norm]
    if norm == WAVE_NORM_PEAK and value is None:
        raise ValueError("wave_normalize 'peak' needs its target: ('peak', target)")
    if value is not None and not (number(value) and value > 0):
        raise ValueError(f"the eps or target of wave_normalize must be finite and > 0, not {value!r}")
    most = int(planned.max()) if planned.size else 0
    if wave_stride is None:
        wave_stride = max(most, 1)
    if not isinstance(wave_stride, numbers.Integral) or isinstance(wave_stride, bool) or wave_stride < 1:
        raise ValueError(f"wave_stride must be an integer >= 1, not {wave_stride!r}")
    if wave_stride < most:
        raise ValueError(f"wave_stride {wave_stride} is below the {most} samples of the longest planned track")
    wave_pad = 0.0 if wave_pad is None else wave_pad
    if not number(wave_pad):
        raise ValueError(f"wave_pad must be a finite number, not {wave_pad!r}")
    if not isinstance(wave_mask, (bool, np.bool_)):
        raise ValueError(f"wave_mask must be True or False, not {wave_mask!r}")
    floats, mask_offset = wave_batch_layout(planned.size, channels, wave_stride, bool(wave_mask))
    rec = np.zeros(1, dtype=WAVE_BATCH_REQ_DTYPE)
    rec["enabled"], rec["stride_samples"], rec["norm"], rec["pad_value"], rec["mask"] = 1, int(wave_stride), norm, wave_pad, 1 if wave_mask else 0
    rec["eps"], rec["target"] = (value if norm == WAVE_NORM_ZMUV and value is not None else WAVE_EPS), (value if norm == WAVE_NORM_PEAK else 1.0)
    return WaveBatch(rec, int(channels), int(wave_stride), bool(wave_mask), int(planned.size), floats, mask_offset)


def trim_spec(top_db=60.0, frame_length=2048, hop_length=512, ref="max", margin=0, flags=False):
    """The opusgpu_wave_trim_req record (a WAVE_TRIM_REQ_DTYPE array of one) of decode_files(wave_trim=...) and
    Context.tracks_wave_trim_device (include/opusgpu.h WAVE TRIM).  Frames of frame_length samples every hop_length, centred as
    librosa.feature.rms centres them; a frame is active where its energy lies less than top_db dB below the reference.  ref="max":
    the track's loudest frame, librosa.effects.trim's default -- REL mode with ratio = 10^(-top_db / 10).  ref a number: dBFS, with a
    frame of full-scale samples (32768^2 * frame_length) at 0 -- ABS mode with threshold = floor(frame_length * 2^30 *
    10^((ref - top_db) / 10)).  margin: samples kept on either side of the active span.  flags=True keeps the per-frame activity
    (info["activity"]; activity_intervals turns it into intervals).  Raises ValueError with the rule broken: frame_length a multiple of
    16 in 16 - 8192, hop_length a multiple of 8 in 8 - frame_length, margin a multiple of 8 and >= 0, top_db finite and >= 0 under
    ref="max" (a ratio in (0, 1]), a threshold that fits 64 bits, flags a bool."""
    import math
    import numbers

    def integer(v):
        return isinstance(v, numbers.Integral) and not isinstance(v, bool)

    def number(v):
        return isinstance(v, numbers.Real) and not isinstance(v, bool) and np.isfinite(v)
    if not integer(frame_length) or frame_length < 16 or frame_length > 8192 or frame_length % 16:
        raise ValueError(f"frame_length must be a multiple of 16 in 16 - 8192, not {frame_length!r}")
    if not integer(hop_length) or hop_length < 8 or hop_length > frame_length or hop_length % 8:
        raise ValueError(f"hop_length must be a multiple of 8 in 8 - frame_length, not {hop_length!r}")
    if not integer(margin) or margin < 0 or margin % 8 or margin > 0x7fffffff:
        raise ValueError(f"margin must be a multiple of 8 and >= 0, not {margin!r}")
    if not number(top_db):
        raise ValueError(f"top_db must be a finite number, not {top_db!r}")
    if not isinstance(flags, (bool, np.bool_)):
        raise ValueError(f"flags must be True or False, not {flags!r}")
    rec = np.zeros(1, dtype=WAVE_TRIM_REQ_DTYPE)
    rec["enabled"], rec["frame_length"], rec["hop"], rec["margin"], rec["flags"] = 1, frame_length, hop_length, margin, 1 if flags else 0
    if isinstance(ref, str):
        if ref != "max":
            raise ValueError(f"ref must be 'max' or a level in dBFS, not {ref!r}")
        ratio = 10.0 ** (-float(top_db) / 10)
        if not 0 < ratio <= 1:
            raise ValueError(f"top_db must be >= 0 and leave a ratio above 0 under ref='max', not {top_db!r}")
        rec["mode"], rec["ratio"] = WAVE_TRIM_REL, ratio
    else:
        if not number(ref):
            raise ValueError(f"ref must be 'max' or a finite level in dBFS, not {ref!r}")
        threshold = math.floor(frame_length * 2.0 ** 30 * 10.0 ** ((float(ref) - float(top_db)) / 10))
        if threshold >= 1 << 64:
            raise ValueError(f"ref {ref!r} and top_db {top_db!r} give a threshold that does not fit 64 bits")
        rec["mode"], rec["ratio"], rec["threshold"] = WAVE_TRIM_ABS, 1.0, threshold
    return rec


def wave_trim_frames(samples, hop):
    """WAVE TRIM's frame count of a track (or an array of tracks) of `samples` samples: 1 + samples // hop."""
    return 1 + np.asarray(samples, dtype=np.int64) // int(hop)


def activity_intervals(flags, hop, length):
    """The activity flags of one track (info["activity"][t]: one uint8 per frame) -> its active [start, end) sample intervals, an
    int64 array [k, 2], as librosa.effects.split forms them: a run of active frames f0 .. f1 is [f0 * hop, (f1 + 1) * hop), cut at
    `length`, the track's untrimmed length (info["wave_trim"][t]["full"]).  On the host."""
    on = np.concatenate(([0], (np.asarray(flags).reshape(-1) != 0).astype(np.int8), [0]))
    edges = np.flatnonzero(np.diff(on))  # rises at even places, falls at odd ones
    out = np.minimum(edges.reshape(-1, 2).astype(np.int64) * int(hop), int(length))
    return out[out[:, 1] > out[:, 0]]


class FilesRequest(typing.NamedTuple):
    """What one decode_files call asks of the library, made by files_request before any decoder is touched."""
    entry: str        # the C entry point without its opusgpu_ / opusgpu_ms_ prefix
    args: tuple       # its scalar and record arguments between the batch and the format, in call order (a record: an array of one, or None)
    kind: str         # "tracks" (the planned grid at 48 kHz), "resampled" or "features"
    fmt: int          # TRACKS_*
    scale: object     # float32 array or None
    out: object       # the caller's tensor, flattened, or None
    channels: int     # output channels
    offsets: object   # the planned grid of the result: offsets, planes (planar tracks and band-major features) and total, per channel
    planes: object
    total: int
    mix: object       # the matrix record or None
    params: object    # the features' record or None
    loudness: object = None  # the loudness request's record (loudness_request) or None
    stride: int = 0   # a strided batch of cuts: every track `stride` samples per channel apart, zeros behind its final length
    cut_info: object = None  # the batch's CUT_INFO_DTYPE records (a batch of cuts) or None
    feature_batch: object = None  # the FeatureBatch of feature_stride= / normalize= or None; with one, offsets and total are the dense tensor's
    wave_batch: object = None  # the WaveBatch of wave_stride= / wave_normalize= / wave_mask= or None; with one, offsets and total are the dense tensor's
    wave_trim: object = None  # the trim_spec() record of wave_trim= or None; only beside a wave_batch
    stft_batch: object = None  # the StftBatch of stft_stride= / stft_normalize= / stft_pad= or None; with one, offsets and total are the dense tensor's


STRIDE_REFUSED = ("the batch has a stride, which only tracks at 48 kHz keep (format=, scale=, out=, and loudness= with \"s16\"): resampled, "
                  "mixed and feature outputs have grids of their own -- plan the cuts without stride= for these arguments")


def _files_request(batch, multistream=False, device=0, format=None, scale=None, out=None, rate=None, mono=False, mix=None, features=None,
                  n_mels=80, feature_layout="bands", resample=None, loudness=None, peak_limit=1.0, channel_weights=None):
    """The keywords of decode_files for a planned batch -> the FilesRequest that _run_files_request carries out.  Every refusal of
    decode_files is raised here, as ValueError, by the track_*_args helpers; nothing of a decoder is needed.  multistream: the batch
    is an MsFileBatch, whose C calls take no `mono` and whose tracks have no mono downmix.
    loudness=None is exactly the request it always was.  Otherwise the request carries the loudness record; a target needs a float
    format or features; and float tracks at 48 kHz without a mix, whose call (files_decode_as) never has an int16 track to measure,
    go through files_decode_mixed with the identity matrix, which writes the same elements (include/opusgpu.h TRACK LOUDNESS)."""
    lreq = loudness_request(batch, loudness, peak_limit, channel_weights)
    if lreq is not None:
        req = _files_request(batch, multistream, device, format, scale, out, rate, mono, mix, features, n_mels, feature_layout, resample)
        if req.entry == "files_decode_as":
            identity = 16384 * np.eye(batch.channels, dtype=np.int16)
            req = _files_request(batch, multistream, device, format, scale, out, rate, mono, identity, features, n_mels, feature_layout, resample)
        if int(lreq["mode"][0]) == LOUDNESS_NORMALIZE and req.kind != "features" and req.fmt == TRACKS_S16:
            raise ValueError("a loudness target needs a float format or features: int16 tracks are not scaled")
        return req._replace(loudness=lreq)
    if mix is not None and mono:
        raise ValueError("mix and mono=True exclude each other: the row {8192, 8192} is mono")
    allow_mono, mono_arg = not multistream, () if multistream else (1 if mono else 0,)
    planned = batch.info["track_samples"]
    if getattr(features, "dtype", None) == SPEC_PARAMS_DTYPE:
        sargs = track_spectrogram_args(batch, features, rate, resample, mono, mix, format, scale, out, device, allow_mono)
        rec, mrec, scale, offsets, planes, total, out, how = sargs
        return FilesRequest("files_decode_melspec", how + mono_arg + (mrec, rec), "features", TRACKS_F32, scale, out, 1, offsets, planes, total,
                            mrec, rec)
    if getattr(features, "dtype", None) == STFT_PARAMS_DTYPE:
        rec, mrec, scale, offsets, planes, total, out, how = track_stft_args(batch, features, rate, resample, mono, mix, format, scale, out,
                                                                             device, allow_mono)
        return FilesRequest("files_decode_stft", how + mono_arg + (mrec, rec), "features", TRACKS_F32, scale, out, 1, offsets, planes, total,
                            mrec, rec)
    if getattr(features, "dtype", None) == FBANK_PARAMS_DTYPE:
        rec, mrec, scale, offsets, planes, total, out, how = track_kaldi_args(batch, features, rate, resample, mono, mix, format, scale, out,
                                                                              device, allow_mono)
        return FilesRequest("files_decode_fbank", how + mono_arg + (mrec, rec), "features", TRACKS_F32, scale, out, 1, offsets, planes, total,
                            mrec, rec)
    if resample is not None:
        format = "s16" if format is None else format
        (up, down), ch, offsets, total, out, mrec = track_ratio_args(batch, resample, mono, mix, format, out, device, allow_mono, rate, features)
        fmt, scale, _ = track_format_args(batch, format, scale, None, device)
        return FilesRequest("files_decode_ratio", (up, down) + mono_arg + (mrec,), "resampled", fmt, scale, out, ch, offsets,
                            ((planned * up + down - 1) // down + 63) // 64 * 64, total, mrec, None)
    fargs = track_feature_args(batch, features, n_mels, feature_layout, rate, mono, mix, format, scale, out, device, allow_mono)
    if fargs is not None:
        rec, mrec, scale, offsets, planes, total, out = fargs
        return FilesRequest("files_decode_mel", mono_arg + (mrec, rec), "features", TRACKS_F32, scale, out, 1, offsets, planes, total, mrec, rec)
    rate, format = 48000 if rate is None else rate, "s16" if format is None else format
    mrec = None
    if mix is not None:
        D, ch, offsets, total, rout, mrec = track_mix_args(batch, mix, rate, format, out, device)
        entry, args = "files_decode_mixed", (int(rate), mrec)
    else:
        rargs = track_rate_args(batch, rate, mono, format, out, device, allow_mono)
        if rargs is None:
            fmt, scale, out = track_format_args(batch, format, scale, out, device)
            return FilesRequest("files_decode" if fmt == TRACKS_S16 else "files_decode_as", (), "tracks", fmt, scale, out, batch.channels,
                                batch.info["track_offset"], (planned + 63) // 64 * 64, int(batch.track_samples), None, None)
        D, ch, offsets, total, rout = rargs
        entry, args = "files_decode_resampled", (int(rate),) + mono_arg
    fmt, scale, _ = track_format_args(batch, format, scale, None, device)
    return FilesRequest(entry, args, "resampled", fmt, scale, rout, ch, offsets, ((planned + D - 1) // D + 63) // 64 * 64, total, mrec, None)


def files_request(batch, multistream=False, device=0, format=None, scale=None, out=None, rate=None, mono=False, mix=None, features=None,
                  n_mels=80, feature_layout="bands", resample=None, loudness=None, peak_limit=1.0, channel_weights=None,
                  feature_stride=None, normalize=None, feature_pad=None, wave_stride=None, wave_normalize=None, wave_pad=None,
                  wave_mask=False, stft_stride=None, stft_normalize=None, stft_pad=None, wave_trim=None):
    """The keywords of decode_files for a planned batch -> the FilesRequest that _run_files_request carries out (_files_request says
    how).  A batch of cuts (FileBatch(cuts=...)) is a batch like any other: the request carries its cut records, which only info
    reads.  A strided one is refused here, as ValueError, with everything but tracks at 48 kHz; its planes lie the stride apart.
    feature_stride=, normalize= and feature_pad= (FEATURE BATCHES; feature_batch_request says what they may be) need features= and
    turn the request's result into one dense tensor: its `feature_batch` carries the record, and total, offsets, planes (the stride
    for every track) and the out= size check follow opusgpu_feat_batch_layout.  Without them the request is what it always was.
    wave_stride=, wave_normalize=, wave_pad= and wave_mask= (WAVE BATCHES; wave_batch_request says what they may be) need a float
    format and no features=, and turn the TRACKS of the request into one dense tensor: its `wave_batch` carries the record and the
    buffer's layout, total is n * S and offsets t * S.  Tracks at 48 kHz without a mix, whose call has no resampling kernel, go
    through files_decode_mixed with the identity matrix, which writes the same elements.
    wave_trim= (WAVE TRIM: a trim_spec() record) counts as one of the wave keywords -- alone it makes the dense tensor with the
    defaults of the others -- and becomes the request's `wave_trim`: every row is then the track without its leading and trailing
    silence.  Anything but None or such a record of one element with `enabled` set raises ValueError.
    stft_stride=, stft_normalize= and stft_pad= (STFT BATCHES; stft_batch_request says what they may be) need a stft_spec() record as
    features= and turn its result into one dense tensor: the request's `stft_batch` carries the record, and total, offsets, planes
    (the stride for every track) and the out= size check follow opusgpu_stft_batch_layout."""
    stride, cut_info = int(getattr(batch, "stride", 0) or 0), getattr(batch, "cut_info", None)
    wave = wave_stride is not None or wave_normalize is not None or wave_pad is not None or wave_mask is not False or wave_trim is not None
    if wave_trim is not None and not (isinstance(wave_trim, np.ndarray) and wave_trim.dtype == WAVE_TRIM_REQ_DTYPE and wave_trim.shape == (1,)
                                      and int(wave_trim["enabled"][0]) == 1):
        raise ValueError(f"wave_trim must be None or a trim_spec() record, not {wave_trim!r}")
    sdense = stft_stride is not None or stft_normalize is not None or stft_pad is not None
    if stride and (rate not in (None, 48000) or mono or mix is not None or features is not None or resample is not None or wave or
                   (loudness is not None and format not in (None, "s16"))):
        raise ValueError(STRIDE_REFUSED)
    dense = feature_stride is not None or normalize is not None or feature_pad is not None
    if dense and features is None:
        raise ValueError("feature_stride=, normalize= and feature_pad= need features=")
    if dense and getattr(features, "dtype", None) == STFT_PARAMS_DTYPE:
        raise ValueError("feature_stride=, normalize= and feature_pad= do not go with a stft_spec() record: feature batches hold widths of "
                         "1 - 128, a linear spectrogram has n_fft / 2 + 1 bins")
    if sdense and getattr(features, "dtype", None) != STFT_PARAMS_DTYPE:
        raise ValueError("stft_stride=, stft_normalize= and stft_pad= need a stft_spec() record as features=")
    if wave and features is not None:
        raise ValueError("wave_stride=, wave_normalize=, wave_pad=, wave_mask= and wave_trim= are for tracks: features have feature_stride= and normalize=")
    if wave and format in (None, "s16"):
        raise ValueError("wave_stride=, wave_normalize=, wave_pad=, wave_mask= and wave_trim= need format='f32' or 'f32_planar': the dense tensor is float32")
    req = _files_request(batch, multistream, device, format, scale, None if dense or wave or sdense else out, rate, mono, mix, features, n_mels,
                         feature_layout, resample, loudness, peak_limit, channel_weights)
    if wave:
        if req.entry == "files_decode_as":  # 16384 on the diagonal is exactly x = s
            req = _files_request(batch, multistream, device, format, scale, None, rate, mono, 16384 * np.eye(batch.channels, dtype=np.int16),
                                 features, n_mels, feature_layout, resample, loudness, peak_limit, channel_weights)
        up, down = req.args[:2] if req.entry == "files_decode_ratio" else (1, TRACK_RATES[req.args[0]])
        wb = wave_batch_request(-(-np.asarray(batch.info["track_samples"], dtype=np.int64) * up // down), req.channels, wave_stride, wave_normalize,
                                wave_pad, wave_mask)
        if out is not None:
            out = _out_flat(out, max(wb.floats, 1), format, device)
        req = req._replace(wave_batch=wb, offsets=np.arange(batch.n_files, dtype=np.int64) * wb.stride, total=batch.n_files * wb.stride, out=out,
                           planes=np.full(batch.n_files, wb.stride, dtype=np.int64), wave_trim=None if wave_trim is None else wave_trim.copy())
    if dense:
        width = _feature_width(req.params)
        fb = feature_batch_request(_planned_feature_frames(batch, req), width, feature_stride, normalize, feature_pad)
        offsets, total = feat_batch_layout(batch.n_files, width, fb.stride)
        if out is not None:
            out = _out_flat(out, max(total, 1), "f32", device)
        req = req._replace(feature_batch=fb, offsets=offsets, total=total, out=out, planes=np.full(batch.n_files, fb.stride, dtype=np.int64))
    if sdense:
        bins, c = int(req.params["n_fft"][0]) // 2 + 1, 2 if int(req.params["power"][0]) == STFT_COMPLEX else 1
        if bins > STFT_BATCH_MAX_BINS:  # (only an algo="fft" record has that many)
            raise ValueError(f"stft_stride=, stft_normalize= and stft_pad= hold spectrograms of 1 - {STFT_BATCH_MAX_BINS} bins, "
                             f"this record has {bins}")
        sb = stft_batch_request(_planned_feature_frames(batch, req), bins, c, stft_stride, stft_normalize, stft_pad)
        offsets, total = stft_batch_layout(batch.n_files, bins, c, sb.stride)
        if out is not None:
            out = _out_flat(out, max(total, 1), "f32", device)
        req = req._replace(stft_batch=sb, offsets=offsets, total=total, out=out, planes=np.full(batch.n_files, sb.stride, dtype=np.int64))
    if stride:
        req = req._replace(stride=stride, planes=np.full(batch.n_files, stride, dtype=np.int64))
    return req if cut_info is None else req._replace(cut_info=cut_info)


def _run_files_request(req, lib, prefix, handle, chk, batch, mem):
    """Carries out a FilesRequest for the decoder `handle` (its C family `prefix`: "opusgpu_" or "opusgpu_ms_") over `batch`, into
    req.out (a torch tensor on the device: nothing comes to the host) or into a buffer from `mem` (a Context: dev_alloc, d2h,
    dev_free); chk(code, what) raises.  -> (tracks or features, info).  Tracks are [samples, channels] (planar: transposed), features
    float32 [n_mels, F] or [F, n_mels].  info: FILE_INFO_DTYPE records plus `final_status` and `bad_packet`, `track_samples` the FINAL
    length at 48 kHz; resampled tracks have `out_samples` and `out_offset` more; features `feat_offset`, and their `frames` is F, the
    track's feature frames (the plan's count of Opus frames is batch.info["frames"]).  With a loudness request (req.loudness) the
    request is set on the decoder for this call alone and cleared behind it, and info has `lufs`, `peak`, `loudness_blocks`,
    `loudness_gated` and `gain` more.  With a feature-batch request (req.feature_batch) that request is set and cleared the same way,
    and the features are ONE float32 array or tensor [n, n_mels, S] or [n, S, n_mels] (with out=: a view of the caller's memory), padded
    behind every track's info["frames"]; info["feat_offset"] is t * S * n_mels.  With a wave-batch request (req.wave_batch), set and
    cleared the same way, the tracks are ONE float32 array or tensor [n, S, channels] ([n, S] for one channel; planar: [n, channels, S]),
    padded behind every track's info["out_samples"]; info["out_offset"] is t * S, info["wave_stats"] the WAVE_STAT_DTYPE records and, with
    a mask, info["mask"] the uint8 [n, S] mask.  With a trim request beside it (req.wave_trim), set and cleared the same way, every row is
    the track without its leading and trailing silence: info["out_samples"] is the trimmed length, info["trim_start"] and
    info["trim_samples"] the samples kept of the untrimmed track, info["wave_trim"] the WAVE_TRIM_STAT_DTYPE records and, where the record
    asks for flags, info["activity"] a list of uint8 arrays, one flag per frame."""
    name = prefix + req.entry
    n, ch, fmt = batch.n_files, req.channels, req.fmt
    offsets, counts, lengths = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    head = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in req.args]
    if req.entry != "files_decode":  # (which has neither)
        head += ([] if req.kind == "features" else [fmt]) + [None if req.scale is None else req.scale.ctypes.data]
    tail = [a.ctypes.data for a in ((lengths, status) if req.kind == "tracks" else (offsets, counts, lengths, status))]

    loud = np.zeros(n, dtype=LOUDNESS_DTYPE)
    gains = np.ones(n, dtype=np.float64)

    fb, wb, sb = req.feature_batch, req.wave_batch, req.stft_batch
    wave_stats = np.zeros(n, dtype=WAVE_STAT_DTYPE)
    tr = req.wave_trim
    trim_stats, activity = np.zeros(n, dtype=WAVE_TRIM_STAT_DTYPE), []

    def run(d_out):
        if wb is not None:
            chk(getattr(lib, prefix + "set_wave_batch")(handle, wb.rec.ctypes.data), prefix + "set_wave_batch")
            try:
                if tr is not None:
                    chk(getattr(lib, prefix + "set_wave_trim")(handle, tr.ctypes.data), prefix + "set_wave_trim")
                run_loud(d_out)
                got = getattr(lib, prefix + "last_wave_stats")(handle, n, wave_stats.ctypes.data)
                assert got == n, (got, n)
                if tr is not None:
                    got = getattr(lib, prefix + "last_wave_trim")(handle, n, trim_stats.ctypes.data)
                    assert got == n, (got, n)
                if tr is not None and int(tr["flags"][0]):
                    packed_flags = np.zeros(int(trim_stats["frames"].sum()), dtype=np.uint8)
                    got = getattr(lib, prefix + "last_wave_trim_flags")(handle, packed_flags.size, packed_flags.ctypes.data)
                    assert got == packed_flags.size, (got, packed_flags.size)
                    activity.extend(np.split(packed_flags, np.cumsum(trim_stats["frames"])[:-1]))
            finally:
                getattr(lib, prefix + "set_wave_trim")(handle, None)
                getattr(lib, prefix + "set_wave_batch")(handle, None)
            return
        if sb is not None:
            vecs = [None if v is None else v.ctypes.data for v in (sb.sub, sb.mul)]
            chk(getattr(lib, prefix + "set_stft_batch")(handle, sb.rec.ctypes.data, *vecs, sb.bins), prefix + "set_stft_batch")
            try:
                run_loud(d_out)
            finally:
                getattr(lib, prefix + "set_stft_batch")(handle, None, None, None, 0)
            return
        if fb is None:
            return run_loud(d_out)
        vecs = [None if v is None else v.ctypes.data for v in (fb.sub, fb.mul)]
        chk(getattr(lib, prefix + "set_feature_batch")(handle, fb.rec.ctypes.data, *vecs, fb.width), prefix + "set_feature_batch")
        try:
            run_loud(d_out)
        finally:
            getattr(lib, prefix + "set_feature_batch")(handle, None, None, None, 0)

    def run_loud(d_out):
        if req.loudness is None:
            chk(getattr(lib, name)(handle, batch.h, *head, d_out, *tail), name)
            return
        chk(getattr(lib, prefix + "set_loudness")(handle, req.loudness.ctypes.data), prefix + "set_loudness")
        try:
            chk(getattr(lib, name)(handle, batch.h, *head, d_out, *tail), name)
            got = getattr(lib, prefix + "last_loudness")(handle, n, loud.ctypes.data, gains.ctypes.data)
            assert got == n, (got, n)
        finally:
            getattr(lib, prefix + "set_loudness")(handle, None)
    if req.out is not None:
        import torch
        torch.cuda.current_stream(req.out.device).synchronize()  # whatever filled `out` has finished; the call itself waits for its own work
        run(req.out.data_ptr())
        packed = req.out
    else:
        packed = np.zeros(max(req.total, 1) * ch if wb is None else max(wb.floats, 1), dtype=np.int16 if fmt == TRACKS_S16 else np.float32)
        d_out = mem.dev_alloc(packed.nbytes)
        try:
            run(d_out)
            mem.d2h(packed, d_out)
        finally:
            mem.dev_free(d_out)
    # the result's own count and offset per file: the fields of `info` that hold them, and which of them are new
    count_field, offset_field, more = {"tracks": (None, None, []), "resampled": ("out_samples", "out_offset", ["out_samples", "out_offset"]),
                                       "features": ("frames", "feat_offset", ["feat_offset"])}[req.kind]
    louder = [] if req.loudness is None else [("lufs", "<f4"), ("peak", "<f4"), ("loudness_blocks", "<i4"), ("loudness_gated", "<i4"), ("gain", "<f8")]
    cut_fields = [] if req.cut_info is None else [("cut_" + f, CUT_INFO_DTYPE[f].str) for f in CUT_INFO_DTYPE.names]
    wave_fields = [] if wb is None else [("wave_stats", WAVE_STAT_DTYPE)] + ([("mask", "u1", (wb.stride,))] if wb.mask else [])
    if tr is not None:
        wave_fields += [("trim_start", "<i8"), ("trim_samples", "<i8"), ("wave_trim", WAVE_TRIM_STAT_DTYPE)]
        wave_fields += [("activity", "O")] if int(tr["flags"][0]) else []  # (ragged: one array per track)
    info = np.zeros(n, dtype=np.dtype(FILE_INFO_DTYPE.descr + [("final_status", "<i4"), ("bad_packet", "<i4")] + [(f, "<i8") for f in more] +
                                      louder + cut_fields + wave_fields))
    for f in CUT_INFO_DTYPE.names if cut_fields else ():
        info["cut_" + f] = req.cut_info[f]
    if louder:
        info["lufs"], info["peak"], info["loudness_blocks"], info["loudness_gated"] = loud["lufs"], loud["peak"], loud["blocks"], loud["gated"]
        info["gain"] = gains
    for field in FILE_INFO_DTYPE.names:
        info[field] = batch.info[field]
    info["track_samples"], info["final_status"], info["bad_packet"] = lengths, status[:, 0], status[:, 1]
    if req.kind == "tracks":
        offsets, counts = req.offsets, lengths
    else:
        assert (offsets == req.offsets).all()
        info[count_field], info[offset_field] = counts, offsets
    if req.kind == "features" and req.params.dtype == STFT_PARAMS_DTYPE:  # TRACK STFT: [bins, F] or [F, bins], complex64 over the pairs
        bins, pairs = int(req.params["n_fft"][0]) // 2 + 1, int(req.params["power"][0]) == STFT_COMPLEX
        c = 2 if pairs else 1

        def cells(flat, *shape):  # `flat`: the track's floats as they lie; a numpy array or a torch tensor
            if not pairs:
                return flat.reshape(*shape)
            if isinstance(flat, np.ndarray):
                return flat.view(np.complex64).reshape(*shape)
            import torch
            return torch.view_as_complex(flat.reshape(*shape, 2))
        if sb is not None:  # STFT BATCHES: one dense tensor, every track sb.stride frames, padded behind its info["frames"]
            shape = (n, sb.stride, bins) if int(req.params["layout"][0]) == MEL_FRAMES_MAJOR else (n, bins, sb.stride)
            return cells(packed[:n * sb.stride * bins * c], *shape), info
        if int(req.params["layout"][0]) == MEL_FRAMES_MAJOR:
            return [cells(packed[o:o + F * bins * c], F, bins) for o, F in zip(offsets, counts)], info
        return [cells(packed[o:o + bins * p * c], bins, p)[:, :F] for o, p, F in zip(offsets, req.planes, counts)], info
    if req.kind == "features":
        n_mels = fbank_width(req.params) if req.params.dtype == FBANK_PARAMS_DTYPE else int(req.params["n_mels"][0])
        if fb is not None:  # FEATURE BATCHES: one dense tensor, every track fb.stride frames, padded behind its info["frames"]
            shape = (n, fb.stride, n_mels) if int(req.params["layout"][0]) == MEL_FRAMES_MAJOR else (n, n_mels, fb.stride)
            dense = packed[:n * fb.stride * n_mels]
            return (dense.view(*shape) if req.out is not None else dense.reshape(shape)), info
        if int(req.params["layout"][0]) == MEL_FRAMES_MAJOR:
            return [packed[o:o + F * n_mels].reshape(F, n_mels) for o, F in zip(offsets, counts)], info
        return [packed[o:o + n_mels * p].reshape(n_mels, p)[:, :F] for o, p, F in zip(offsets, req.planes, counts)], info
    if wb is not None:  # WAVE BATCHES: one dense tensor, every track wb.stride samples, padded behind its info["out_samples"]
        info["wave_stats"] = wave_stats
        if tr is not None:
            info["trim_start"], info["trim_samples"], info["wave_trim"] = trim_stats["start"], trim_stats["count"], trim_stats
            for t, flags in enumerate(activity):
                info["activity"][t] = flags
        if wb.mask and req.out is not None:
            mask = np.zeros((n, wb.stride), dtype=np.uint8)
            mem.d2h(mask, C.c_void_p(req.out.data_ptr() + wb.mask_offset))
            info["mask"] = mask
        elif wb.mask:
            info["mask"] = packed.view(np.uint8)[wb.mask_offset:wb.mask_offset + n * wb.stride].reshape(n, wb.stride)
        shape = (n, ch, wb.stride) if fmt == TRACKS_F32_PLANAR else (n, wb.stride, ch) if ch > 1 else (n, wb.stride)
        dense = packed[:n * wb.stride * ch]
        return (dense.view(*shape) if req.out is not None else dense.reshape(shape)), info
    if req.stride and req.out is not None:  # the caller's memory as the tensor it is: every track at its stride, zeros behind its length
        shape = (n, ch, req.stride) if fmt == TRACKS_F32_PLANAR else (n, req.stride, ch)
        return packed[:n * req.stride * ch].view(*shape), info
    if fmt == TRACKS_F32_PLANAR:  # track t: `ch` planes of its planned length rounded up to 64, where its interleaved form would lie
        return [packed[ch * o:ch * (o + p)].reshape(ch, p)[:, :ln] for o, p, ln in zip(offsets, req.planes, counts)], info
    return [packed[ch * o:ch * (o + ln)].reshape(ln, ch) for o, ln in zip(offsets, counts)], info


class Context:
    """One GPU context: per-stream state in HBM plus the batched decode entry points."""

    def __init__(self, device: int = 0):
        self.lib = load_lib()
        h = C.c_void_p()
        rc = self.lib.opusgpu_ctx_create(device, C.byref(h))
        if rc != 0:
            raise OpusGpuError(f"opusgpu_ctx_create(device={device}) failed with {rc}"
                               + (" (no usable HIP device; no CPU fallback exists)" if rc == OPUSGPU_ERR_NO_DEVICE else ""))
        self.h = h
        self.device = device
        self.channels = 0
        self.n_streams = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.opusgpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            e = OpusGpuError(f"{what} failed: {rc} ({self.lib.opusgpu_last_error(self.h).decode()})")
            e.code = rc
            raise e

    def streams_alloc(self, n, channels):
        self._chk(self.lib.opusgpu_streams_alloc(self.h, n, channels), "opusgpu_streams_alloc")
        self.n_streams, self.channels = n, channels

    def set_mode(self, rfc):
        """RFC mode on / off (include/opusgpu.h, OPUSGPU_MODE_RFC): frames at the durations their TOC names."""
        self._chk(self.lib.opusgpu_set_mode(self.h, 1 if rfc else 0), "opusgpu_set_mode")

    def set_pipeline(self, on):
        """Pipelined decode steps (include/opusgpu.h, opusgpu_set_pipeline): step k+1's CELT parse next to step k's
        reconstruction.  The tables of a decode_step_device call must then be complete in device memory at the call."""
        self._chk(self.lib.opusgpu_set_pipeline(self.h, 1 if on else 0), "opusgpu_set_pipeline")

    def streams_reset(self, first, count, full=True):
        self._chk(self.lib.opusgpu_streams_reset(self.h, first, count, 1 if full else 0), "opusgpu_streams_reset")

    def decode_packets_fec(self, stream_ids, packets, frame_capacity=1):
        """RFC mode: packets[i] FOLLOWS a lost packet of its stream; produces the lost packet's audio from packets[i]'s forward
        error correction data where it has any, by concealment otherwise (opusgpu_decode_packets_fec).  Decode the packets
        themselves with decode_packets afterwards."""
        return self.decode_packets(stream_ids, packets, frame_capacity, _fn="opusgpu_decode_packets_fec")

    def decode_packets(self, stream_ids, packets, frame_capacity=1, _fn="opusgpu_decode_packets"):
        """Batched opus_multistream_decode: returns (pcm[n, cap*960, ch] int16, result[n] int32).
        RFC mode: an empty (or None) packet is a LOST packet, concealed for as long as the stream's last packet was.
        Reference mode: an empty packet is what the reference makes of one (include/opusgpu.h "EMPTY PACKETS"): passes of an empty
        frame in the stream's last mode, 960 samples each, frame_capacity of them or until one fails."""
        packets = [b"" if p is None else p for p in packets]
        n = len(packets)
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        lens = np.array([len(p) for p in packets], dtype=np.int32)
        bufs = [C.create_string_buffer(bytes(p), max(len(p), 1)) for p in packets]
        ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        pcm = np.zeros((n, frame_capacity * FRAME, self.channels), dtype=np.int16)
        res = np.zeros(n, dtype=np.int32)
        self._chk(getattr(self.lib, _fn)(self.h, n, ids.ctypes.data, C.addressof(ptrs), lens.ctypes.data,
                                         pcm.ctypes.data, frame_capacity, res.ctypes.data), _fn)
        return pcm, res

    def decode_packets_arena(self, stream_ids, arena, offsets, lens, frame_capacity=1, pcm=None):
        """opusgpu_decode_packets for packets that lie in one uint8 array (packet i = arena[offsets[i] : offsets[i] +
        lens[i]]): the pointer table is made by numpy, not packet by packet -- at 65,536 packets per call the Python-side
        marshalling of decode_packets costs several times the call itself.  `pcm`: an int16 array to decode into
        (n, frame_capacity * 960, channels), reused between calls; a fresh one otherwise."""
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        offsets = np.asarray(offsets, dtype=np.int64)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        ids = np.ascontiguousarray(stream_ids, dtype=np.int32)
        n = len(lens)
        if len(offsets) != n or len(ids) != n:
            raise ValueError("stream_ids, offsets and lens must have one entry per packet")
        if n and (offsets.min() < 0 or (offsets + lens).max() > arena.size):
            raise ValueError("a packet lies outside the arena")
        ptrs = (np.uint64(arena.ctypes.data) + offsets.astype(np.uint64)).astype(np.uint64)
        shape = (n, frame_capacity * FRAME, self.channels)
        if pcm is None:
            pcm = np.empty(shape, dtype=np.int16)
            pcm[...] = 0
        elif pcm.shape != shape or pcm.dtype != np.int16 or not pcm.flags.c_contiguous:
            raise ValueError(f"pcm must be a C-contiguous int16 array of shape {shape}")
        res = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.opusgpu_decode_packets(self.h, n, ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data,
                                                  pcm.ctypes.data, frame_capacity, res.ctypes.data),
                  "opusgpu_decode_packets")
        return pcm, res

    def decode_packets_raw(self, ids, ptrs, lens, pcm, res, frame_capacity=1):
        """opusgpu_decode_packets with every table made by the caller beforehand (int32 ids / lens, uint64 packet addresses, int16
        pcm, int32 res; all C-contiguous, one entry per packet): nothing but the call itself -- what a C caller pays."""
        self._chk(self.lib.opusgpu_decode_packets(self.h, len(lens), ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data,
                                                  pcm.ctypes.data, frame_capacity, res.ctypes.data), "opusgpu_decode_packets")

    # ---- device-resident path -------------------------------------------------------------------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.opusgpu_dev_alloc(self.h, nbytes, C.byref(p)), "opusgpu_dev_alloc")
        return p

    def dev_free(self, p):
        self._chk(self.lib.opusgpu_dev_free(self.h, p), "opusgpu_dev_free")

    def h2d(self, dptr, arr):
        a = np.ascontiguousarray(arr)
        self._chk(self.lib.opusgpu_memcpy_h2d(self.h, dptr, a.ctypes.data, a.nbytes), "opusgpu_memcpy_h2d")

    def d2h(self, arr, dptr):
        self._chk(self.lib.opusgpu_memcpy_d2h(self.h, arr.ctypes.data, dptr, arr.nbytes), "opusgpu_memcpy_d2h")

    def debug_stage_taps(self, slot):
        """Stage taps of slot `slot` of the last decode_step_device call (test / debug entry, include/opusgpu.h)."""
        t = StageTaps()
        self._chk(self.lib.opusgpu_debug_stage_taps(self.h, slot, C.byref(t)), "opusgpu_debug_stage_taps")
        return t

    def decode_step_device(self, n, d_descs, d_arena, d_pcm, d_result, stream=None, modes=0):
        """modes: 0 = not known, else a mask of HAS_SILK / HAS_HYBRID / HAS_CELT (opusgpu_decode_step_device_modes)."""
        if modes:
            self._chk(self.lib.opusgpu_decode_step_device_modes(self.h, n, d_descs, d_arena, d_pcm, d_result, stream, modes),
                      "opusgpu_decode_step_device_modes")
        else:
            self._chk(self.lib.opusgpu_decode_step_device(self.h, n, d_descs, d_arena, d_pcm, d_result, stream),
                      "opusgpu_decode_step_device")

    def decode_steps_device(self, n, d_descs, d_arena, d_pcm, d_result, stream=None, modes=0):
        """A window of consecutive steps in one call (opusgpu_decode_steps_device): n is a list of frame counts, the others lists
        of device pointers, one entry per step."""
        k = len(n)

        def ptrs(v):
            return (C.c_void_p * k)(*[p.value if isinstance(p, C.c_void_p) else int(p) for p in v])
        counts = (C.c_int32 * k)(*[int(x) for x in n])
        self._chk(self.lib.opusgpu_decode_steps_device(self.h, k, counts, ptrs(d_descs), ptrs(d_arena), ptrs(d_pcm), ptrs(d_result), stream, modes),
                  "opusgpu_decode_steps_device")

    def pages_crc_device(self, n_pages, d_blob, d_offsets, d_lens, d_status, stream=None):
        """Page checksums on the GPU (include/opusgpu.h): d_status[i] = 1 match, 0 mismatch, PAGE_BAD_CAPTURE malformed."""
        self._chk(self.lib.opusgpu_pages_crc_device(self.h, n_pages, d_blob, d_offsets, d_lens, d_status, stream),
                  "opusgpu_pages_crc_device")

    def output_stage_device(self, n_blocks, block_samples, d_pcm, pcm_stride, d_i2s, i2s_stride, d_valid=None, valid_all=0,
                            d_cfgs=None, volume=64, force_mono=False, bits=16, channels=2, stream=None):
        """The player's output stage on the GPU (include/opusgpu.h): PCM blocks -> 32-bit I2S words."""
        cfg = OutputCfg(volume, 1 if force_mono else 0, bits, channels)
        self._chk(self.lib.opusgpu_output_stage_device(self.h, n_blocks, block_samples, d_pcm, pcm_stride, d_valid, valid_all,
                                                       d_cfgs, cfg, d_i2s, i2s_stride, stream), "opusgpu_output_stage_device")

    def tracks_assemble_device(self, n_segs, d_segs, d_pcm, row_samples, d_result, d_tracks, d_track_state, stream=None):
        """k_tracks_assemble (include/opusgpu.h WHOLE FILES): segments [TRACK_SEG_DTYPE] of a step's PCM rows -> the packed tracks."""
        self._chk(self.lib.opusgpu_tracks_assemble_device(self.h, n_segs, d_segs, d_pcm, row_samples, d_result, d_tracks, d_track_state,
                                                          stream), "opusgpu_tracks_assemble_device")

    def tracks_assemble_device_as(self, n_segs, d_segs, d_pcm, row_samples, d_result, format, d_place, d_tracks, d_track_state, stream=None):
        """opusgpu_tracks_assemble_device_as: the same into tracks of `format` (TRACKS_*), d_place a device array of TRACK_PLACE_DTYPE."""
        self._chk(self.lib.opusgpu_tracks_assemble_device_as(self.h, n_segs, d_segs, d_pcm, row_samples, d_result, format, d_place, d_tracks,
                                                             d_track_state, stream), "opusgpu_tracks_assemble_device_as")

    def tracks_resample_device(self, spans, d_in, channels, rate, mono, format, d_out, stream=None):
        """k_tracks_resample alone (include/opusgpu.h TRACK RATES): spans a HOST array of RESAMPLE_SPAN_DTYPE, d_in packed int16
        tracks, d_out the resampled ones in `format` (TRACKS_*).  Waits for the kernel."""
        spans = np.ascontiguousarray(spans, dtype=RESAMPLE_SPAN_DTYPE)
        self._chk(self.lib.opusgpu_tracks_resample_device(self.h, spans.size, spans.ctypes.data, d_in, channels, int(rate), 1 if mono else 0,
                                                          format, d_out, stream), "opusgpu_tracks_resample_device")

    def tracks_resample_mixed_device(self, spans, d_in, channels, rate, mix, format, d_out, stream=None):
        """k_tracks_resample_mix alone (include/opusgpu.h CHANNEL MIX): as tracks_resample_device, with `mix` an int16 Q14 matrix
        [out, in] or a MIX_MATRIX_DTYPE record in place of mono; d_out holds the matrix's rows as channels."""
        spans = np.ascontiguousarray(spans, dtype=RESAMPLE_SPAN_DTYPE)
        rec = mix if getattr(mix, "dtype", None) == MIX_MATRIX_DTYPE else mix_matrix(mix, channels)
        rec = np.ascontiguousarray(rec)
        self._chk(self.lib.opusgpu_tracks_resample_mixed_device(self.h, spans.size, spans.ctypes.data, d_in, channels, int(rate),
                                                                rec.ctypes.data, format, d_out, stream), "opusgpu_tracks_resample_mixed_device")

    def tracks_resample_ratio_device(self, spans, d_in, channels, up, down, mono, mix, format, d_out, stream=None):
        """k_tracks_resample_ratio alone (include/opusgpu.h TRACK RATIOS): as tracks_resample_device with up / down in place of the
        rate; mix: None, or what tracks_resample_mixed_device takes.  Waits for the kernel."""
        spans = np.ascontiguousarray(spans, dtype=RESAMPLE_SPAN_DTYPE)
        rec = None if mix is None else np.ascontiguousarray(mix if getattr(mix, "dtype", None) == MIX_MATRIX_DTYPE else mix_matrix(mix, channels))
        self._chk(self.lib.opusgpu_tracks_resample_ratio_device(self.h, spans.size, spans.ctypes.data, d_in, channels, int(up), int(down),
                                                                1 if mono else 0, None if rec is None else rec.ctypes.data, format, d_out,
                                                                stream), "opusgpu_tracks_resample_ratio_device")

    def tracks_mel_device(self, spans, d_in, n_mels, feature_layout, d_out, stream=None):
        """k_tracks_mel alone (include/opusgpu.h TRACK FEATURES): spans a HOST array of MEL_SPAN_DTYPE, d_in packed int16 mono tracks
        at 16 kHz, d_out the float32 feature tracks; feature_layout "bands" or "frames" (or a MEL_PARAMS_DTYPE record in place of
        n_mels).  Waits for the kernel."""
        spans = np.ascontiguousarray(spans, dtype=MEL_SPAN_DTYPE)
        rec = np.ascontiguousarray(n_mels) if getattr(n_mels, "dtype", None) == MEL_PARAMS_DTYPE else mel_params(n_mels, feature_layout)
        self._chk(self.lib.opusgpu_tracks_mel_device(self.h, spans.size, spans.ctypes.data, d_in, rec.ctypes.data, d_out, stream),
                  "opusgpu_tracks_mel_device")

    def tracks_fbank_device(self, spans, d_in, rec, d_out, stream=None):
        """k_tracks_fbank alone (include/opusgpu.h TRACK KALDI FEATURES): spans a HOST array of MEL_SPAN_DTYPE, d_in packed int16 mono
        tracks at the record's rate, rec a kaldi_fbank / kaldi_mfcc record, d_out the float32 feature tracks.  Waits for the kernel."""
        spans = np.ascontiguousarray(spans, dtype=MEL_SPAN_DTYPE)
        rec = _record(rec, *_FBANK)
        self._chk(self.lib.opusgpu_tracks_fbank_device(self.h, spans.size, spans.ctypes.data, d_in, rec.ctypes.data, d_out, stream),
                  "opusgpu_tracks_fbank_device")

    def tracks_feature_batch_device(self, spans, width, feature_layout, request, d_grid, d_out, stream=None):
        """k_feat_stats, k_feat_fold and k_feat_batch alone (include/opusgpu.h FEATURE BATCHES): spans a HOST array of FEAT_SPAN_DTYPE over
        the packed float32 grid d_grid of `width` bins in feature_layout ("bands" or "frames"), request a FeatureBatch
        (feature_batch_request), d_out the dense tensor of len(spans) * stride * width floats.  Waits for the kernels."""
        spans = np.ascontiguousarray(spans, dtype=FEAT_SPAN_DTYPE)
        vecs = [None if v is None else v.ctypes.data for v in (request.sub, request.mul)]
        self._chk(self.lib.opusgpu_tracks_feature_batch_device(self.h, spans.size, spans.ctypes.data, int(width), MEL_LAYOUTS[feature_layout],
                                                               request.rec.ctypes.data, *vecs, d_grid, d_out, stream),
                  "opusgpu_tracks_feature_batch_device")

    def tracks_stft_batch_device(self, spans, feature_layout, request, d_grid, d_out, stream=None):
        """k_stft_stats, k_stft_fold and k_stft_batch alone (include/opusgpu.h STFT BATCHES): spans a HOST array of STFT_BATCH_SPAN_DTYPE
        over the packed float32 grid d_grid in feature_layout ("bands" or "frames"), request a StftBatch (stft_batch_request: its bins
        and c are the grid's), d_out the dense tensor of len(spans) * stride * bins * c floats.  Waits for the kernels."""
        spans = np.ascontiguousarray(spans, dtype=STFT_BATCH_SPAN_DTYPE)
        vecs = [None if v is None else v.ctypes.data for v in (request.sub, request.mul)]
        self._chk(self.lib.opusgpu_tracks_stft_batch_device(self.h, spans.size, spans.ctypes.data, request.bins, request.c,
                                                            MEL_LAYOUTS[feature_layout], request.rec.ctypes.data, *vecs, d_grid, d_out, stream),
                  "opusgpu_tracks_stft_batch_device")

    def tracks_wave_trim_device(self, spans, channels, request, d_s16, stream=None):
        """k_wave_trim_energy and k_wave_trim_fold alone (include/opusgpu.h WAVE TRIM): spans a HOST array of WAVE_SPAN_DTYPE over the
        interleaved int16 tracks d_s16 of `channels` channels, request a trim_spec() record.  Waits for the kernels -> (the
        WAVE_TRIM_STAT_DTYPE records, the activity flags as a list of uint8 arrays -- one per track, one flag per frame -- or None
        where the request keeps none)."""
        spans = np.ascontiguousarray(spans, dtype=WAVE_SPAN_DTYPE)
        request = np.ascontiguousarray(request, dtype=WAVE_TRIM_REQ_DTYPE)
        stats = np.zeros(spans.size, dtype=WAVE_TRIM_STAT_DTYPE)
        frames = wave_trim_frames(spans["samples"], max(int(request["hop"][0]), 1))
        flags = np.zeros(int(frames.sum()), dtype=np.uint8) if int(request["flags"][0]) == 1 else None
        self._chk(self.lib.opusgpu_tracks_wave_trim_device(self.h, spans.size, spans.ctypes.data, int(channels), request.ctypes.data,
                                                           d_s16, stats.ctypes.data, None if flags is None else flags.ctypes.data,
                                                           stream),
                  "opusgpu_tracks_wave_trim_device")
        return stats, (None if flags is None else np.split(flags, np.cumsum(frames)[:-1]))

    def tracks_wave_batch_device(self, spans, channels, format, request, d_s16, d_out, stream=None):
        """k_wave_stats, k_wave_fold and k_wave_batch alone (include/opusgpu.h WAVE BATCHES): spans a HOST array of WAVE_SPAN_DTYPE over
        the interleaved int16 tracks d_s16 of `channels` channels, format "f32" or "f32_planar", request a WaveBatch
        (wave_batch_request), d_out the buffer of wave_batch_layout's floats.  Waits for the kernels -> the WAVE_STAT_DTYPE records."""
        spans = np.ascontiguousarray(spans, dtype=WAVE_SPAN_DTYPE)
        stats = np.zeros(spans.size, dtype=WAVE_STAT_DTYPE)
        self._chk(self.lib.opusgpu_tracks_wave_batch_device(self.h, spans.size, spans.ctypes.data, int(channels), TRACK_FORMATS[format],
                                                            request.rec.ctypes.data, d_s16, d_out, stats.ctypes.data, stream),
                  "opusgpu_tracks_wave_batch_device")
        return stats

    def tracks_melspec_device(self, spans, d_in, rec, d_out, stream=None):
        """k_tracks_melspec alone (include/opusgpu.h TRACK SPECTROGRAMS): spans a HOST array of MEL_SPAN_DTYPE, d_in packed int16 mono
        tracks at the record's rate, rec a mel_spec record, d_out the float32 feature tracks.  Waits for the kernel."""
        spans = np.ascontiguousarray(spans, dtype=MEL_SPAN_DTYPE)
        rec = _record(rec, *_SPEC)
        self._chk(self.lib.opusgpu_tracks_melspec_device(self.h, spans.size, spans.ctypes.data, d_in, rec.ctypes.data, d_out, stream),
                  "opusgpu_tracks_melspec_device")

    def tracks_stft_device(self, spans, d_in, rec, d_out, stream=None):
        """k_tracks_stft alone (include/opusgpu.h TRACK STFT): spans a HOST array of MEL_SPAN_DTYPE, d_in packed int16 mono tracks at
        the record's rate, rec a stft_spec record, d_out the float32 spectrogram tracks (pairs for the complex STFT).  Waits for the
        kernel."""
        spans = np.ascontiguousarray(spans, dtype=MEL_SPAN_DTYPE)
        rec = _record(rec, *_STFT)
        self._chk(self.lib.opusgpu_tracks_stft_device(self.h, spans.size, spans.ctypes.data, d_in, rec.ctypes.data, d_out, stream),
                  "opusgpu_tracks_stft_device")

    def tracks_loudness_device(self, spans, d_in, channels, weights=None, stream=None):
        """k_tracks_loudness_seg and k_tracks_loudness_gate alone (include/opusgpu.h TRACK LOUDNESS): spans a HOST array of
        LOUDNESS_SPAN_DTYPE, d_in packed int16 tracks of `channels` channels, weights None (the defaults) or one float per channel
        -> a LOUDNESS_DTYPE record per track.  Waits for the kernels."""
        spans = np.ascontiguousarray(spans, dtype=LOUDNESS_SPAN_DTYPE)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        if w is not None and w.shape != (channels,):
            raise ValueError(f"weights must have one entry per channel ({channels}), not shape {w.shape}")
        out = np.zeros(spans.size, dtype=LOUDNESS_DTYPE)
        self._chk(self.lib.opusgpu_tracks_loudness_device(self.h, spans.size, spans.ctypes.data, d_in, channels,
                                                          None if w is None else w.ctypes.data, out.ctypes.data, stream),
                  "opusgpu_tracks_loudness_device")
        return out

    def tracks_fill_tail(self, spans, format, channels, d_tracks, stream=None):
        """opusgpu_tracks_fill_tail_device: zero samples [first, end) of every track named by spans (TAIL_SPAN_DTYPE records, or
        rows of (track_offset, plane_samples, first, end)) in the device buffer d_tracks of `format` ("s16", "f32", "f32_planar")."""
        if not (isinstance(spans, np.ndarray) and spans.dtype == TAIL_SPAN_DTYPE):
            spans = np.array([tuple(int(v) for v in r) for r in spans], dtype=TAIL_SPAN_DTYPE)
        spans = np.ascontiguousarray(spans)
        self._chk(self.lib.opusgpu_tracks_fill_tail_device(self.h, spans.size, spans.ctypes.data, TRACK_FORMATS.get(format, format), channels,
                                                           d_tracks, stream), "opusgpu_tracks_fill_tail_device")

    def decode_files(self, files, rfc=False, flags=PAGES_GROUP_BY_MODE, threads=1, batch=None, format=None, scale=None, out=None,
                     rate=None, mono=False, mix=None, features=None, n_mels=80, feature_layout="bands", resample=None, loudness=None,
                     peak_limit=1.0, channel_weights=None, cuts=None, preroll=CUT_PREROLL, stride=None, feature_stride=None, normalize=None,
                     feature_pad=None, wave_stride=None, wave_normalize=None, wave_pad=None, wave_mask=False, stft_stride=None,
                     stft_normalize=None, stft_pad=None, wave_trim=None):
        """Whole Ogg Opus files -> (list of int16 arrays [samples, channels], one trimmed track per file, info).  The context's
        streams 0 .. len(files) - 1 are (re)allocated when there are too few and get fresh state; its mode is set to `rfc`.
        info: FILE_INFO_DTYPE records with two more fields: `final_status` (the first failed frame's code, else the plan's status)
        and `bad_packet` (that frame's packet, or -1); `track_samples` is the FINAL length.  batch: a FileBatch made beforehand
        from the same files (its channels and mode must be the context's).
        format: "s16", or "f32" (float32 [samples, channels]) or "f32_planar" (float32 [channels, samples]), every sample the
        int16 one times scale (include/opusgpu.h TRACK FORMATS).  scale: None (1 / 32768), "head_gain" (each file's OpusHead output
        gain applied as well) or one float per file.  out: a contiguous torch tensor on this context's GPU, of the format's dtype,
        128-byte aligned, with at least track_samples * channels elements: the tracks are decoded straight into it, nothing is
        copied to the host, and the tracks returned are views of it (ValueError before any device work if it does not fit).
        rate: 48000, or 24000 / 16000 / 12000 / 8000 for tracks decimated by D = 48000 / rate on the GPU (include/opusgpu.h TRACK
        RATES: an integer FIR over the int16 track, bit-exact); mono: one channel, (l + r + 1) >> 1 of a stereo track, at any rate.
        The tracks are then [ceil(len / D), 1 or channels] (planar: transposed), `out` is sized for them (track_rate_args), and
        info has `out_samples` and `out_offset` more; `track_samples` stays the final length at 48 kHz.
        mix: None, or a channel mix in front of the rate (include/opusgpu.h CHANNEL MIX; mix_matrix says what it may be: "mono",
        "stereo", a Q14 integer matrix [out, in] or a float one), at any rate, 48000 included; not together with mono=True.  The
        tracks are then [ceil(len / D), out] (planar: transposed), `out` is sized for them (track_mix_args).
        format and rate left out are "s16" and 48000.
        features: None, or "logmel" for log-mel features of the mono track at 16 kHz in place of the samples (include/opusgpu.h
        TRACK FEATURES: 400-sample Hann window, hop 160, n_mels = 80 or 128 Slaney bands, log10(max(mel, 1e-10))), made on the GPU
        in the same call.  It needs ONE channel -- mono=True or a mix of one row --, takes scale=, and refuses any rate but 16000 and
        any format but "f32" (track_feature_args).  The result is a list of float32 arrays [n_mels, F] (feature_layout "bands") or
        [F, n_mels] ("frames"), F = ceil(len / 3) // 160, or views of `out` (mel_layout's total floats); info has `feat_offset` more
        and its `frames` is F (the plan's count of Opus frames stays in batch.info["frames"]).  Whisper's clip-wide max - 8 clamp
        and (x + 4) / 4 are not applied: they are two torch operations on the result, or normalize="whisper" (below).
        resample: None, or (up, down) as for scipy.signal.resample_poly, or an output rate in Hz as an int, which is reduced against
        48000 -- 44100 is (147, 160), 32000 is (2, 3), 22050 is (147, 320) -- for tracks at 48000 up / down Hz by a rational FIR on
        the GPU (include/opusgpu.h TRACK RATIOS: integer arithmetic over the int16 track, bit-exact; track_ratio says which ratios
        there are).  mono, mix, format, scale and out act as with rate=: the tracks are [ceil(len up / down), output channels],
        `out` is sized for them (track_ratio_args) and info has `out_samples` and `out_offset` more.  Not together with rate= or
        features="logmel".
        features may also be a mel_spec() record: a mel spectrogram of the mono track at the record's sample_rate (include/opusgpu.h
        TRACK SPECTROGRAMS: n_fft, win_length, hop, n_mels, fmin / fmax, Slaney or HTK, power 1 or 2, log10 / ln / none and a floor
        are fields), with rate= or resample= naming that rate (or neither: the record's is taken), mono=True or a mix of one row,
        and scale=, out= and info as with "logmel"; n_mels= and feature_layout= are the record's (track_spectrogram_args).
        features may also be a kaldi_fbank() or kaldi_mfcc() record: Kaldi's fbank or MFCC features of the mono track at the record's
        sample_rate (include/opusgpu.h TRACK KALDI FEATURES), with the same keywords as for a mel_spec() record (track_kaldi_args);
        scale=1.0 gives Kaldi's int16-range convention.  The result is [F, n_mels or n_ceps] ("frames", the record's default).
        features may also be a stft_spec() record: the linear spectrogram of the mono track at the record's sample_rate, all
        n_fft / 2 + 1 bins as power, magnitude or the complex STFT with torch.stft's sign (include/opusgpu.h TRACK STFT), with the
        same keywords as for a mel_spec() record (track_stft_args).  The result is float32 [bins, F] ("bands") or [F, bins]
        ("frames"), complex64 for power=None (a view of the pairs; out= stays a float32 tensor of stft_layout's total floats).
        feature_stride=, normalize= and feature_pad= are refused with it: feature batches hold widths of 1 - 128.
        loudness: None, or "measure" for the integrated loudness (ITU-R BS.1770-4) and sample peak of every track, measured on the
        GPU on the 48 kHz int16 track in the same call (include/opusgpu.h TRACK LOUDNESS) -- the result is what it is without it,
        and info gains `lufs` (-inf: no block passed the gates), `peak`, `loudness_blocks`, `loudness_gated` and `gain` (1.0) --, or
        a target in LUFS (e.g. -23.0): every track is then scaled by loudness_gain(record, target, peak_limit) on top of scale=,
        `gain` says by how much, and the result must be a float format or features (ValueError otherwise, before any device
        work).  peak_limit: the largest sample peak a gain may leave (<= 0: none).  channel_weights: one weight per decoded channel
        in place of the defaults (loudness_weights).  The measurement is taken on all decoded channels, in front of mix and rate.
        cuts: None, or a sequence of (file, start, count) or (file, start, count, preroll) in samples at 48 kHz (cut_seconds makes
        them from seconds): the tracks are then these pieces of the files' whole-file tracks, one decoder stream per cut, each
        decoded from a reset decoder that starts at least `preroll` samples (default 3840: 80 ms, RFC 7845 section 4.6) in front of
        it (include/opusgpu.h WHOLE FILES / CUTS).  Tracks and info come back per cut; info gains `cut_first_packet`, `cut_packets`,
        `cut_lead`, `cut_exact` and `cut_start`.  A cut with `cut_exact` is the whole-file track's slice bit for bit, any other is
        not.  Every other keyword acts on the cuts as it does on files.  stride: None, or a multiple of 64 that holds every cut:
        track t then begins at t * stride and is zero from its final length to the stride; with out= (n_cuts * stride * channels
        elements) the result is that memory viewed as [n_cuts, stride, channels] ([n_cuts, channels, stride] planar) in place of
        the list.  A stride goes with format=, scale=, out= and loudness= on "s16" only (ValueError otherwise).
        feature_stride, normalize, feature_pad (with features= only; include/opusgpu.h FEATURE BATCHES): the features as ONE float32
        array [n, n_mels, S] ("bands") or [n, S, n_mels] ("frames") -- with out= (n * S * n_mels floats) a view of it --, every track
        normalised by statistics of its own info["frames"] real frames and padded to S = feature_stride frames (any integer that holds
        every planned track, 3000 for Whisper; None: the longest planned track's frames); info["feat_offset"] is t * S * n_mels.
        normalize: None, "whisper" ((max(x, track max - 8) + 4) / 4), "cmn" (per-bin mean removed, Kaldi's subtract_mean), "cmvn" (and
        divided by the per-bin standard deviation), ("affine", sub, mul) ((x - sub[j]) * mul[j], global CMVN), or a feature_norm()
        record with numbers of its own.  feature_pad: the pad cells' value, a number (verbatim) or (number, "normalized") for the
        track's normalisation of it; None is (-10, "normalized") under "whisper" -- the log-mel of zero audio, as Whisper pads --
        and 0 otherwise.  The batch's own stride= is still refused with features.
        wave_stride, wave_normalize, wave_pad, wave_mask (with format="f32" or "f32_planar", without features=; include/opusgpu.h WAVE
        BATCHES): the tracks -- at any rate=, resample=, mono= or mix= -- as ONE float32 array [n, S, channels] ([n, S] for one channel;
        "f32_planar": [n, channels, S]) -- with out= (wave_batch_layout's floats) a view of it --, every track padded with wave_pad (0)
        to S = wave_stride samples (any integer that holds every planned track; None: the longest) behind its info["out_samples"];
        info["out_offset"] is t * S.  wave_normalize: None, "zmuv" (zero mean and unit variance over the track's real samples of all
        channels, eps 1e-7 under the root as Wav2Vec2FeatureExtractor has it), ("zmuv", eps) or ("peak", target) (the largest |sample|
        becomes target), from exact integer statistics of the int16 track: info["wave_stats"] has them (WAVE_STAT_DTYPE) with the sub
        and mul applied, (y * scale - sub) * mul.  wave_mask=True: info["mask"] is the uint8 [n, S] attention mask, 1 on real samples.
        The batch's own stride= is still refused with these.
        wave_trim (a trim_spec() record; include/opusgpu.h WAVE TRIM): one of the wave keywords.  Every row of the dense tensor is the
        track without its leading and trailing silence -- librosa.effects.trim's indices from exact integer frame energies of the int16
        track, or an absolute dBFS gate --, and the statistics, the padding and the mask follow the trimmed track.  info["out_samples"]
        is the trimmed length, info["trim_start"] and info["trim_samples"] the samples kept, info["wave_trim"] the records
        (WAVE_TRIM_STAT_DTYPE: `full` the untrimmed length, emax, thr, frames, first, last, active) and, with trim_spec(flags=True),
        info["activity"] a list of uint8 arrays, one flag per frame (activity_intervals).
        stft_stride, stft_normalize, stft_pad (with a stft_spec() record as features= only; include/opusgpu.h STFT BATCHES): the
        spectrograms as ONE float32 array [n, bins, S] ("bands") or [n, S, bins] ("frames"), complex64 of that shape for power=None (a
        view of the pairs) -- with out= (a float32 tensor of n * S * bins floats, twice that for pairs) a view of it --, every track
        padded to S = stft_stride frames (any integer that holds every planned track; None: the longest planned track's frames)
        behind its info["frames"]; info["feat_offset"] is t * S * bins (* 2 for pairs).  stft_normalize: what normalize= takes, with
        vectors of `bins` entries, and "refmax" ((max(x, track max - 8) - track max) * 10: dB under the track's own maximum for a log10
        power spectrogram, top_db 80), or a stft_norm() record with numbers of its own; complex spectrograms take None and ("affine",
        sub, mul) only.  stft_pad: as feature_pad.  With stft_normalize None and S a multiple of 64 the kernel writes the tensor
        itself and no scratch grid is allocated.  The batch's own stride= is still refused."""
        if mix is not None and mono:  # (files_request's first refusal, ahead of the plan as it always was)
            raise ValueError("mix and mono=True exclude each other: the row {8192, 8192} is mono")
        own = batch is None
        if own:
            batch = FileBatch(files, channels=self.channels or 2, rfc=rfc, flags=flags, threads=threads, cuts=cuts, preroll=preroll,
                              stride=stride)
        try:
            req = files_request(batch, False, self.device, format, scale, out, rate, mono, mix, features, n_mels, feature_layout, resample,
                                loudness, peak_limit, channel_weights, feature_stride, normalize, feature_pad, wave_stride, wave_normalize,
                                wave_pad, wave_mask, stft_stride, stft_normalize, stft_pad, wave_trim)
            if self.n_streams < batch.n_files or self.channels != batch.channels:
                self.streams_alloc(max(batch.n_files, 1), batch.channels)
            self.set_mode(batch.rfc)
            return _run_files_request(req, self.lib, "opusgpu_", self.h, self._chk, batch, self)
        finally:
            if own:
                batch.close()

    def decode_step_by_kind(self, n_silk, n_hybrid, n_celt, d_descs, d_arena, d_pcm, d_result, keeps_kind=False, stream=None):
        """One step whose table is grouped by mode (OPUSGPU_PAGES_GROUP_BY_MODE: SILK-only, hybrid, CELT-only frames in that
        order), issued as up to three DECLARED sub-steps over the parts of the table, of d_pcm and of d_result: declared steps are
        what opusgpu_set_pipeline lets run ahead.  keeps_kind: OPUSGPU_STEP_KEEPS_MODE (include/opusgpu.h) -- the caller's word that
        a stream's mode never crosses between CELT-only and SILK-only / hybrid (config 5: it is fixed)."""
        def at(p, off):
            return C.c_void_p((p.value if isinstance(p, C.c_void_p) else int(p)) + off)
        if self.lib.opusgpu_get_mode(self.h) != 0:
            raise OpusGpuError("decode_step_by_kind: reference mode only (a frame's PCM block is 960 samples here; RFC mode's is 2880)")
        f0 = 0
        extra = STEP_KEEPS_MODE if keeps_kind else 0
        for cnt, mode in ((n_silk, HAS_SILK), (n_hybrid, HAS_HYBRID), (n_celt, HAS_CELT)):
            if cnt:
                self.decode_step_device(cnt, at(d_descs, 16 * f0), d_arena, at(d_pcm, f0 * 960 * self.channels * 2), at(d_result, 4 * f0),
                                        stream=stream, modes=mode | extra)
            f0 += cnt

    def decode_work_step(self, base, layout, k, d_pcm, d_result, by_kind=False, keeps_kind=False):
        """Step k of a packed work buffer (shard.pack_work / shard.WorkLayout) resident in HBM at address `base`: the
        step's descriptor table and the arena are used where they lie.  keeps_kind: OPUSGPU_STEP_KEEPS_MODE (a stream's mode is
        fixed): the step -- frames of every mode -- runs ahead like a declared one; by_kind: as three declared sub-steps
        (decode_step_by_kind), if the step's table is grouped by mode."""
        base = base.value if isinstance(base, C.c_void_p) else int(base)
        n = layout.counts[k]
        ns, nh = layout.mode_counts[k] if by_kind else (-1, -1)
        if ns >= 0:
            self.decode_step_by_kind(ns, nh, n - ns - nh, C.c_void_p(base + layout.desc_at[k]), C.c_void_p(base + layout.arena_at),
                                     d_pcm, d_result, keeps_kind=keeps_kind)
        else:
            self.decode_step_device(n, C.c_void_p(base + layout.desc_at[k]), C.c_void_p(base + layout.arena_at), d_pcm, d_result,
                                    modes=(HAS_SILK | HAS_HYBRID | HAS_CELT | STEP_KEEPS_MODE) if keeps_kind else 0)

    def synchronize(self):
        self._chk(self.lib.opusgpu_synchronize(self.h), "opusgpu_synchronize")

    def event(self):
        e = C.c_void_p()
        self._chk(self.lib.opusgpu_event_create(self.h, C.byref(e)), "opusgpu_event_create")
        return e

    def event_record(self, e):
        self._chk(self.lib.opusgpu_event_record(self.h, e), "opusgpu_event_record")

    def event_elapsed_ms(self, a, b):
        ms = C.c_float()
        self._chk(self.lib.opusgpu_event_elapsed_ms(self.h, a, b, C.byref(ms)), "opusgpu_event_elapsed_ms")
        return ms.value

    def event_destroy(self, e):
        self.lib.opusgpu_event_destroy(self.h, e)

    def event_synchronize(self, e):
        self._chk(self.lib.opusgpu_event_synchronize(self.h, e), "opusgpu_event_synchronize")

    # uploads next to the decode (include/opusgpu.h: opusgpu_upload_async and friends; ingest.py drives them)
    def upload_async(self, dptr, arr):
        """Queue a host -> HBM copy on the context's copy stream; `arr` must stay alive until a later fence has passed."""
        arr = np.ascontiguousarray(arr)
        self._chk(self.lib.opusgpu_upload_async(self.h, dptr, arr.ctypes.data, arr.nbytes), "opusgpu_upload_async")
        return arr

    def upload_fence(self, e):
        self._chk(self.lib.opusgpu_upload_fence(self.h, e), "opusgpu_upload_fence")

    def stream_wait_event(self, e, stream=None):
        self._chk(self.lib.opusgpu_stream_wait_event(self.h, e, stream), "opusgpu_stream_wait_event")

    def host_register(self, arr):
        self._chk(self.lib.opusgpu_host_register(self.h, arr.ctypes.data, arr.nbytes), "opusgpu_host_register")

    def host_unregister(self, arr):
        self._chk(self.lib.opusgpu_host_unregister(self.h, arr.ctypes.data), "opusgpu_host_unregister")


# ---- synthetic workloads ---------------------------------------------------
class MultistreamContext:
    """n_decoders multistream decoders of one layout (include/opusgpu.h, MULTISTREAM): `streams` elementary streams, the first
    `coupled` of them stereo, output channel c <- decoded channel mapping[c] (255: silent)."""

    def __init__(self, device, n_decoders, channels, streams, coupled, mapping=None):
        self.lib = load_lib()
        self.layout = ms_layout(channels, streams, coupled, mapping)
        h = C.c_void_p()
        rc = self.lib.opusgpu_ms_create(device, C.byref(self.layout), n_decoders, C.byref(h))
        if rc != 0:
            e = OpusGpuError(f"opusgpu_ms_create failed with {rc}")
            e.code = rc
            raise e
        self.h = h
        self.device = device
        self.n_decoders, self.channels, self.streams, self.coupled = n_decoders, channels, streams, coupled
        self.rfc = False

    def close(self):
        if getattr(self, "h", None):
            self.lib.opusgpu_ms_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            e = OpusGpuError(f"{what} failed: {rc} ({self.lib.opusgpu_ms_last_error(self.h).decode()})")
            e.code = rc
            raise e

    def set_mode(self, rfc):
        self._chk(self.lib.opusgpu_ms_set_mode(self.h, 1 if rfc else 0), "opusgpu_ms_set_mode")
        self.rfc = bool(rfc)

    def reset(self, first=0, count=None, full=True):
        count = self.n_decoders - first if count is None else count
        self._chk(self.lib.opusgpu_ms_reset(self.h, first, count, 1 if full else 0), "opusgpu_ms_reset")

    def decode_packets(self, decoder_ids, packets, frame_capacity=1, pcm=None):
        """Batched opus_multistream_decode: -> (pcm [n, cap*960, channels] int16, result [n] int32).  `pcm`: an array to decode
        into (blocks of failed packets keep what they held)."""
        packets = [b"" if p is None else bytes(p) for p in packets]
        n = len(packets)
        ids = np.ascontiguousarray(decoder_ids, dtype=np.int32)
        lens = np.array([len(p) for p in packets], dtype=np.int32)
        blob = np.frombuffer(b"".join(packets) + b"\0", dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64) if n else np.zeros(0, np.uint64)
        ptrs = (np.uint64(blob.ctypes.data) + offs).astype(np.uint64)
        shape = (n, frame_capacity * FRAME, self.channels)
        if pcm is None:
            pcm = np.zeros(shape, dtype=np.int16)
        elif pcm.shape != shape or pcm.dtype != np.int16 or not pcm.flags.c_contiguous:
            raise ValueError(f"pcm must be a C-contiguous int16 array of shape {shape}")
        res = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.opusgpu_ms_decode_packets(self.h, n, ids.ctypes.data, ptrs.ctypes.data, lens.ctypes.data, pcm.ctypes.data,
                                                     frame_capacity, res.ctypes.data), "opusgpu_ms_decode_packets")
        return pcm, res

    def decode_step_device(self, n, d_descs, d_arena, d_pcm, d_result, stream=None):
        """n rows of `streams` descriptors (DESC_DTYPE, stream field = decoder) in device memory -> d_pcm [n][960 * channels]
        (RFC mode: 2880 * channels), d_result [n]."""
        self._chk(self.lib.opusgpu_ms_decode_step_device(self.h, n, d_descs, d_arena, d_pcm, d_result, stream),
                  "opusgpu_ms_decode_step_device")

    def synchronize(self):
        self._chk(self.lib.opusgpu_ms_synchronize(self.h), "opusgpu_ms_synchronize")

    def tracks_assemble_device(self, n_segs, d_segs, d_pcm_coupled, d_pcm_mono, row_samples, d_res_coupled, d_res_mono, d_tracks,
                               d_track_state, stream=None):
        """k_ms_tracks_assemble (include/opusgpu.h WHOLE FILES / MULTISTREAM): segments [TRACK_SEG_DTYPE] of a step's ELEMENTARY PCM
        rows (coupled [rows * coupled, row_samples, 2], mono [rows * mono, row_samples]) -> the packed interleaved tracks."""
        self._chk(self.lib.opusgpu_ms_tracks_assemble_device(self.h, n_segs, d_segs, d_pcm_coupled, d_pcm_mono, row_samples, d_res_coupled,
                                                             d_res_mono, d_tracks, d_track_state, stream),
                  "opusgpu_ms_tracks_assemble_device")

    def tracks_assemble_device_as(self, n_segs, d_segs, d_pcm_coupled, d_pcm_mono, row_samples, d_res_coupled, d_res_mono, format, d_place,
                                  d_tracks, d_track_state, stream=None):
        """opusgpu_ms_tracks_assemble_device_as: the same into tracks of `format` (TRACKS_*), d_place a device array of TRACK_PLACE_DTYPE."""
        self._chk(self.lib.opusgpu_ms_tracks_assemble_device_as(self.h, n_segs, d_segs, d_pcm_coupled, d_pcm_mono, row_samples, d_res_coupled,
                                                                d_res_mono, format, d_place, d_tracks, d_track_state, stream),
                  "opusgpu_ms_tracks_assemble_device_as")

    def decode_files(self, files, rfc=False, threads=1, batch=None, format=None, scale=None, out=None, rate=None, mix=None, features=None,
                     n_mels=80, feature_layout="bands", resample=None, loudness=None, peak_limit=1.0, channel_weights=None, cuts=None,
                     preroll=CUT_PREROLL, stride=None, feature_stride=None, normalize=None, feature_pad=None, wave_stride=None,
                     wave_normalize=None, wave_pad=None, wave_mask=False, stft_stride=None, stft_normalize=None, stft_pad=None, wave_trim=None):
        """Whole Ogg Opus files of this object's layout -> (list of int16 arrays [samples, channels], one trimmed track per file,
        info), as Context.decode_files returns them: FILE_INFO_DTYPE records plus `final_status` and `bad_packet`, `track_samples`
        the FINAL length.  Decoders 0 .. len(files) - 1 get fresh state; the object's mode is set to the batch's.  batch: an
        MsFileBatch made beforehand from the same files (of this layout; `rfc` is then the batch's).  format, scale, out, rate: as
        for Context.decode_files, all channels at `rate`.  mix: as for Context.decode_files -- "mono" and "stereo" are the default
        downmix tables of the layout's channel count; there is no `mono` argument here.
        features, n_mels, feature_layout: as for Context.decode_files, with mix="mono" or a matrix of one row.
        resample: as for Context.decode_files, all channels or those of the mix.  features may be a mel_spec(), kaldi_fbank() or kaldi_mfcc() record as there.
        loudness, peak_limit, channel_weights: as for Context.decode_files; the default weights are those of the layout's channel
        count (1.41 for the rear pair, 0 for the LFE).  cuts, preroll, stride: as for Context.decode_files.
        feature_stride, normalize, feature_pad, wave_stride, wave_normalize, wave_pad, wave_mask, stft_stride, stft_normalize, stft_pad,
        wave_trim: as for Context.decode_files."""
        own = batch is None
        if own:
            batch = MsFileBatch(files, self.layout, rfc=rfc, threads=threads, cuts=cuts, preroll=preroll, stride=stride)
        mem = None
        try:
            req = files_request(batch, True, self.device, format, scale, out, rate, False, mix, features, n_mels, feature_layout, resample,
                                loudness, peak_limit, channel_weights, feature_stride, normalize, feature_pad, wave_stride, wave_normalize,
                                wave_pad, wave_mask, stft_stride, stft_normalize, stft_pad, wave_trim)
            mem = Context(self.device)  # (device memory and copies are a plain context's calls)
            self.set_mode(batch.rfc)
            return _run_files_request(req, self.lib, "opusgpu_ms_", self.h, self._chk, batch, mem)
        finally:
            if mem is not None:
                mem.close()
            if own:
                batch.close()


TOC_CELT_FB_STEREO = 0xFC
TOC_SILK_NB_STEREO = 0x0C
TOC_HYBRID_FB_STEREO = 0x7C


def lcg_payloads(n_streams, n_frames, payload_len, seed_base=0x9E3779B9):
    """Per-stream LCG payload bytes: x <- 1664525 x + 1013904223 (mod 2^32), byte = x >> 24,
    seed = seed_base ^ stream_id, running continuously over the stream's frames.
    Returns uint8 [n_frames, n_streams, payload_len]."""
    x = (np.uint32(seed_base) ^ np.arange(n_streams, dtype=np.uint32)).astype(np.uint32)
    out = np.empty((n_frames, n_streams, payload_len), dtype=np.uint8)
    a, c = np.uint32(1664525), np.uint32(1013904223)
    with np.errstate(over="ignore"):
        for f in range(n_frames):
            for i in range(payload_len):
                x = x * a + c
                out[f, :, i] = (x >> np.uint32(24)).astype(np.uint8)
    return out


_CRC_T = None


def ogg_crc_rows(rows):
    """Ogg page CRC-32 (polynomial 0x04c11db7, MSB first, zero start; src/ogg.cpp:439) of every row of a uint8 matrix,
    all rows in step: one table lookup per byte column."""
    global _CRC_T
    if _CRC_T is None:
        t = np.arange(256, dtype=np.uint64) << np.uint64(24)
        for _ in range(8):
            t = np.where(t & np.uint64(0x80000000), (t << np.uint64(1)) ^ np.uint64(0x04C11DB7), t << np.uint64(1)) & np.uint64(0xFFFFFFFF)
        _CRC_T = t.astype(np.uint32)
    crc = np.zeros(rows.shape[0], dtype=np.uint32)
    for j in range(rows.shape[1]):
        crc = (crc << np.uint32(8)) ^ _CRC_T[(crc >> np.uint32(24)) ^ rows[:, j]]
    return crc


def build_pages(toc, payloads, serials, seqno=2, granule_step=960):
    """Synthetic Ogg pages, one per stream: page s carries payloads[:, s] as code-0 packets (TOC + payload each).
    payloads uint8 [packets, n, L] with L + 1 < 255 (one lacing value per packet).  Returns uint8 [n, page_len]:
    "OggS", version 0, header type 0, granule position packets * granule_step, serial number, page sequence number,
    CRC, segment table, packets (src/ogg.cpp:439-480 for the layout the reference checks)."""
    npk, n, L = payloads.shape
    if L + 1 >= 255 or npk > 255:
        raise ValueError("one lacing value per packet, at most 255 packets")
    hdr = 27 + npk
    pages = np.zeros((n, hdr + npk * (L + 1)), dtype=np.uint8)
    pages[:, 0:4] = np.frombuffer(b"OggS", dtype=np.uint8)
    pages[:, 6:14] = np.frombuffer(np.int64(npk * granule_step).tobytes(), dtype=np.uint8)
    pages[:, 14:18] = np.asarray(serials, dtype="<u4").reshape(n, 1).view(np.uint8)
    pages[:, 18:22] = np.frombuffer(np.uint32(seqno).tobytes(), dtype=np.uint8)
    pages[:, 26] = npk
    pages[:, 27:hdr] = L + 1
    body = pages[:, hdr:].reshape(n, npk, L + 1)
    body[:, :, 0] = toc
    body[:, :, 1:] = payloads.transpose(1, 0, 2)
    pages[:, 22:26] = ogg_crc_rows(pages).astype("<u4").reshape(n, 1).view(np.uint8)
    return pages


def silk_header_key(first_payload_bytes, stereo):
    """What a SILK-only / hybrid frame's header will make its decoder do, read off the frame's first byte: the VAD and LBRR flags
    are the range coder's first symbols, each of probability 1/2 -- exactly the byte's top bits (reference src/silk.cpp:1568-1573:
    VAD flag and LBRR flag of the mid channel, then of the side channel).  -> 2-bit key: bit 0 the mid channel carries an LBRR
    frame, bit 1 the side channel does (each is a whole extra frame of side information and pulses that the decoder must read
    past, src/silk.cpp:1590-1616).  Frames handed to the lane-per-frame parse kernel in key order make its waves uniform: a wave
    whose 32 frames have no LBRR data skips those passes instead of idling through them.  The bit positions are those of
    a frame decoded as 20 ms -- every frame in reference mode (Q6), the only mode with such steps."""
    b = np.asarray(first_payload_bytes, dtype=np.uint8)
    key = (b >> 6) & 1
    if stereo:
        key = key | (((b >> 4) & 1) << 1)
    return key.astype(np.uint8)


def build_step(toc, payloads, order_by_header=False):
    """Arena + descriptors for one decode step: payloads uint8 [n_streams, L], one code-0 packet each.
    The arena holds TOC + payload per stream; descriptors point past the TOC byte.
    order_by_header: the table in the order of silk_header_key (stable; SILK-only / hybrid TOCs only) -- slot j of the step's
    PCM and results then belongs to stream descs["stream"][j]."""
    n, L = payloads.shape
    arena = np.empty((n, L + 1), dtype=np.uint8)
    arena[:, 0] = toc
    arena[:, 1:] = payloads
    if toc & 0x80:
        mode, bw = 2, ((toc >> 5) & 3)
        bw = 0 if bw == 0 else bw + 1
    elif (toc & 0x60) == 0x60:
        mode, bw = 1, (4 if toc & 0x10 else 3)
    else:
        mode, bw = 0, (toc >> 5) & 3
    flags = mode | (bw << 2) | (32 if toc & 4 else 0)
    descs = np.zeros(n, dtype=DESC_DTYPE)
    descs["stream"] = np.arange(n, dtype=np.int32)
    descs["offset"] = np.arange(n, dtype=np.int32) * (L + 1) + 1
    descs["len"] = L
    descs["flags"] = flags
    if order_by_header and mode != 2 and L > 0:
        descs = descs[np.argsort(silk_header_key(payloads[:, 0], bool(toc & 4)), kind="stable")]
    return arena.reshape(-1), descs
