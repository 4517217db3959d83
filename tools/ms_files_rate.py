#!/usr/bin/env python3
"""Whole multistream files rate (include/opusgpu.h, WHOLE FILES / MULTISTREAM): N 5.1 files (6 channels, 4 streams, 2 coupled) of one
page of 10 packets, CELT-FB 20 ms frames of 160 bytes on every elementary stream, random pre-skips and end trims of 0 - 2,000
samples, planned once and decoded device-resident.  Per batch of 10 steps, mean and spread over --reps repeats, the two variants
interleaved:
(A) the batch's 10 steps through opusgpu_ms_decode_step_device: split, both halves, k_ms_map into [rows][960 * 6]; no trimming.
    Host clock around the 10 calls and a synchronise.
(B) the same 10 steps inside opusgpu_ms_files_decode, k_ms_tracks_assemble behind each instead of the map.  The call uploads the
    batch first, so its steps are timed by the library itself, with events around the step loop (opusgpu_ms_files_last_steps_ms).
The kernels' own times come from a kernel trace: run this script under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR
-o msfiles --` and then `python3 tools/ms_files_rate.py --stats DIR` reads DIR's kernel_stats.csv (k_ms_tracks_assemble: per batch
it reads and writes the kept samples x 6 channels x 2 bytes each, k_ms_tracks_assemble_f32 reads 2 bytes and writes 4; k_ms_map:
ms_rate.py's count per step).
--format f32 | f32_planar: the whole call per track format instead (tools/format_rate.py).
--rate R: the whole call at a track rate instead (tools/resample_rate.py).
--rate R --mix mono | stereo: the same through the 5.1 default downmix table (opusgpu_ms_files_decode_mixed).
--rate R [--mix M] --wave-batch S[:NORM] [--packets-per-file P]: the fused call under a wave-batch request (include/opusgpu.h WAVE
BATCHES) next to the packed float32 call followed by padding, normalising and masking in torch (tools/wave_rate.py, as
tools/files_rate.py --wave-batch).  With --wave-trim TOPDB[:FL:HOP] as well: the fused call under both requests (WAVE TRIM) next to
the call without the trim and to the packed int16 call followed by the same trim and collate in torch, as tools/files_rate.py has it.
--mel [--n-mels N]: the fused log-mel call (opusgpu_ms_files_decode_mel through the default mono downmix) next to float32 16 kHz mono
tracks followed by torch.stft, the filterbank matmul and log10, and k_tracks_mel's share of the call (tools/mel_rate.py).
--melspec tts | kaldi | clap | music | sep | big [--melspec-algo dense | fft] [--melspec-layout bands | frames]: the fused mel-spectrogram call (opusgpu_ms_files_decode_melspec through the default mono downmix)
next to float32 mono tracks at the set's rate followed by torch.stft, the filterbank matmul, the floor and the log, and
k_tracks_melspec's share of the call (tools/mel_rate.py: compare_spec).
--stft SET --stft-batch S[:NORM]: the dense STFT call (include/opusgpu.h STFT BATCHES; opusgpu_ms_set_stft_batch) on both paths next to the
packed call and the packed call followed by padding and normalising in torch (tools/mel_rate.py: compare_stft_batch).
--stft tiny | enh | vits | wide | whisper_lin | fft_tiny | fft_enh | fft_vits | fft_wide | fft_sep | fft_big [--stft-layout bands | frames]
[--stft-algo dense | fft]: the fused linear / complex STFT call
(opusgpu_ms_files_decode_stft through the default mono downmix; include/opusgpu.h TRACK STFT) next to float32 mono tracks at the set's
rate followed by torch.stft, abs / abs ** 2 / nothing, the floor and the log, and k_tracks_stft's share of the call (tools/mel_rate.py:
compare_stft).
--fbank wenet | mfcc | mfcc8k | wide: the fused Kaldi fbank / MFCC call (opusgpu_ms_files_decode_fbank through the default mono downmix)
next to float32 mono tracks at the set's rate followed by unfold, mean, pre-emphasis, window, rfft, matmul and log in torch, and
k_tracks_fbank's share of the call (tools/mel_rate.py: compare_fbank); a set at 16 kHz is followed by --melspec kaldi's line.
--resample UP/DOWN [--mix M]: the fused ratio call (opusgpu_ms_files_decode_ratio) next to rate=24000 on the same corpus and to
float32 48 kHz tracks resampled by a polyphase conv1d in torch, and the two kernels alone (tools/ratio_rate.py).
--loudness [TARGET] [--packets-per-file P]: what a loudness request adds to the float32 call at 48 kHz (include/opusgpu.h TRACK
LOUDNESS; tools/loudness_rate.py): without the request, with loudness="measure" and, with a TARGET in LUFS, normalising --
interleaved; the added time per call and its share of the call.  P (at most 80: one page) packets per file in place of 10: tracks
need 400 ms for a block.
--cuts C [--cut-seconds S] [--stride] [--packets-per-file P]: the files (one page, P <= 80 packets) decoded whole, then C random cuts
of S seconds out of each as N x C tracks (include/opusgpu.h WHOLE FILES / CUTS; tools/cuts_rate.py, as tools/files_rate.py --cuts).
usage (GPU box): python3 tools/ms_files_rate.py [--n N] [--reps R] [--loudness [T] [--packets-per-file P] | --format F | --rate R [--mix M] | --resample U/D [--mix M] | --mel [--n-mels N] | --melspec SET | --stft SET | --fbank SET] | python3 tools/ms_files_rate.py --stats DIR [--n N]"""
import argparse
import ctypes as C
import glob
import importlib.util
import json
import os
import sys
import time

import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(here, "..", "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--stats", default=None)
ap.add_argument("--format", choices=["f32", "f32_planar"], default=None,
                help="compare the whole decode call: int16 tracks, int16 + conversion in torch, the fused float format (tools/format_rate.py)")
ap.add_argument("--rate", type=int, choices=[24000, 16000, 12000, 8000], default=None,
                help="compare the whole decode call: int16 tracks, int16 + resampling in torch, the resampled tracks (tools/resample_rate.py)")
ap.add_argument("--mix", choices=["mono", "stereo"], default=None, help="with --rate: the 5.1 default downmix table as a channel mix")
ap.add_argument("--resample", default=None, metavar="UP/DOWN",
                help="compare the fused ratio call with rate=24000 and with 48 kHz float tracks + a polyphase conv1d in torch (tools/ratio_rate.py)")
ap.add_argument("--mel", action="store_true", help="compare the fused log-mel call with 16 kHz mono float tracks + torch.stft (tools/mel_rate.py)")
ap.add_argument("--n-mels", type=int, choices=[80, 128], default=80)
ap.add_argument("--melspec", choices=["tts", "kaldi", "clap", "music", "sep", "big"], default=None,
                help="compare the fused mel-spectrogram call with float mono tracks at the set's rate + torch.stft (tools/mel_rate.py)")
ap.add_argument("--stft", choices=["tiny", "enh", "vits", "wide", "whisper_lin", "fft_tiny", "fft_enh", "fft_vits", "fft_wide", "fft_sep", "fft_big"], default=None,
                help="compare the fused STFT call with float mono tracks at the set's rate + torch.stft (tools/mel_rate.py: compare_stft)")
ap.add_argument("--stft-layout", choices=["bands", "frames"], default="bands", help="with --stft: the record's feature_layout")
ap.add_argument("--melspec-algo", choices=["dense", "fft"], default=None,
                help="with --melspec: the record's algorithm (mel_spec's algo=; default: the set's own, dense but for sep and big, which are fft only)")
ap.add_argument("--melspec-layout", choices=["bands", "frames"], default="bands", help="with --melspec: the record's feature_layout")
ap.add_argument("--stft-algo", choices=["dense", "fft"], default=None,
                help="with --stft: the record's algorithm (stft_spec's algo=; default: the set's own, dense for the sets without fft_)")
ap.add_argument("--stft-batch", default=None, metavar="S[:NORM]",
                help="with --stft: the dense call with an STFT-batch request (stride S, 0: the longest track; none, whisper, refmax, cmn or cmvn) "
                     "next to the packed call followed by padding and normalising in torch (tools/mel_rate.py: compare_stft_batch)")
ap.add_argument("--fbank", choices=["wenet", "mfcc", "mfcc8k", "wide"], default=None,
                help="compare the fused Kaldi fbank / MFCC call with float mono tracks at the set's rate + unfold / rfft in torch (tools/mel_rate.py)")
ap.add_argument("--loudness", nargs="?", const="measure", default=None, metavar="TARGET",
                help="what a loudness request adds to the float32 call, measuring and (with a target in LUFS) normalising (tools/loudness_rate.py)")
ap.add_argument("--wave-batch", default=None, metavar="S[:NORM]",
                help="with --rate: the fused call with a wave-batch request (stride S, 0: the longest track; none, zmuv or peak) next to the "
                     "packed float32 call followed by padding, normalising and masking in torch (tools/wave_rate.py)")
ap.add_argument("--wave-trim", default=None, metavar="TOPDB[:FL:HOP]",
                help="with --wave-batch: the fused call with a trim request as well (include/opusgpu.h WAVE TRIM; frame 2048, hop 512) next to "
                     "the call without it and to the packed int16 call followed by the same trim and collate in torch (tools/wave_rate.py)")
ap.add_argument("--packets-per-file", type=int, default=10, help="with --loudness, --cuts or --wave-batch: packets of 20 ms per file, at most 80")
ap.add_argument("--cuts", type=int, default=None, metavar="C", help="C random cuts per file next to the whole files (tools/cuts_rate.py)")
ap.add_argument("--cut-seconds", type=float, default=0.5, metavar="S")
ap.add_argument("--stride", action="store_true", help="with --cuts: cuts of unequal length, packed and at a stride with zeroed tails")
ap.add_argument("--whole-reps", type=int, default=3, help="with --cuts: timed whole-file batches")
args = ap.parse_args()
if args.cuts is not None and (args.fbank or args.loudness or args.melspec or args.mel or args.resample or args.rate or args.format or args.mix):
    ap.error("--cuts goes alone (with --cut-seconds, --stride, --n, --packets-per-file, --reps, --whole-reps)")
if args.fbank and (args.rate or args.format or args.resample or args.mel or args.melspec or args.loudness or args.mix):
    ap.error("--fbank goes alone")
if args.loudness and (args.format or args.rate or args.mel or args.melspec or args.resample or args.mix):
    ap.error("--loudness goes alone")
if args.wave_batch and not args.rate:
    ap.error("--wave-batch goes with --rate R")
if args.wave_trim and not args.wave_batch:
    ap.error("--wave-trim goes with --wave-batch")
if args.packets_per_file != 10 and (not (args.loudness or args.cuts is not None or args.wave_batch) or not 1 <= args.packets_per_file <= 80):
    ap.error("--packets-per-file goes with --loudness, --cuts or --wave-batch and is at most 80: the files have one page")
if args.melspec and (args.rate or args.format or args.resample or args.mel):
    ap.error("--melspec goes without --rate, --resample, --format and --mel")
if args.stft and (args.rate or args.format or args.resample or args.mel or args.melspec or args.fbank or args.loudness or args.mix or
                  args.cuts is not None):
    ap.error("--stft goes alone (with --stft-layout, --n, --reps)")
if args.stft_batch and not args.stft:
    ap.error("--stft-batch goes with --stft")
if args.stft_algo and not args.stft:
    ap.error("--stft-algo goes with --stft")
if (args.melspec_algo or args.melspec_layout != "bands") and not args.melspec:
    ap.error("--melspec-algo and --melspec-layout go with --melspec")
if args.melspec in ("sep", "big") and args.melspec_algo == "dense":
    ap.error("--melspec sep and big have no dense leg: n_fft 4096 and 8192 are algo='fft' only")
if args.mix and not (args.rate or args.resample):
    ap.error("--mix goes with --rate or --resample")
if args.mel and (args.rate or args.format or args.resample):
    ap.error("--mel goes without --rate, --resample and --format")
if args.resample and (args.rate or args.format):
    ap.error("--resample goes without --rate and --format")
if args.format or args.rate or args.mel or args.resample or args.melspec or args.stft or args.fbank:
    import torch  # before the library is loaded: one HIP runtime for both
n = args.n

spec = importlib.util.spec_from_file_location("esp32_opus_player_amd", os.path.join(here, "..", "esp32-opus-player_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pkg)
import files_util as fu  # noqa: E402
import ms_files_util as mf  # noqa: E402
import ogg_util  # noqa: E402

LAYOUT = (6, 4, 2, [0, 4, 1, 2, 3, 5])
CH, S, CP, L, PACKETS = 6, 4, 2, 160, args.packets_per_file
rng = np.random.default_rng(3)
pre = rng.integers(0, 2001, n)
trim = rng.integers(0, 2001, n)
kept = int((PACKETS * 960 - pre - trim).sum())  # samples per channel of all tracks
MOVED = 2 * kept * CH * 2                       # bytes the fused assembly reads + writes per batch
MAP_BYTES = n * (2 * 960 * 2 * 2 + 2 * 960 * 2) + n * 960 * 6 * 2  # k_ms_map, per full step

if args.stats:
    import csv
    rows = []
    for f in glob.glob(os.path.join(args.stats, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    out = []
    for key, per_launch in (("k_ms_tracks_assemble", MOVED / PACKETS), ("k_ms_map", MAP_BYTES), ("k_tracks_assemble", None)):
        for r in rows:
            if r["Name"].startswith(key) or ("void " + key) in r["Name"]:
                if key == "k_ms_tracks_assemble" and "_f32" in r["Name"]:
                    per_launch = MOVED * 3 / 2 / PACKETS  # float tracks: 2 bytes in, 4 bytes out
                elif key == "k_ms_tracks_assemble":
                    per_launch = MOVED / PACKETS
                avg_ms = float(r["AverageNs"]) / 1e6
                o = {"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_ms_per_launch": round(avg_ms, 4),
                     "min_ms": round(float(r["MinNs"]) / 1e6, 4), "max_ms": round(float(r["MaxNs"]) / 1e6, 4)}
                if per_launch:
                    o["bytes_per_launch"] = int(per_launch)
                    o["tb_per_s"] = round(per_launch / (avg_ms / 1e3) / 1e12, 2)
                out.append(o)
    assert out, "neither kernel in the kernel statistics"
    print(json.dumps(out))
    raise SystemExit(0)


def crc_fill(rows):
    rows[:, 22:26] = 0
    rows[:, 22:26] = pkg.ogg_crc_rows(rows).astype("<u4").reshape(-1, 1).view(np.uint8)


# ---- the files, numpy all the way --------------------------------------------------------------------------------------------
serial = np.arange(n, dtype=np.uint32) + 1000
head = np.frombuffer(ogg_util.page(0, 0, 0, [mf.head(LAYOUT, 0)], bos=True), dtype=np.uint8)
tags = np.frombuffer(ogg_util.page(0, 1, 0, [ogg_util.opus_tags()]), dtype=np.uint8)
H, T = np.tile(head, (n, 1)), np.tile(tags, (n, 1))
for rows in (H, T):
    rows[:, 14:18] = serial.astype("<u4").reshape(n, 1).view(np.uint8)
H[:, 28 + 10:28 + 12] = pre.astype("<u2").reshape(n, 1).view(np.uint8)  # 27 + 1 lacing value, then OpusHead: pre-skip at 10
crc_fill(H)
crc_fill(T)
# a multistream packet: [TOC, 160, payload] for streams 0 - 2 (self-delimited), [TOC, payload] for stream 3
PK = (S - 1) * (L + 2) + (L + 1)
lacing = fu.raw_page(0, 2, 0, mf.lace(PK) * PACKETS, b"")  # the page header with the segment table, no body yet
hdr = len(lacing)
page = np.zeros((n, hdr + PACKETS * PK), dtype=np.uint8)
page[:, :hdr] = np.frombuffer(lacing, dtype=np.uint8)
page[:, 5] = 4  # end of stream
page[:, 6:14] = (PACKETS * 960 - trim).astype("<i8").reshape(n, 1).view(np.uint8)
page[:, 14:18] = serial.astype("<u4").reshape(n, 1).view(np.uint8)
pay = pkg.lcg_payloads(n, PACKETS * S, L, seed_base=3 * 7919 + 1)  # [PACKETS * S, n, L]
body = page[:, hdr:].reshape(n, PACKETS, PK)
at = 0
for s in range(S):
    body[:, :, at] = 0xFC if s < CP else 0xF8  # CELT FB 20 ms, stereo / mono
    at += 1
    if s != S - 1:
        body[:, :, at] = L
        at += 1
    body[:, :, at:at + L] = pay[s::S].transpose(1, 0, 2)
    at += L
crc_fill(page)
files = np.concatenate([H, T, page], axis=1)
blobs = [r.tobytes() for r in files]
del files, page, pay

t0 = time.perf_counter()
b = pkg.MsFileBatch(blobs, LAYOUT, threads=args.threads)
plan_s = time.perf_counter() - t0
assert (b.info["status"] == 0).all() and b.n_steps == PACKETS, (np.unique(b.info["status"]), b.n_steps)
assert (b.info["track_samples"] == PACKETS * 960 - pre - trim).all()

if args.cuts is not None:  # F files of P <= 80 packets whole, then C cuts of S seconds out of each (tools/cuts_rate.py)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import cuts_rate
    b.close()
    ms = pkg.MultistreamContext(0, n * args.cuts, *LAYOUT)
    ms.set_mode(False)
    mem = pkg.Context(0)  # (device memory is a plain context's call)
    print(json.dumps(cuts_rate.compare(
        pkg, mem, lambda **kw: pkg.MsFileBatch(blobs, LAYOUT, threads=args.threads, **kw),
        lambda bt, d, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode(ms.h, bt.h, d, ln, st), "opusgpu_ms_files_decode"), blobs, args.cuts,
        args.cut_seconds, args.stride, args.reps, args.whole_reps, 3, f"5.1 CELT-FB, {args.threads} planner threads")))
    mem.close()
    ms.close()
    raise SystemExit(0)

if args.loudness:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import loudness_rate
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    ms.set_mode(b.rfc)
    mem = pkg.Context(0)  # (device memory is a plain context's call)
    target = None if args.loudness == "measure" else float(args.loudness)
    print(json.dumps(loudness_rate.compare(pkg, mem, ms.lib, "opusgpu_ms_", ms.h, ms._chk, b, True, args.reps, target,
                                           f"5.1, 48 kHz f32, {PACKETS} packets per file", format="f32")))
    mem.close()
    ms.close()
    raise SystemExit(0)

if args.format:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import format_rate
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    print(json.dumps(format_rate.compare(torch, pkg, ms.lib.opusgpu_ms_files_decode_as, ms.h, ms._chk, b, args.format, args.reps, "in_order")))
    ms.close()
    raise SystemExit(0)

if args.rate:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import resample_rate
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    rec = pkg.mix_matrix(args.mix, CH) if args.mix else None

    def resampled(fmt, d, oo, ol, ln, st):
        if rec is not None:
            return ms._chk(ms.lib.opusgpu_ms_files_decode_mixed(ms.h, b.h, args.rate, rec.ctypes.data, fmt, None, d, oo, ol, ln, st),
                           "opusgpu_ms_files_decode_mixed")
        return ms._chk(ms.lib.opusgpu_ms_files_decode_resampled(ms.h, b.h, args.rate, fmt, None, d, oo, ol, ln, st),
                       "opusgpu_ms_files_decode_resampled")
    if args.wave_batch:
        import wave_rate
        stride, norm = wave_rate.wave_batch_arg(args.wave_batch)
        if args.wave_trim:
            print(json.dumps(wave_rate.compare_wave_trim(
                torch, pkg, resampled,
                lambda wb: ms._chk(ms.lib.opusgpu_ms_set_wave_batch(ms.h, None if wb is None else wb.rec.ctypes.data), "opusgpu_ms_set_wave_batch"),
                lambda tr: ms._chk(ms.lib.opusgpu_ms_set_wave_trim(ms.h, None if tr is None else tr.ctypes.data), "opusgpu_ms_set_wave_trim"),
                b, 1, 48000 // args.rate, int(rec["out_channels"][0]) if rec is not None else CH, stride, norm,
                wave_rate.wave_trim_arg(pkg, args.wave_trim), args.reps, f"5.1 CELT-FB, {PACKETS} packets per file, in_order")))
            ms.close()
            raise SystemExit(0)
        print(json.dumps(wave_rate.compare_wave_batch(
            torch, pkg, resampled,
            lambda wb: ms._chk(ms.lib.opusgpu_ms_set_wave_batch(ms.h, None if wb is None else wb.rec.ctypes.data), "opusgpu_ms_set_wave_batch"),
            b, 1, 48000 // args.rate, int(rec["out_channels"][0]) if rec is not None else CH, stride, norm, args.reps,
            f"5.1 CELT-FB, {PACKETS} packets per file, in_order")))
        ms.close()
        raise SystemExit(0)
    print(json.dumps(resample_rate.compare(
        torch, pkg, lambda d, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode(ms.h, b.h, d, ln, st), "opusgpu_ms_files_decode"), resampled,
        b, args.rate, False, args.reps, "in_order", mix=pkg.downmix_matrix(CH, 1 if args.mix == "mono" else 2) if args.mix else None)))
    ms.close()
    raise SystemExit(0)

if args.resample:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ratio_rate
    up, down = pkg.track_ratio(tuple(int(v) for v in args.resample.split("/")))
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    mem = pkg.Context(0)  # the kernels alone are a plain context's calls
    rec = pkg.mix_matrix(args.mix, CH) if args.mix else None
    rec_p = None if rec is None else rec.ctypes.data

    def at_24000(fmt, d, oo, ol, ln, st):
        if rec is not None:
            return ms._chk(ms.lib.opusgpu_ms_files_decode_mixed(ms.h, b.h, 24000, rec_p, fmt, None, d, oo, ol, ln, st), "opusgpu_ms_files_decode_mixed")
        return ms._chk(ms.lib.opusgpu_ms_files_decode_resampled(ms.h, b.h, 24000, fmt, None, d, oo, ol, ln, st), "opusgpu_ms_files_decode_resampled")

    def at_24000_kernel(spans, d_in, fmt, d_out):
        if rec is not None:
            return mem.tracks_resample_mixed_device(spans, d_in, CH, 24000, rec, fmt, d_out)
        return mem.tracks_resample_device(spans, d_in, CH, 24000, False, fmt, d_out)
    print(json.dumps(ratio_rate.compare(
        torch, pkg,
        lambda d, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode_as(ms.h, b.h, pkg.TRACKS_F32, None, d, ln, st), "opusgpu_ms_files_decode_as"),
        at_24000,
        lambda fmt, d, oo, ol, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode_ratio(ms.h, b.h, up, down, rec_p, fmt, None, d, oo, ol, ln, st),
                                               "opusgpu_ms_files_decode_ratio"),
        lambda d, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode(ms.h, b.h, d, ln, st), "opusgpu_ms_files_decode"),
        (lambda spans, d_in, fmt, d_out: mem.tracks_resample_ratio_device(spans, d_in, CH, up, down, False, rec, fmt, d_out), at_24000_kernel),
        b, up, down, False, args.reps, "in_order", mix=pkg.downmix_matrix(CH, 1 if args.mix == "mono" else 2) if args.mix else None)))
    mem.close()
    ms.close()
    raise SystemExit(0)

if args.fbank:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mel_rate
    maker, kw, up, down = mel_rate.FBANK_SETS[args.fbank]
    frec = getattr(pkg, maker)(**kw)
    rate = 48000 // down
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    mem = pkg.Context(0)
    rec = pkg.mix_matrix("mono", CH)

    def tracks(fmt, d, oo, ol, ln, st):
        return ms._chk(ms.lib.opusgpu_ms_files_decode_mixed(ms.h, b.h, rate, rec.ctypes.data, fmt, None, d, oo, ol, ln, st), "opusgpu_ms_files_decode_mixed")
    print(json.dumps(mel_rate.compare_fbank(
        torch, pkg, tracks,
        lambda p, d, fo, fr, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode_fbank(ms.h, b.h, rate, 0, 0, rec.ctypes.data, p, None, d, fo, fr, ln, st),
                                             "opusgpu_ms_files_decode_fbank"),
        lambda spans, d_in, r, d_out: mem.tracks_fbank_device(spans, d_in, r, d_out), b, frec, up, down, args.reps, f"{args.fbank}, in_order")), flush=True)
    if rate == 16000:  # k_tracks_melspec's share at the same files
        print(json.dumps(mel_rate.compare_spec(
            torch, pkg, tracks,
            lambda p, d, fo, fr, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode_melspec(ms.h, b.h, rate, 0, 0, rec.ctypes.data, p, None, d, fo, fr, ln, st),
                                                 "opusgpu_ms_files_decode_melspec"),
            lambda spans, d_in, r, d_out: mem.tracks_melspec_device(spans, d_in, r, d_out), b, pkg.mel_spec(**mel_rate.SPEC_SETS["kaldi"][0]), up, down,
            args.reps, "melspec kaldi, in_order")))
    mem.close()
    ms.close()
    raise SystemExit(0)

if args.melspec:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mel_rate
    srec, up, down = mel_rate.spec_record(pkg, args.melspec, args.melspec_layout, args.melspec_algo)
    rate = 48000 // down if up == 1 else 0
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    mem = pkg.Context(0)
    rec = pkg.mix_matrix("mono", CH)

    def tracks(fmt, d, oo, ol, ln, st):
        if rate:
            return ms._chk(ms.lib.opusgpu_ms_files_decode_mixed(ms.h, b.h, rate, rec.ctypes.data, fmt, None, d, oo, ol, ln, st),
                           "opusgpu_ms_files_decode_mixed")
        return ms._chk(ms.lib.opusgpu_ms_files_decode_ratio(ms.h, b.h, up, down, rec.ctypes.data, fmt, None, d, oo, ol, ln, st),
                       "opusgpu_ms_files_decode_ratio")
    print(json.dumps(mel_rate.compare_spec(
        torch, pkg, tracks,
        lambda p, d, fo, fr, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode_melspec(ms.h, b.h, rate, 0 if rate else up, 0 if rate else down,
                                                                                    rec.ctypes.data, p, None, d, fo, fr, ln, st),
                                             "opusgpu_ms_files_decode_melspec"),
        lambda spans, d_in, r, d_out: mem.tracks_melspec_device(spans, d_in, r, d_out), b, srec, up, down, args.reps, f"{args.melspec}, in_order")))
    mem.close()
    ms.close()
    raise SystemExit(0)

if args.stft:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mel_rate
    srec, up, down = mel_rate.stft_record(pkg, args.stft, args.stft_layout, args.stft_algo)
    rate = 48000 // down if up == 1 else 0
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    mem = pkg.Context(0)
    rec = pkg.mix_matrix("mono", CH)

    def tracks(fmt, d, oo, ol, ln, st):
        if rate:
            return ms._chk(ms.lib.opusgpu_ms_files_decode_mixed(ms.h, b.h, rate, rec.ctypes.data, fmt, None, d, oo, ol, ln, st),
                           "opusgpu_ms_files_decode_mixed")
        return ms._chk(ms.lib.opusgpu_ms_files_decode_ratio(ms.h, b.h, up, down, rec.ctypes.data, fmt, None, d, oo, ol, ln, st),
                       "opusgpu_ms_files_decode_ratio")
    def decode_stft(p, d, fo, fr, ln, st):
        return ms._chk(ms.lib.opusgpu_ms_files_decode_stft(ms.h, b.h, rate, 0 if rate else up, 0 if rate else down, rec.ctypes.data, p, None, d,
                                                           fo, fr, ln, st), "opusgpu_ms_files_decode_stft")

    def set_stft_batch(sb):
        """The STFT-batch request `sb` (a StftBatch; None: off) on the multistream decoder."""
        vecs = [None, None] if sb is None else [None if v is None else v.ctypes.data for v in (sb.sub, sb.mul)]
        ms._chk(ms.lib.opusgpu_ms_set_stft_batch(ms.h, None if sb is None else sb.rec.ctypes.data, *vecs, 0 if sb is None else sb.bins),
                "opusgpu_ms_set_stft_batch")
    print(json.dumps(mel_rate.compare_stft(
        torch, pkg, tracks, decode_stft, lambda spans, d_in, r, d_out: mem.tracks_stft_device(spans, d_in, r, d_out), b, srec, up, down, args.reps,
        f"{args.stft} {args.stft_layout}, in_order")), flush=True)
    if args.stft_batch:
        S, norm = mel_rate.stft_batch_arg(args.stft_batch)
        print(json.dumps(mel_rate.compare_stft_batch(
            torch, pkg, decode_stft, set_stft_batch, mem.tracks_stft_batch_device, mem.tracks_feature_batch_device, b, srec, up, down, S, norm,
            args.reps, f"{args.stft} {args.stft_layout}, in_order")), flush=True)
    mem.close()
    ms.close()
    raise SystemExit(0)

if args.mel:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import mel_rate
    ms = pkg.MultistreamContext(0, n, *LAYOUT)
    mem = pkg.Context(0)
    rec = pkg.mix_matrix("mono", CH)
    print(json.dumps(mel_rate.compare(
        torch, pkg,
        lambda fmt, d, oo, ol, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode_mixed(ms.h, b.h, 16000, rec.ctypes.data, fmt, None, d, oo, ol, ln, st),
                                               "opusgpu_ms_files_decode_mixed"),
        lambda p, d, fo, fr, ln, st: ms._chk(ms.lib.opusgpu_ms_files_decode_mel(ms.h, b.h, rec.ctypes.data, p, None, d, fo, fr, ln, st),
                                             "opusgpu_ms_files_decode_mel"),
        lambda spans, d_in, mp, d_out: mem.tracks_mel_device(spans, d_in, mp, None, d_out), b, args.n_mels, args.reps, "in_order")))
    mem.close()
    ms.close()
    raise SystemExit(0)

# ---- (A) and (B), interleaved --------------------------------------------------------------------------------------------------
ctx = pkg.Context(0)
ms = pkg.MultistreamContext(0, n, *LAYOUT)
steps = [b.step(k) for k in range(PACKETS)]
descs = np.concatenate([s[0].reshape(-1) for s in steps])
d_descs, d_arena = ctx.dev_alloc(descs.nbytes), ctx.dev_alloc(b.arena.nbytes)
d_pcm, d_res = ctx.dev_alloc(n * 960 * CH * 2), ctx.dev_alloc(4 * n)
d_tracks = ctx.dev_alloc(max(int(b.track_samples), 1) * CH * 2)
ctx.h2d(d_descs, descs)
ctx.h2d(d_arena, b.arena)
lengths = np.zeros(n, dtype=np.int64)
status = np.zeros((n, 2), dtype=np.int32)


def run_a():
    ms.reset()
    at = 0
    t0 = time.perf_counter()
    for k in range(PACKETS):
        m = len(steps[k][1])
        ms.decode_step_device(m, C.c_void_p(d_descs.value + 16 * S * at), d_arena, d_pcm, d_res)
        at += m
    ms.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run_b():
    t0 = time.perf_counter()
    ms._chk(ms.lib.opusgpu_ms_files_decode(ms.h, b.h, d_tracks, lengths.ctypes.data, status.ctypes.data), "opusgpu_ms_files_decode")
    return ms.lib.opusgpu_ms_files_last_steps_ms(), (time.perf_counter() - t0) * 1e3


run_a()
run_b()
a, w, call = [], [], []
for _ in range(args.reps):
    a.append(run_a())
    x, y = run_b()
    w.append(x)
    call.append(y)
assert (status[:, 0] == 0).all() and (lengths == b.info["track_samples"]).all()
res = np.zeros(n, np.int32)
ctx.d2h(res, d_res)
assert (res == 960).all(), np.unique(res)[:8]
spread = max(a) - min(a)
print(json.dumps({"layout": "5.1", "files": n, "reps": args.reps, "bytes_moved_by_assembly_per_batch": MOVED, "map_bytes_per_step": MAP_BYTES,
                  "plan_files_per_s": round(n / plan_s), "plan_threads": args.threads,
                  "a_ms_steps_ms": round(float(np.mean(a)), 3), "a_min_max_ms": [round(min(a), 3), round(max(a), 3)], "a_spread_ms": round(spread, 3),
                  "b_files_steps_ms": round(float(np.mean(w)), 3), "b_min_max_ms": [round(min(w), 3), round(max(w), 3)],
                  "b_minus_a_ms": round(float(np.mean(w) - np.mean(a)), 3), "condition_b_le_a_plus_spread": bool(np.mean(w) <= np.mean(a) + spread),
                  "b_whole_call_ms": round(float(np.mean(call)), 3)}))
ms.close()
ctx.close()
