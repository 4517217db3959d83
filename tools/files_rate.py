#!/usr/bin/env python3
"""Whole-file path rate (include/opusgpu.h, WHOLE FILES): N stereo files of one page of 10 CELT-FB packets of 160 bytes, random
pre-skips and end trims, planned once and decoded device-resident.  Per batch of 10 steps, mean and spread over --reps repeats:
(a) the steps alone (the path without this feature), (b) the steps with k_tracks_assemble behind each on the same stream,
(d) a device-to-device hipMemcpyAsync of the bytes the assembly moves, in the same process -- in order and with pipelined steps.
(c), the kernel's own time, comes from a kernel trace: run this script under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o files --`
and then `python3 tools/files_rate.py --stats DIR` reads DIR's kernel_stats.csv (bytes read + written per launch: 2 x the step's
kept samples x 4).  Also: the planner's files/s on --threads threads next to opusgpu_pages_demux's pages/s on the same pages.
--format f32 | f32_planar: the whole call per track format instead (tools/format_rate.py), in order and pipelined; --stats then
reads the float kernels' rows too (6 bytes moved per sample and channel instead of 4).
--rate R [--mono]: the whole call at a track rate instead (tools/resample_rate.py), in order and pipelined; --stats then prints
k_tracks_resample's row as well.
--rate R --mix mono | stereo: the same with the default downmix table as a channel mix (opusgpu_files_decode_mixed) in place of
--mono; `--mix mono` and `--mono` produce the same tracks, so their times show what the general staging costs.
--mel [--n-mels N]: the fused log-mel call (opusgpu_files_decode_mel, mono) next to float32 16 kHz mono tracks followed by
torch.stft, the filterbank matmul and log10, and k_tracks_mel's share of the call (tools/mel_rate.py).
--melspec tts | kaldi | clap | music | sep | big [--melspec-algo dense | fft] [--melspec-layout bands | frames]: the fused mel-spectrogram call (opusgpu_files_decode_melspec, mono; include/opusgpu.h TRACK
SPECTROGRAMS) at that set's rate next to float32 mono tracks at the rate followed by torch.stft, the filterbank matmul, the floor and
the log, and k_tracks_melspec's share of the call (tools/mel_rate.py: compare_spec).
--stft SET --stft-batch S[:NORM] [--stft-batch-only] [--pipe in_order | pipelined]: the dense STFT call (include/opusgpu.h STFT BATCHES)
with the request as asked, without a norm on the general and on the direct path, next to the packed call and the packed call followed by
padding and normalising in torch; the stage alone beside k_feat_batch, and the peak device memory of both paths (tools/mel_rate.py:
compare_stft_batch).
--stft tiny | enh | vits | wide | whisper_lin | fft_tiny | fft_enh | fft_vits | fft_wide | fft_sep | fft_big [--stft-layout bands | frames]
[--stft-algo dense | fft]: the fused linear / complex STFT call
(opusgpu_files_decode_stft, mono; include/opusgpu.h TRACK STFT) at that set's rate next to float32 mono tracks at the rate followed by
torch.stft, abs / abs ** 2 / nothing, the floor and the log, k_tracks_stft's share of the call and the bytes it writes per second
(tools/mel_rate.py: compare_stft).
--fbank wenet | mfcc | mfcc8k | wide: the fused Kaldi fbank / MFCC call (opusgpu_files_decode_fbank, mono; include/opusgpu.h TRACK KALDI
FEATURES) against float mono tracks at the set's rate followed by the torch restatement (unfold, mean, pre-emphasis, window, rfft,
matmul, log), and k_tracks_fbank's share of the call (tools/mel_rate.py: compare_fbank); a set at 16 kHz is followed by --melspec
kaldi's line at the same files, for the two kernels' shares side by side.
--feature-batch S[:NORM] with --mel or --fbank: the fused call under a feature-batch request (include/opusgpu.h FEATURE BATCHES; one
dense padded tensor, NORM none | whisper | cmn | cmvn) next to the packed call followed by the gather into a padded tensor and the
normalisation in torch (tools/mel_rate.py: compare_feature_batch).
--rate R [--mono | --mix M] --wave-batch S[:NORM] [--packets-per-file P]: the fused call under a wave-batch request (include/opusgpu.h
WAVE BATCHES; one dense padded float32 tensor and its mask, S 0: the longest planned track, NORM none | zmuv | peak) next to the packed
float32 call followed by the gather into a padded tensor, the normalisation and the mask in torch (tools/wave_rate.py).
--rate R ... --wave-batch S[:NORM] --wave-trim TOPDB[:FL:HOP]: that fused call with a trim request as well (include/opusgpu.h WAVE
TRIM; TOPDB under the track's loudest frame, frames of FL every HOP, 2048 and 512 by default) next to the call without the trim and
to the packed int16 call followed by the same trim, gather, normalisation and mask in torch (tools/wave_rate.py: compare_wave_trim).
--packets-per-file P: files of P packets of 20 ms (in pages of at most 250) in place of the default 10, for --mel and --melspec: long
tracks, whose tiles are full.
--resample UP/DOWN [--mono | --mix M]: the fused ratio call (opusgpu_files_decode_ratio, include/opusgpu.h TRACK RATIOS) next to
rate=24000 on the same corpus and to float32 48 kHz tracks resampled by a polyphase conv1d in torch, interleaved, and the two
kernels alone per output sample (tools/ratio_rate.py).
--loudness [TARGET] [--rate R --mono] [--packets-per-file P]: what a loudness request adds to the call (include/opusgpu.h TRACK
LOUDNESS; tools/loudness_rate.py): float32 tracks at 48 kHz, or mono ones at --rate, without the request, with loudness="measure"
and, with a TARGET in LUFS, normalising -- interleaved; the added time per call and its share of the call.  Tracks need 400 ms for
a block: --packets-per-file 500 gives 10 s files.
--cuts C --cut-seconds S [--stride] --n F --packets-per-file P: F long files of P packets decoded whole, then C random cuts of S
seconds out of each as F x C tracks (include/opusgpu.h WHOLE FILES / CUTS; tools/cuts_rate.py), pipelined: both times, audio seconds
out per second for both, both planner times, the pre-roll's share; --stride adds cuts of unequal length packed and strided, whose
difference is what the zeroed tails cost.  --stats DIR --tail-bytes B reads k_tracks_fill_tail's row of a kernel trace of that run.
usage (GPU box): python3 tools/files_rate.py [--n N] [--reps R] [--loudness [T] |--format F | --rate R [--mono | --mix M] | --resample U/D [--mono | --mix M] | --mel [--n-mels N] | --melspec SET | --stft SET | --fbank SET] [--packets-per-file P] | python3 tools/files_rate.py --stats DIR [--n N]"""
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
sys.path.insert(0, here)
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=65536)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--stats", default=None)
ap.add_argument("--format", choices=["f32", "f32_planar"], default=None,
                help="compare the whole decode call: int16 tracks, int16 + conversion in torch, the fused float format (tools/format_rate.py)")
ap.add_argument("--rate", type=int, choices=[48000, 24000, 16000, 12000, 8000], default=None,
                help="compare the whole decode call: int16 tracks, int16 + resampling in torch, the resampled tracks (tools/resample_rate.py)")
ap.add_argument("--mono", action="store_true")
ap.add_argument("--mix", choices=["mono", "stereo"], default=None, help="with --rate: the default downmix table as a channel mix")
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
                help="with --stft: the dense call with an STFT-batch request (stride S, 0: the longest track; none, whisper, refmax, cmn or cmvn), "
                     "on the general and the direct path, next to the packed call followed by padding and normalising in torch, and the stage "
                     "alone beside k_feat_batch (tools/mel_rate.py: compare_stft_batch)")
ap.add_argument("--stft-batch-only", action="store_true", help="with --stft-batch: skip compare_stft's legs")
ap.add_argument("--pipe", choices=["both", "in_order", "pipelined"], default="both", help="with --stft or --melspec: which step order to time")
ap.add_argument("--fbank", choices=["wenet", "mfcc", "mfcc8k", "wide"], default=None,
                help="compare the fused Kaldi fbank / MFCC call with float mono tracks at the set's rate + unfold / rfft in torch (tools/mel_rate.py)")
ap.add_argument("--feature-batch", default=None, metavar="S[:NORM]",
                help="with --mel or --fbank: the fused call with a feature-batch request (stride S; none, whisper, cmn or cmvn) next to the "
                     "packed call followed by padding and normalising in torch (tools/mel_rate.py: compare_feature_batch)")
ap.add_argument("--wave-batch", default=None, metavar="S[:NORM]",
                help="with --rate: the fused call with a wave-batch request (stride S, 0: the longest track; none, zmuv or peak) next to the "
                     "packed float32 call followed by padding, normalising and masking in torch (tools/wave_rate.py)")
ap.add_argument("--wave-trim", default=None, metavar="TOPDB[:FL:HOP]",
                help="with --wave-batch: the fused call with a trim request as well (include/opusgpu.h WAVE TRIM; frame 2048, hop 512) next to "
                     "the call without it and to the packed int16 call followed by the same trim and collate in torch (tools/wave_rate.py)")
ap.add_argument("--packets-per-file", type=int, default=10,
                help="with --mel, --melspec, --fbank, --loudness or --wave-batch: packets of 20 ms per file")
ap.add_argument("--loudness", nargs="?", const="measure", default=None, metavar="TARGET",
                help="what a loudness request adds to the float32 call, measuring and (with a target in LUFS) normalising (tools/loudness_rate.py)")
ap.add_argument("--cuts", type=int, default=None, metavar="C", help="C random cuts per file next to the whole files (tools/cuts_rate.py)")
ap.add_argument("--cut-seconds", type=float, default=10.0, metavar="S")
ap.add_argument("--stride", action="store_true", help="with --cuts: cuts of unequal length, packed and at a stride with zeroed tails")
ap.add_argument("--tail-bytes", type=int, default=None, help="with --stats: stride.tail_bytes_s16 of the traced --cuts --stride run")
ap.add_argument("--whole-reps", type=int, default=3, help="with --cuts: timed whole-file batches (a step per packet: long)")
args = ap.parse_args()
if args.cuts is not None and (args.fbank or args.loudness or args.melspec or args.mel or args.resample or args.rate or args.format or args.mix or
                              args.mono):
    ap.error("--cuts goes alone (with --cut-seconds, --stride, --n, --packets-per-file, --reps, --whole-reps)")
if args.fbank and (args.rate or args.format or args.resample or args.mel or args.melspec or args.loudness or args.mix or args.mono):
    ap.error("--fbank goes alone")
if args.loudness and (args.format or args.mel or args.melspec or args.resample or args.mix or (args.rate and not args.mono)):
    ap.error("--loudness goes alone or with --rate R --mono")
if args.melspec and (args.rate or args.format or args.resample or args.mel):
    ap.error("--melspec goes without --rate, --resample, --format and --mel")
if args.stft and (args.rate or args.format or args.resample or args.mel or args.melspec or args.fbank or args.loudness or args.mix or args.mono or
                  args.cuts is not None):
    ap.error("--stft goes alone (with --stft-layout, --n, --packets-per-file, --reps)")
if (args.stft_batch or args.stft_batch_only) and not args.stft:
    ap.error("--stft-batch goes with --stft")
if args.stft_algo and not args.stft:
    ap.error("--stft-algo goes with --stft")
if (args.melspec_algo or args.melspec_layout != "bands") and not args.melspec:
    ap.error("--melspec-algo and --melspec-layout go with --melspec")
if args.melspec in ("sep", "big") and args.melspec_algo == "dense":
    ap.error("--melspec sep and big have no dense leg: n_fft 4096 and 8192 are algo='fft' only")
if args.feature_batch and not (args.mel or args.fbank):
    ap.error("--feature-batch goes with --mel or --fbank")
if args.wave_batch and (not args.rate or args.loudness or (args.rate == 48000 and not (args.mono or args.mix))):
    ap.error("--wave-batch goes with --rate R, and at 48000 with --mono or --mix")
if args.wave_trim and not args.wave_batch:
    ap.error("--wave-trim goes with --wave-batch")
if args.packets_per_file != 10 and not (args.mel or args.melspec or args.stft or args.fbank or args.loudness or args.cuts is not None or
                                        args.wave_batch):
    ap.error("--packets-per-file goes with --mel, --melspec, --stft, --fbank, --loudness, --cuts or --wave-batch")
if args.mix and (args.mono or not (args.rate or args.resample)):
    ap.error("--mix goes with --rate or --resample and without --mono")
if args.mel and (args.rate or args.format or args.resample):
    ap.error("--mel goes without --rate, --resample and --format")
if args.resample and (args.rate or args.format):
    ap.error("--resample goes without --rate and --format")
n = args.n
if (args.format or args.rate or args.mel or args.resample or args.melspec or args.stft or args.fbank) and not args.loudness:
    import torch  # before the library: one HIP runtime for both

spec = importlib.util.spec_from_file_location("esp32_opus_player_amd", os.path.join(here, "..", "esp32-opus-player_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pkg)
import files_util as fu  # noqa: E402

PAGES = -(-args.packets_per_file // 250)
PER_PAGE = -(-args.packets_per_file // PAGES)  # (a count that no number of equal pages makes is rounded up)
files, pre, trim = fu.bulk_files(pkg, n, pkg.TOC_CELT_FB_STEREO, 160, pages=PAGES, per_page=PER_PAGE)
kept = int((960 * PAGES * PER_PAGE - pre - trim).sum())  # samples per channel of all tracks
MOVED = 2 * kept * 4                           # bytes the assembly reads + writes per batch

if args.stats:
    import csv
    rows = []
    for f in glob.glob(os.path.join(args.stats, "**", "*kernel_stats.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if any(k in r["Name"] for k in ("k_tracks_assemble", "k_tracks_resample", "k_tracks_fill_tail"))]
    assert rows, "no k_tracks_assemble in the kernel statistics"
    for r in rows:
        if "k_tracks_fill_tail" in r["Name"]:  # one launch per strided batch; --tail-bytes: what the run's record says it zeroes
            o = {"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_ms_per_launch": round(float(r["AverageNs"]) / 1e6, 4),
                 "min_ms": round(float(r["MinNs"]) / 1e6, 4), "max_ms": round(float(r["MaxNs"]) / 1e6, 4)}
            if args.tail_bytes:
                o["bytes_per_launch"], o["tb_per_s"] = args.tail_bytes, round(args.tail_bytes / (float(r["AverageNs"]) / 1e9) / 1e12, 2)
            print(json.dumps(o))
            continue
        if "k_tracks_resample" in r["Name"]:  # one launch per batch; its bytes depend on rate and format: time only
            print(json.dumps({"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_ms_per_launch": round(float(r["AverageNs"]) / 1e6, 4),
                              "min_ms": round(float(r["MinNs"]) / 1e6, 4), "s16_bytes_read_per_batch": MOVED // 2}))
            continue
        avg_ms = float(r["AverageNs"]) / 1e6
        moved = MOVED * 3 // 2 if "_f32" in r["Name"] else MOVED  # float tracks: 2 bytes in, 4 bytes out
        print(json.dumps({"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "avg_ms_per_launch": round(avg_ms, 4),
                          "min_ms": round(float(r["MinNs"]) / 1e6, 4), "ms_per_batch_of_10": round(avg_ms * 10, 3),
                          "bytes_per_batch": moved, "tb_per_s": round(moved / 10 / (avg_ms / 1e3) / 1e12, 2)}))
    raise SystemExit(0)

if args.cuts is not None:
    import cuts_rate
    blobs = [r.tobytes() for r in files]
    ctx = pkg.Context(0)
    ctx.streams_alloc(n * args.cuts, 2)
    ctx.set_pipeline(1)
    ctx.set_mode(False)
    print(json.dumps(cuts_rate.compare(
        pkg, ctx, lambda **kw: pkg.FileBatch(blobs, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads, **kw),
        lambda b, d, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode(ctx.h, b.h, d, ln, st), "opusgpu_files_decode"), blobs, args.cuts,
        args.cut_seconds, args.stride, args.reps, args.whole_reps, 3, f"stereo CELT-FB, {args.threads} planner threads, pipelined")))
    ctx.close()
    raise SystemExit(0)

if args.loudness:
    import loudness_rate
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == PAGES * PER_PAGE
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)
    ctx.set_mode(b.rfc)
    kw = dict(rate=args.rate, mono=True, format="f32") if args.rate else dict(format="f32")
    target = None if args.loudness == "measure" else float(args.loudness)
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        ctx.set_pipeline(pipe)
        what = f"stereo, {'%d Hz mono' % args.rate if args.rate else '48 kHz'} f32, {PAGES * PER_PAGE} packets per file, {name}"
        print(json.dumps(loudness_rate.compare(pkg, ctx, ctx.lib, "opusgpu_", ctx.h, ctx._chk, b, False, args.reps, target, what, **kw)), flush=True)
    ctx.close()
    raise SystemExit(0)

if args.format:
    import format_rate
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == 10
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        ctx.set_pipeline(pipe)
        print(json.dumps(format_rate.compare(torch, pkg, ctx.lib.opusgpu_files_decode_as, ctx.h, ctx._chk, b, args.format, args.reps, name)))
    ctx.close()
    raise SystemExit(0)

if args.rate:
    import resample_rate
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == PAGES * PER_PAGE
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)
    rec = pkg.mix_matrix(args.mix, 2) if args.mix else None

    def resampled(fmt, d, oo, ol, ln, st):
        if rec is not None:
            return ctx._chk(ctx.lib.opusgpu_files_decode_mixed(ctx.h, b.h, args.rate, rec.ctypes.data, fmt, None, d, oo, ol, ln, st),
                            "opusgpu_files_decode_mixed")
        return ctx._chk(ctx.lib.opusgpu_files_decode_resampled(ctx.h, b.h, args.rate, int(args.mono), fmt, None, d, oo, ol, ln, st),
                        "opusgpu_files_decode_resampled")
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        ctx.set_pipeline(pipe)
        if args.wave_batch:
            import wave_rate
            S, norm = wave_rate.wave_batch_arg(args.wave_batch)
            set_batch = lambda wb: ctx._chk(ctx.lib.opusgpu_set_wave_batch(ctx.h, None if wb is None else wb.rec.ctypes.data), "opusgpu_set_wave_batch")
            channels = 1 if args.mono else int(rec["out_channels"][0]) if rec is not None else 2
            if args.wave_trim:
                print(json.dumps(wave_rate.compare_wave_trim(
                    torch, pkg, resampled, set_batch,
                    lambda tr: ctx._chk(ctx.lib.opusgpu_set_wave_trim(ctx.h, None if tr is None else tr.ctypes.data), "opusgpu_set_wave_trim"),
                    b, 1, 48000 // args.rate, channels, S, norm, wave_rate.wave_trim_arg(pkg, args.wave_trim), args.reps,
                    f"stereo CELT-FB, {PAGES * PER_PAGE} packets per file, {name}")), flush=True)
                continue
            print(json.dumps(wave_rate.compare_wave_batch(
                torch, pkg, resampled,
                lambda wb: ctx._chk(ctx.lib.opusgpu_set_wave_batch(ctx.h, None if wb is None else wb.rec.ctypes.data), "opusgpu_set_wave_batch"),
                b, 1, 48000 // args.rate, 1 if args.mono else int(rec["out_channels"][0]) if rec is not None else 2, S, norm, args.reps,
                f"stereo CELT-FB, {PAGES * PER_PAGE} packets per file, {name}")), flush=True)
            continue
        print(json.dumps(resample_rate.compare(
            torch, pkg, lambda d, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode(ctx.h, b.h, d, ln, st), "opusgpu_files_decode"), resampled,
            b, args.rate, args.mono, args.reps, name, mix=pkg.downmix_matrix(2, 1 if args.mix == "mono" else 2) if args.mix else None)))
    ctx.close()
    raise SystemExit(0)

if args.resample:
    import ratio_rate
    up, down = pkg.track_ratio(tuple(int(v) for v in args.resample.split("/")))
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == 10
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)
    rec = pkg.mix_matrix(args.mix, 2) if args.mix else None
    rec_p = None if rec is None else rec.ctypes.data

    def at_24000(fmt, d, oo, ol, ln, st):
        if rec is not None:
            return ctx._chk(ctx.lib.opusgpu_files_decode_mixed(ctx.h, b.h, 24000, rec_p, fmt, None, d, oo, ol, ln, st), "opusgpu_files_decode_mixed")
        return ctx._chk(ctx.lib.opusgpu_files_decode_resampled(ctx.h, b.h, 24000, int(args.mono), fmt, None, d, oo, ol, ln, st),
                        "opusgpu_files_decode_resampled")

    def at_24000_kernel(spans, d_in, fmt, d_out):
        if rec is not None:
            return ctx.tracks_resample_mixed_device(spans, d_in, 2, 24000, rec, fmt, d_out)
        return ctx.tracks_resample_device(spans, d_in, 2, 24000, args.mono, fmt, d_out)
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        ctx.set_pipeline(pipe)
        print(json.dumps(ratio_rate.compare(
            torch, pkg,
            lambda d, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_as(ctx.h, b.h, pkg.TRACKS_F32, None, d, ln, st), "opusgpu_files_decode_as"),
            at_24000,
            lambda fmt, d, oo, ol, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_ratio(ctx.h, b.h, up, down, int(args.mono), rec_p, fmt, None, d,
                                                                                       oo, ol, ln, st), "opusgpu_files_decode_ratio"),
            lambda d, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode(ctx.h, b.h, d, ln, st), "opusgpu_files_decode"),
            (lambda spans, d_in, fmt, d_out: ctx.tracks_resample_ratio_device(spans, d_in, 2, up, down, args.mono, rec, fmt, d_out), at_24000_kernel),
            b, up, down, args.mono, args.reps, name, mix=pkg.downmix_matrix(2, 1 if args.mix == "mono" else 2) if args.mix else None)))
    ctx.close()
    raise SystemExit(0)

def set_feature_batch(fb):
    """The feature-batch request `fb` (a FeatureBatch; None: off) on the context `ctx` of the leg that runs."""
    vecs = [None, None] if fb is None else [None if v is None else v.ctypes.data for v in (fb.sub, fb.mul)]
    ctx._chk(ctx.lib.opusgpu_set_feature_batch(ctx.h, None if fb is None else fb.rec.ctypes.data, *vecs, 0 if fb is None else fb.width),
             "opusgpu_set_feature_batch")


if args.fbank:
    import mel_rate
    maker, kw, up, down = mel_rate.FBANK_SETS[args.fbank]
    rec = getattr(pkg, maker)(**kw)
    rate = 48000 // down
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == PAGES * PER_PAGE
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)

    def tracks(fmt, d, oo, ol, ln, st):
        return ctx._chk(ctx.lib.opusgpu_files_decode_resampled(ctx.h, b.h, rate, 1, fmt, None, d, oo, ol, ln, st), "opusgpu_files_decode_resampled")
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        ctx.set_pipeline(pipe)
        note = f"{name}, {PAGES * PER_PAGE} packets per file"
        print(json.dumps(mel_rate.compare_fbank(
            torch, pkg, tracks,
            lambda p, d, fo, fr, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_fbank(ctx.h, b.h, rate, 0, 0, 1, None, p, None, d, fo, fr, ln, st),
                                                  "opusgpu_files_decode_fbank"),
            lambda spans, d_in, r, d_out: ctx.tracks_fbank_device(spans, d_in, r, d_out), b, rec, up, down, args.reps,
            f"{args.fbank}, {note}")), flush=True)
        if args.feature_batch:
            S, norm = mel_rate.feature_batch_arg(args.feature_batch)
            print(json.dumps(mel_rate.compare_feature_batch(
                torch, pkg,
                lambda p, d, fo, fr, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_fbank(ctx.h, b.h, rate, 0, 0, 1, None, p, None, d, fo, fr, ln, st),
                                                      "opusgpu_files_decode_fbank"),
                set_feature_batch, b, rec, pkg.fbank_layout(b.info["track_samples"], up, down, rec),
                pkg.fbank_frames(rec, -(-b.info["track_samples"] * up // down)), S, norm, args.reps, f"{args.fbank}, {note}")), flush=True)
        if rate == 16000:  # k_tracks_melspec's share at the same files
            print(json.dumps(mel_rate.compare_spec(
                torch, pkg, tracks,
                lambda p, d, fo, fr, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_melspec(ctx.h, b.h, rate, 0, 0, 1, None, p, None, d, fo, fr, ln, st),
                                                      "opusgpu_files_decode_melspec"),
                lambda spans, d_in, r, d_out: ctx.tracks_melspec_device(spans, d_in, r, d_out), b, pkg.mel_spec(**mel_rate.SPEC_SETS["kaldi"][0]),
                up, down, args.reps, f"melspec kaldi, {note}")), flush=True)
    ctx.close()
    raise SystemExit(0)

if args.melspec:
    import mel_rate
    rec, up, down = mel_rate.spec_record(pkg, args.melspec, args.melspec_layout, args.melspec_algo)
    rate = 48000 // down if up == 1 else 0
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == PAGES * PER_PAGE
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)

    def tracks(fmt, d, oo, ol, ln, st):
        if rate:
            return ctx._chk(ctx.lib.opusgpu_files_decode_resampled(ctx.h, b.h, rate, 1, fmt, None, d, oo, ol, ln, st), "opusgpu_files_decode_resampled")
        return ctx._chk(ctx.lib.opusgpu_files_decode_ratio(ctx.h, b.h, up, down, 1, None, fmt, None, d, oo, ol, ln, st), "opusgpu_files_decode_ratio")
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        if args.pipe not in ("both", name):
            continue
        ctx.set_pipeline(pipe)
        print(json.dumps(mel_rate.compare_spec(
            torch, pkg, tracks,
            lambda p, d, fo, fr, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_melspec(ctx.h, b.h, rate, 0 if rate else up, 0 if rate else down, 1,
                                                                                       None, p, None, d, fo, fr, ln, st), "opusgpu_files_decode_melspec"),
            lambda spans, d_in, r, d_out: ctx.tracks_melspec_device(spans, d_in, r, d_out), b, rec, up, down, args.reps,
            f"{args.melspec}, {args.melspec_algo or 'set default'}, {args.melspec_layout}, {name}, {PAGES * PER_PAGE} packets per file")), flush=True)
    ctx.close()
    raise SystemExit(0)

if args.stft:
    import mel_rate
    rec, up, down = mel_rate.stft_record(pkg, args.stft, args.stft_layout, args.stft_algo)
    rate = 48000 // down if up == 1 else 0
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == PAGES * PER_PAGE
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)

    def tracks(fmt, d, oo, ol, ln, st):
        if rate:
            return ctx._chk(ctx.lib.opusgpu_files_decode_resampled(ctx.h, b.h, rate, 1, fmt, None, d, oo, ol, ln, st), "opusgpu_files_decode_resampled")
        return ctx._chk(ctx.lib.opusgpu_files_decode_ratio(ctx.h, b.h, up, down, 1, None, fmt, None, d, oo, ol, ln, st), "opusgpu_files_decode_ratio")
    def decode_stft(p, d, fo, fr, ln, st):
        return ctx._chk(ctx.lib.opusgpu_files_decode_stft(ctx.h, b.h, rate, 0 if rate else up, 0 if rate else down, 1, None, p, None, d, fo, fr, ln, st),
                        "opusgpu_files_decode_stft")

    def set_stft_batch(sb):
        """The STFT-batch request `sb` (a StftBatch; None: off) on the context."""
        vecs = [None, None] if sb is None else [None if v is None else v.ctypes.data for v in (sb.sub, sb.mul)]
        ctx._chk(ctx.lib.opusgpu_set_stft_batch(ctx.h, None if sb is None else sb.rec.ctypes.data, *vecs, 0 if sb is None else sb.bins),
                 "opusgpu_set_stft_batch")
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        if args.pipe not in ("both", name):
            continue
        ctx.set_pipeline(pipe)
        note = f"{args.stft} {args.stft_layout}, {name}, {PAGES * PER_PAGE} packets per file"
        if not args.stft_batch_only:
            print(json.dumps(mel_rate.compare_stft(
                torch, pkg, tracks, decode_stft, lambda spans, d_in, r, d_out: ctx.tracks_stft_device(spans, d_in, r, d_out), b, rec, up, down,
                args.reps, note)), flush=True)
        if args.stft_batch:
            S, norm = mel_rate.stft_batch_arg(args.stft_batch)
            print(json.dumps(mel_rate.compare_stft_batch(
                torch, pkg, decode_stft, set_stft_batch, ctx.tracks_stft_batch_device, ctx.tracks_feature_batch_device, b, rec, up, down, S, norm,
                args.reps, note)), flush=True)
    ctx.close()
    raise SystemExit(0)

if args.mel:
    import mel_rate
    b = pkg.FileBatch([r.tobytes() for r in files], channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
    assert (b.info["status"] == 0).all() and b.n_steps == PAGES * PER_PAGE
    ctx = pkg.Context(0)
    ctx.streams_alloc(n, 2)
    for name, pipe in (("in_order", 0), ("pipelined", 1)):
        ctx.set_pipeline(pipe)
        print(json.dumps(mel_rate.compare(
            torch, pkg,
            lambda fmt, d, oo, ol, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_resampled(ctx.h, b.h, 16000, 1, fmt, None, d, oo, ol, ln, st),
                                                    "opusgpu_files_decode_resampled"),
            lambda p, d, fo, fr, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_mel(ctx.h, b.h, 1, None, p, None, d, fo, fr, ln, st),
                                                  "opusgpu_files_decode_mel"),
            lambda spans, d_in, rec, d_out: ctx.tracks_mel_device(spans, d_in, rec, None, d_out), b, args.n_mels, args.reps, name)))
        if args.feature_batch:
            S, norm = mel_rate.feature_batch_arg(args.feature_batch)
            print(json.dumps(mel_rate.compare_feature_batch(
                torch, pkg,
                lambda p, d, fo, fr, ln, st: ctx._chk(ctx.lib.opusgpu_files_decode_mel(ctx.h, b.h, 1, None, p, None, d, fo, fr, ln, st),
                                                      "opusgpu_files_decode_mel"),
                set_feature_batch, b, pkg.mel_params(args.n_mels, "bands"), pkg.mel_layout(b.info["track_samples"], args.n_mels, "bands"),
                -(-b.info["track_samples"] // 3) // 160, S, norm, args.reps, f"{name}, {PAGES * PER_PAGE} packets per file")), flush=True)
    ctx.close()
    raise SystemExit(0)

# ---- planner and page demux rates ----------------------------------------------------------------------
blobs = [r.tobytes() for r in files]
t0 = time.perf_counter()
b = pkg.FileBatch(blobs, channels=2, flags=pkg.PAGES_GROUP_BY_MODE, threads=args.threads)
plan_s = time.perf_counter() - t0
assert (b.info["status"] == 0).all() and b.n_steps == 10
hdr = files.shape[1] - (27 + 10 + 10 * 161)  # the audio page is the file's tail
pages = np.ascontiguousarray(files[:, hdr:])
t0 = time.perf_counter()
pb = pkg.PageBatch(pages.reshape(-1), np.arange(n, dtype=np.int64) * pages.shape[1], np.full(n, pages.shape[1], np.int32), np.arange(n),
                   threads=args.threads)
demux_s = time.perf_counter() - t0
pb.close()

# ---- device-resident steps -------------------------------------------------------------------------------
ctx = pkg.Context(0)
ctx.streams_alloc(n, 2)
steps = [b.step(k) for k in range(10)]
descs = np.concatenate([s[0] for s in steps])
segs = np.concatenate([s[2] for s in steps])
d_descs, d_segs, d_arena = ctx.dev_alloc(descs.nbytes), ctx.dev_alloc(segs.nbytes), ctx.dev_alloc(b.arena.nbytes)
d_pcm, d_res = ctx.dev_alloc(n * 960 * 4), ctx.dev_alloc(4 * n)
d_tracks, d_copy = ctx.dev_alloc(int(b.track_samples) * 4), ctx.dev_alloc(int(b.track_samples) * 4)
state = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
state["first_bad"] = 2**31 - 1
d_state = ctx.dev_alloc(state.nbytes)
for d, a in ((d_descs, descs), (d_segs, segs), (d_arena, b.arena), (d_state, state)):
    ctx.h2d(d, a)
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipDeviceSynchronize.argtypes = []


def batch(assemble):
    at = 0
    for k in range(10):
        m = len(steps[k][0])
        ctx.decode_step_device(m, C.c_void_p(d_descs.value + 16 * at), d_arena, d_pcm, d_res, modes=steps[k][3])
        if assemble:
            ctx.tracks_assemble_device(m, C.c_void_p(d_segs.value + 32 * at), d_pcm, 960, d_res, d_tracks, d_state)
        at += m


def timed(fn, sync):
    fn()
    sync()
    out = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def copy():
    assert hip.hipMemcpyAsync(d_copy, d_tracks, MOVED // 2, 3, None) == 0  # hipMemcpyDeviceToDevice: reads and writes MOVED / 2 each


out = {"files": n, "bytes_moved_per_batch": MOVED, "plan_files_per_s": round(n / plan_s), "plan_threads": args.threads,
       "demux_pages_per_s": round(n / demux_s)}
for name, pipe in (("in_order", 0), ("pipelined", 1)):
    ctx.set_pipeline(pipe)
    a, w = [], []
    for _ in range(3):  # (a) and (b) interleaved, three rounds each: drift shows up as spread, not as a difference
        a += timed(lambda: batch(False), ctx.synchronize)
        w += timed(lambda: batch(True), ctx.synchronize)
    out[name] = {"a_steps_ms": round(float(np.mean(a)), 3), "a_min_max_ms": [round(min(a), 3), round(max(a), 3)], "a_std_ms": round(float(np.std(a)), 3),
                 "b_steps_assembly_ms": round(float(np.mean(w)), 3), "b_min_max_ms": [round(min(w), 3), round(max(w), 3)],
                 "b_minus_a_ms": round(float(np.mean(w) - np.mean(a)), 3)}
ctx.set_pipeline(0)
c = timed(copy, hip.hipDeviceSynchronize)
out["d_memcpy_d2d_ms"] = round(float(np.mean(c)), 3)
out["d_memcpy_tb_per_s"] = round(MOVED / (float(np.mean(c)) / 1e3) / 1e12, 2)
got = np.zeros(n, dtype=pkg.TRACK_STATE_DTYPE)
ctx.d2h(got, d_state)
assert (got["first_bad"] == 2**31 - 1).all()
print(json.dumps(out))
ctx.close()
