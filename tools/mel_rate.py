"""What tools/files_rate.py and tools/ms_files_rate.py run for --mel: the whole decode call of a planned batch into torch tensors,
variants interleaved per repeat (include/opusgpu.h TRACK FEATURES):
(a) float32 mono tracks at 16 kHz, the call as it was (decode_files(rate=16000, mono=True, format="f32", out=...)); (b) (a)
followed by the front end a consumer runs on them in torch -- the ragged tracks gathered into a zero-padded [files, longest]
batch (the gather index is made once, outside the timing), torch.stft(400, 160, periodic Hann, center=True) without its last
frame, |.|^2, the filterbank matmul, log10(clamp(1e-10)); (c) the fused call, log-mel features bands-major.  Then (m):
k_tracks_mel alone (opusgpu_tracks_mel_device: its uploads, the launch and the wait) over the int16 tracks of the same batch, and its
share of (c).  Means, medians, min / max; no ratio is asked of (c) against (b): both are printed.
One track of (c) is held against (b) away from the track's end, where (b) pads with zeros in place of reflecting.
compare_spec is the same for --melspec (include/opusgpu.h TRACK SPECTROGRAMS) with a mel_spec record in place of Whisper's constants:
(a) float32 mono tracks at the record's rate, (b) (a) + torch.stft(n_fft, hop, win_length, periodic Hann, center=True), |.| or |.|^2,
the filterbank matmul, the floor and the log, (c) the fused call, (m) opusgpu_tracks_melspec_device alone.
compare_fbank is the same for --fbank (include/opusgpu.h TRACK KALDI FEATURES) with a kaldi_fbank / kaldi_mfcc record (snip_edges on):
(a) float32 mono tracks at the record's rate, (b) (a) + the torch restatement -- unfold, the frame's mean, the pre-emphasis, the
window, torch.fft.rfft at n_fft, |.| or |.|^2 without the Nyquist bin, the filterbank matmul, the floor, the log and for MFCC the
DCT matmul --, (c) the fused call, (m) opusgpu_tracks_fbank_device alone.
compare_stft is the same for --stft (include/opusgpu.h TRACK STFT) with a stft_spec record: (a) float32 mono tracks at the record's
rate, (b) (a) + torch.stft + abs, abs ** 2 or nothing + the floor and the log, (c) the fused call, (m) opusgpu_tracks_stft_device
alone, with the bytes it writes per second.
compare_feature_batch is --feature-batch S[:NORM] (include/opusgpu.h FEATURE BATCHES) behind --mel or --fbank: (p) the packed feature
call, (b) (p) + the gather into a padded tensor and the normalisation in torch, (c) the call with the request on.
torch must be imported before the library is loaded: they then share one HIP runtime."""
import time

import numpy as np


def compare(torch, pkg, decode_16k, decode_mel, mel_alone, batch, n_mels, reps, note=""):
    """decode_16k(fmt, d_out, out_offsets, out_lengths, lengths, status) runs the library's mono 16 kHz call for the batch,
    decode_mel(params, d_out, feat_offsets, frames, lengths, status) the fused one, mel_alone(spans, d_in, params, d_out) the
    kernel's; each checks its code.  -> a dict for the JSON line."""
    n = batch.n_files
    planned = batch.info["track_samples"]
    offs, total16 = pkg.resample_layout(planned, 16000)
    feat_offs, planes, total_feat = pkg.mel_layout(planned, n_mels, "bands")
    rec = pkg.mel_params(n_mels, "bands")
    f32 = torch.empty(max(total16, 1), dtype=torch.float32, device="cuda:0")
    s16 = torch.empty(max(total16, 1) + 64, dtype=torch.int16, device="cuda:0")
    feat = torch.empty(max(total_feat, 1), dtype=torch.float32, device="cuda:0")
    lengths, out_offsets, out_lengths, fo, frames = (np.zeros(n, dtype=np.int64) for _ in range(5))
    status = np.zeros((n, 2), dtype=np.int32)
    len16 = -(-planned // 3)
    longest = int(len16.max(initial=1))
    idx = offs[:, None] + np.arange(longest)[None, :]
    valid = np.arange(longest)[None, :] < len16[:, None]
    gather = torch.tensor(np.where(valid, idx, 0), device="cuda:0")
    mask = torch.tensor(valid, device="cuda:0")
    window = torch.hann_window(400, periodic=True, device="cuda:0")
    bank_t = torch.tensor(pkg.mel_filterbank(n_mels).T.copy(), device="cuda:0")  # [201, n_mels]

    def a():
        decode_16k(pkg.TRACKS_F32, f32.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def b():
        a()
        x = torch.where(mask, f32[gather], torch.zeros((), device="cuda:0"))
        spec = torch.stft(x, 400, 160, window=window, center=True, return_complex=True)[..., :-1]  # [files, 201, frames]
        out = torch.log10(torch.clamp((spec.abs() ** 2).transpose(1, 2) @ bank_t, min=1e-10))     # [files, frames, n_mels]
        torch.cuda.synchronize()
        return out

    def c():
        decode_mel(rec.ctypes.data, feat.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    decode_16k(pkg.TRACKS_S16, s16.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)
    spans = np.zeros(n, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_offset"], spans["in_samples"], spans["out_offset"], spans["plane"], spans["scale"] = offs, out_lengths, feat_offs, planes, 2.0 ** -15

    def m():
        mel_alone(spans, s16.data_ptr(), rec, feat.data_ptr())

    times = {"a": [], "b": [], "c": [], "m": []}
    for fn in (a, b, c, m):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a), ("b", b), ("c", c), ("m", m)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    assert (status[:, 0] == 0).all() and (lengths == planned).all() and (fo == feat_offs).all() and (frames == len16 // 160).all()
    # one track of (c) against (b): the same features up to float rounding, but for the last two frames, where (b) sees padding
    c()
    want = b()
    worst = None
    fits = [j for j in range(n // 2, n) if frames[j] > 4]
    if fits:
        i = fits[0]
        F, o, p = int(frames[i]), int(feat_offs[i]), int(planes[i])
        got = feat[o:o + n_mels * p].view(n_mels, p)[:, :F - 2].t()
        worst = float((got - want[i, :F - 2]).abs().max())
        assert worst < 1e-2, worst
    out = {"mel": n_mels, "files": n, "frames": int(frames.sum()), "reps": reps, "note": note, "scratch_s16_16k_bytes": int(total16) * 2,
           "out_bytes": int(total_feat) * 4, "padded_batch_floats_of_b": n * longest,
           "worst_abs_log10_vs_torch": worst if fits else "not checked: no track of more than 4 frames"}
    for k, label in (("a", "a_f32_16k_mono"), ("b", "b_f32_then_torch_stft_mel"), ("c", "c_fused_logmel"), ("m", "m_k_tracks_mel_call")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["mel_share_of_c"] = round(float(np.mean(times["m"]) / np.mean(times["c"])), 3)
    out["c_le_b"] = bool(np.mean(times["c"]) <= np.mean(times["b"]))
    return out


def compare_spec(torch, pkg, decode_tracks, decode_spec, spec_alone, batch, rec, up, down, reps, note=""):
    """decode_tracks(fmt, d_out, out_offsets, out_lengths, lengths, status) runs the library's mono call at up / down of 48 kHz for the
    batch, decode_spec(params, d_out, feat_offsets, frames, lengths, status) the fused one, spec_alone(spans, d_in, rec, d_out) the
    kernel's; each checks its code.  -> a dict for the JSON line."""
    n = batch.n_files
    planned = batch.info["track_samples"]
    offs, total = pkg.resample_ratio_layout(planned, up, down) if up != 1 or down not in (1, 2, 3, 4, 6) else pkg.resample_layout(planned, 48000 // down)
    feat_offs, planes, total_feat = pkg.spec_layout(planned, up, down, rec)
    n_fft, hop, n_mels = int(rec["n_fft"][0]), int(rec["hop"][0]), int(rec["n_mels"][0])
    win, power, log, floor = int(rec["win_length"][0]) or n_fft, int(rec["power"][0]), int(rec["log"][0]), float(rec["floor"][0])
    whisper = int(rec["frames"][0]) == 1
    f32 = torch.empty(max(total, 1), dtype=torch.float32, device="cuda:0")
    s16 = torch.empty(max(total, 1) + 64, dtype=torch.int16, device="cuda:0")
    feat = torch.empty(max(total_feat, 1), dtype=torch.float32, device="cuda:0")
    lengths, out_offsets, out_lengths, fo, frames = (np.zeros(n, dtype=np.int64) for _ in range(5))
    status = np.zeros((n, 2), dtype=np.int32)
    len_r = -(-planned * up // down)
    longest = int(len_r.max(initial=1))
    idx = offs[:, None] + np.arange(longest)[None, :]
    valid = np.arange(longest)[None, :] < len_r[:, None]
    gather = torch.tensor(np.where(valid, idx, 0), device="cuda:0")
    mask = torch.tensor(valid, device="cuda:0")
    window = torch.hann_window(win, periodic=True, device="cuda:0")
    bank_t = torch.tensor(pkg.spec_filterbank(rec).T.copy(), device="cuda:0")  # [bins, n_mels]

    def a():
        decode_tracks(pkg.TRACKS_F32, f32.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def b():
        a()
        x = torch.where(mask, f32[gather], torch.zeros((), device="cuda:0"))
        spec = torch.stft(x, n_fft, hop, win_length=win, window=window, center=True, return_complex=True)  # [files, bins, frames]
        mag = spec.abs()
        out = torch.clamp((mag if power == 1 else mag ** 2).transpose(1, 2) @ bank_t, min=floor)            # [files, frames, n_mels]
        out = torch.log10(out) if log == 1 else torch.log(out) if log == 2 else out
        torch.cuda.synchronize()
        return out

    def c():
        decode_spec(rec.ctypes.data, feat.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    decode_tracks(pkg.TRACKS_S16, s16.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)
    spans = np.zeros(n, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_offset"], spans["in_samples"], spans["out_offset"], spans["plane"], spans["scale"] = offs, out_lengths, feat_offs, planes, 2.0 ** -15

    def m():
        spec_alone(spans, s16.data_ptr(), rec, feat.data_ptr())

    times = {"a": [], "b": [], "c": [], "m": []}
    for fn in (a, b, c, m):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a), ("b", b), ("c", c), ("m", m)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    assert (status[:, 0] == 0).all() and (lengths == planned).all() and (fo == feat_offs).all() and (frames == pkg.spec_frames(rec, len_r)).all()
    # one track of (c) against (b) away from the track's ends, where (b) pads the batch with zeros in place of reflecting
    c()
    want = b()
    edge = n_fft // 2 // hop + 2
    worst = None
    fits = [j for j in range(n // 2, n) if frames[j] > 2 * edge + 2]
    if fits:
        i = fits[0]
        F, o, p = int(frames[i]), int(feat_offs[i]), int(planes[i])
        if int(rec["layout"][0]) == pkg.MEL_FRAMES_MAJOR:
            got = feat[o:o + n_mels * F].view(F, n_mels)[edge:F - edge]
        else:
            got = feat[o:o + n_mels * p].view(n_mels, p)[:, edge:F - edge].t()
        ref = want[i, edge:F - edge]
        d = (got - ref).abs()
        worst = float((d if log else d / ref.abs().clamp(min=1e-30)).max())
        assert worst < 1e-2, worst
    out = {"melspec": [int(rec[k][0]) for k in ("sample_rate", "n_fft", "win_length", "hop", "n_mels")], "files": n, "frames": int(frames.sum()),
           "reps": reps, "note": note, "scratch_s16_bytes": int(total) * 2, "out_bytes": int(total_feat) * 4, "padded_batch_floats_of_b": n * longest,
           "worst_error_vs_torch": worst if fits else "not checked: no track long enough"}
    for k, label in (("a", "a_f32_mono"), ("b", "b_f32_then_torch_stft_mel"), ("c", "c_fused_melspec"), ("m", "m_k_tracks_melspec_call")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["melspec_share_of_c"] = round(float(np.mean(times["m"]) / np.mean(times["c"])), 3)
    out["c_le_b"] = bool(np.mean(times["c"]) <= np.mean(times["b"]))
    return out


def compare_stft(torch, pkg, decode_tracks, decode_stft, stft_alone, batch, rec, up, down, reps, note=""):
    """compare_spec's arguments with a stft_spec record (include/opusgpu.h TRACK STFT): (a) float32 mono tracks at the record's rate,
    (b) (a) + the gather into a padded batch + torch.stft(n_fft, hop, win_length, periodic Hann, center=True) + abs, abs ** 2 or
    nothing + the floor and the log, (c) the fused call, (m) opusgpu_tracks_stft_device alone, with the bytes per second it writes.
    -> a dict for the JSON line."""
    n = batch.n_files
    planned = batch.info["track_samples"]
    offs, total = pkg.resample_ratio_layout(planned, up, down) if up != 1 or down not in (1, 2, 3, 4, 6) else pkg.resample_layout(planned, 48000 // down)
    feat_offs, planes, total_feat = pkg.stft_layout(planned, up, down, rec)
    n_fft, hop, bins, width = int(rec["n_fft"][0]), int(rec["hop"][0]), int(rec["n_fft"][0]) // 2 + 1, pkg.stft_width(rec)
    win, power, log, floor = int(rec["win_length"][0]) or n_fft, int(rec["power"][0]), int(rec["log"][0]), float(rec["floor"][0])
    whisper, frames_major = int(rec["frames"][0]) == 1, int(rec["layout"][0]) == pkg.MEL_FRAMES_MAJOR
    f32 = torch.empty(max(total, 1), dtype=torch.float32, device="cuda:0")
    s16 = torch.empty(max(total, 1) + 64, dtype=torch.int16, device="cuda:0")
    feat = torch.empty(max(total_feat, 1), dtype=torch.float32, device="cuda:0")
    lengths, out_offsets, out_lengths, fo, frames = (np.zeros(n, dtype=np.int64) for _ in range(5))
    status = np.zeros((n, 2), dtype=np.int32)
    len_r = -(-planned * up // down)
    longest = max(int(len_r.max(initial=1)), n_fft // 2 + 1)  # (torch.stft's reflection needs that much)
    idx = offs[:, None] + np.arange(longest)[None, :]
    valid = np.arange(longest)[None, :] < len_r[:, None]
    gather = torch.tensor(np.where(valid, idx, 0), device="cuda:0")
    mask = torch.tensor(valid, device="cuda:0")
    window = torch.hann_window(win, periodic=True, device="cuda:0")

    def a():
        decode_tracks(pkg.TRACKS_F32, f32.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def b():
        a()
        x = torch.where(mask, f32[gather], torch.zeros((), device="cuda:0"))
        out = torch.stft(x, n_fft, hop, win_length=win, window=window, center=True, return_complex=True)  # [files, bins, frames]
        if whisper:
            out = out[..., :-1]
        if power:
            out = torch.clamp(out.abs() if power == 1 else out.abs() ** 2, min=floor)
            out = torch.log10(out) if log == 1 else torch.log(out) if log == 2 else out
        if frames_major:
            out = out.transpose(1, 2).contiguous()
        torch.cuda.synchronize()
        return out

    def c():
        decode_stft(rec.ctypes.data, feat.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    decode_tracks(pkg.TRACKS_S16, s16.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)
    spans = np.zeros(n, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_offset"], spans["in_samples"], spans["out_offset"], spans["plane"], spans["scale"] = offs, out_lengths, feat_offs, planes, 2.0 ** -15

    def m():
        stft_alone(spans, s16.data_ptr(), rec, feat.data_ptr())

    times = {"a": [], "b": [], "c": [], "m": []}
    for fn in (a, b, c, m):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a), ("b", b), ("c", c), ("m", m)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    assert (status[:, 0] == 0).all() and (lengths == planned).all() and (fo == feat_offs).all() and (frames == pkg.stft_frames(rec, len_r)).all()
    # one track of (c) against (b) away from the track's ends, where (b) pads the batch with zeros in place of reflecting
    c()
    want = b()
    edge = n_fft // 2 // hop + 2
    worst = None
    fits = [j for j in range(n // 2, n) if frames[j] > 2 * edge + 2]
    if fits:
        i = fits[0]
        F, o, p = int(frames[i]), int(feat_offs[i]), int(planes[i])
        got = feat[o:o + width * F].view(F, width) if frames_major else feat[o:o + width * p].view(bins, p * (width // bins))
        if power == 0:
            got = torch.view_as_complex(got.reshape(F, bins, 2) if frames_major else got.reshape(bins, p, 2))
        got = got[edge:F - edge] if frames_major else got[:, edge:F - edge]
        ref = want[i, edge:F - edge] if frames_major else want[i, :, edge:F - edge]
        if log:  # back to the linear value: a cell near the floor is all rounding in the log, in both
            got, ref = (10.0 ** got, 10.0 ** ref) if log == 1 else (got.exp(), ref.exp())
        top = ref.abs().amax(dim=1 if frames_major else 0, keepdim=True).clamp(min=1e-30)  # the frame's largest
        worst = float(((got - ref).abs() / top).max())  # relative to the frame's largest cell
        assert worst < 1e-4, worst
    out = {"stft": [int(rec[k][0]) for k in ("sample_rate", "n_fft", "win_length", "hop", "power", "log", "layout")],
           "algo": "fft" if int(rec["reserved"][0][1]) == pkg.STFT_ALGO_FFT else "dense", "files": n,
           "frames": int(frames.sum()), "reps": reps, "note": note, "tile": pkg.stft_tile(rec), "scratch_s16_bytes": int(total) * 2,
           "out_bytes": int(total_feat) * 4, "padded_batch_floats_of_b": n * longest,
           "worst_error_vs_torch": worst if fits else "not checked: no track long enough"}
    for k, label in (("a", "a_f32_mono"), ("b", "b_f32_then_torch_stft"), ("c", "c_fused_stft"), ("m", "m_k_tracks_stft_call")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["stft_share_of_c"] = round(float(np.mean(times["m"]) / np.mean(times["c"])), 3)
    out["m_written_gb_per_s"] = round(float(frames.sum()) * width * 4 / (np.mean(times["m"]) * 1e-3) / 1e9, 2)
    out["b_over_c"] = round(float(np.mean(times["b"]) / np.mean(times["c"])), 3)
    out["c_le_b"] = bool(np.mean(times["c"]) <= np.mean(times["b"]))
    return out


def compare_fbank(torch, pkg, decode_tracks, decode_fbank, fbank_alone, batch, rec, up, down, reps, note=""):
    """compare_spec's arguments with a kaldi_fbank / kaldi_mfcc record whose snip_edges is on.  -> a dict for the JSON line."""
    n = batch.n_files
    planned = batch.info["track_samples"]
    offs, total = pkg.resample_ratio_layout(planned, up, down) if up != 1 or down not in (1, 2, 3, 4, 6) else pkg.resample_layout(planned, 48000 // down)
    feat_offs, planes, total_feat = pkg.fbank_layout(planned, up, down, rec)
    L, H, width, n_mels = int(rec["frame_length"][0]), int(rec["frame_shift"][0]), pkg.fbank_width(rec), int(rec["n_mels"][0])
    bank = pkg.fbank_filterbank(rec)
    N = 2 * bank.shape[1]
    power, log, floor, pre = int(rec["power"][0]), int(rec["log"][0]), float(rec["floor"][0]), float(rec["preemphasis"][0])
    dc, n_ceps = int(rec["remove_dc"][0]), int(rec["n_ceps"][0])
    assert int(rec["snip_edges"][0]) == 1 and int(rec["layout"][0]) == pkg.MEL_FRAMES_MAJOR
    f32 = torch.empty(max(total, 1), dtype=torch.float32, device="cuda:0")
    s16 = torch.empty(max(total, 1) + 64, dtype=torch.int16, device="cuda:0")
    feat = torch.empty(max(total_feat, 1), dtype=torch.float32, device="cuda:0")
    lengths, out_offsets, out_lengths, fo, frames = (np.zeros(n, dtype=np.int64) for _ in range(5))
    status = np.zeros((n, 2), dtype=np.int32)
    len_r = -(-planned * up // down)
    longest = max(int(len_r.max(initial=1)), L)
    idx = offs[:, None] + np.arange(longest)[None, :]
    valid = np.arange(longest)[None, :] < len_r[:, None]
    gather = torch.tensor(np.where(valid, idx, 0), device="cuda:0")
    mask = torch.tensor(valid, device="cuda:0")
    window = torch.tensor(pkg.fbank_window(rec), device="cuda:0")
    bank_t = torch.tensor(bank.T.copy(), device="cuda:0")  # [N / 2, n_mels]
    dct_t = torch.tensor(pkg.fbank_dct(rec).T.copy(), device="cuda:0") if n_ceps else None  # [n_mels, n_ceps]

    def a():
        decode_tracks(pkg.TRACKS_F32, f32.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def b():
        a()
        x = torch.where(mask, f32[gather], torch.zeros((), device="cuda:0"))
        fr = x.unfold(1, L, H)                                                                   # [files, frames, L]
        if dc:
            fr = fr - fr.mean(dim=2, keepdim=True)
        fr = (fr - pre * torch.cat([fr[..., :1], fr[..., :-1]], dim=2)) * window
        mag = torch.fft.rfft(fr, n=N)[..., :N // 2].abs()
        out = torch.clamp((mag if power == 1 else mag ** 2) @ bank_t, min=floor)                 # [files, frames, n_mels]
        out = torch.log(out) if log else out
        out = out @ dct_t if n_ceps else out
        torch.cuda.synchronize()
        return out

    def c():
        decode_fbank(rec.ctypes.data, feat.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    decode_tracks(pkg.TRACKS_S16, s16.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)
    spans = np.zeros(n, dtype=pkg.MEL_SPAN_DTYPE)
    spans["in_offset"], spans["in_samples"], spans["out_offset"], spans["plane"], spans["scale"] = offs, out_lengths, feat_offs, planes, 2.0 ** -15

    def m():
        fbank_alone(spans, s16.data_ptr(), rec, feat.data_ptr())

    times = {"a": [], "b": [], "c": [], "m": []}
    for fn in (a, b, c, m):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a), ("b", b), ("c", c), ("m", m)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    assert (status[:, 0] == 0).all() and (lengths == planned).all() and (fo == feat_offs).all() and (frames == pkg.fbank_frames(rec, len_r)).all()
    # one track of (c) against (b): every frame lies inside the track, so all of them compare
    c()
    want = b()
    worst = None
    fits = [j for j in range(n // 2, n) if frames[j] > 2]
    if fits:
        i = fits[0]
        F, o = int(frames[i]), int(feat_offs[i])
        got, ref = feat[o:o + F * width].view(F, width), want[i, :F]
        d = (got - ref).abs()
        worst = float((d if log else d / ref.abs().clamp(min=1e-30)).max())
        assert worst < 1e-2, worst
    out = {"fbank": [int(rec[k][0]) for k in ("sample_rate", "frame_length", "frame_shift", "n_mels", "n_ceps")] + [N], "files": n,
           "frames": int(frames.sum()), "reps": reps, "note": note, "scratch_s16_bytes": int(total) * 2, "out_bytes": int(total_feat) * 4,
           "padded_batch_floats_of_b": n * longest, "worst_error_vs_torch": worst if fits else "not checked: no track long enough"}
    for k, label in (("a", "a_f32_mono"), ("b", "b_f32_then_torch_unfold_rfft_mel"), ("c", "c_fused_fbank"), ("m", "m_k_tracks_fbank_call")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["fbank_share_of_c"] = round(float(np.mean(times["m"]) / np.mean(times["c"])), 3)
    out["c_le_b"] = bool(np.mean(times["c"]) <= np.mean(times["b"]))
    return out


def feature_batch_arg(text):
    """--feature-batch S[:NORM] -> (S, NORM): NORM one of none, whisper, cmn, cmvn (default none)."""
    s, _, norm = text.partition(":")
    norm = norm or "none"
    if norm not in ("none", "whisper", "cmn", "cmvn") or int(s) < 1:
        raise ValueError(f"--feature-batch takes S[:none|whisper|cmn|cmvn] with S >= 1, not {text!r}")
    return int(s), norm


def compare_feature_batch(torch, pkg, decode_feat, set_request, batch, rec, layout, planned_frames, stride, norm, reps, note=""):
    """--feature-batch S[:NORM] (include/opusgpu.h FEATURE BATCHES): decode_feat(params, d_out, feat_offsets, frames, lengths, status)
    runs a fused feature call of the batch for the record `rec`, whose packed grid is layout = (feat_offsets, planes, total floats)
    and whose tracks have planned_frames frames; set_request(FeatureBatch or None) puts a request on the decoder or takes it off.
    (p) the packed feature call as it was; (b) (p) followed by the torch form a user writes today -- the ragged features gathered
    into a padded [files, S, W] or [files, W, S] tensor (the gather index is made once, outside the timing), then amax / clamp for
    whisper or the masked mean / variance per bin for cmn / cmvn; (c) the same call with the request on, which writes that tensor.
    Variants interleaved per repeat; both are printed, no ratio is asked.  -> a dict for the JSON line."""
    n = batch.n_files
    feat_offs, planes, total_feat = layout
    W = pkg.fbank_width(rec) if rec.dtype == pkg.FBANK_PARAMS_DTYPE else int(rec["n_mels"][0])
    frames_major = int(rec["layout"][0]) == pkg.MEL_FRAMES_MAJOR
    fb = pkg.feature_batch_request(planned_frames, W, stride, None if norm == "none" else norm)
    S = fb.stride
    pad_value = float(fb.rec["pad_value"][0])
    packed = torch.empty(max(total_feat, 1), dtype=torch.float32, device="cuda:0")
    dense = torch.empty(max(n * S * W, 1), dtype=torch.float32, device="cuda:0")
    lengths, fo, frames = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    f, j = np.arange(S)[None, :, None], np.arange(W)[None, None, :]
    F = np.asarray(planned_frames, dtype=np.int64)[:, None, None]
    at = feat_offs[:, None, None] + (f * W + j if frames_major else j * planes[:, None, None] + f)
    valid = np.broadcast_to(f < F, at.shape)
    if not frames_major:
        at, valid = at.transpose(0, 2, 1), valid.transpose(0, 2, 1)
    gather = torch.tensor(np.where(valid, at, 0), device="cuda:0")
    mask = torch.tensor(np.ascontiguousarray(valid), device="cuda:0")
    count = torch.tensor(np.maximum(F, 1).astype(np.float32), device="cuda:0")
    fdim = 1 if frames_major else 2
    pad = torch.full((), pad_value, device="cuda:0")
    zero = torch.zeros((), device="cuda:0")

    def p():
        decode_feat(rec.ctypes.data, packed.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def b():
        p()
        x = torch.where(mask, packed[gather], pad)
        if norm == "whisper":
            m = torch.where(mask, x, torch.full((), -float("inf"), device="cuda:0")).amax(dim=(1, 2), keepdim=True)
            x = (torch.maximum(x, m - 8.0) + 4.0) / 4.0
        elif norm in ("cmn", "cmvn"):
            mean = torch.where(mask, x, zero).sum(dim=fdim, keepdim=True) / count
            d = x - mean
            if norm == "cmvn":
                var = torch.where(mask, d * d, zero).sum(dim=fdim, keepdim=True) / count
                d = d / torch.sqrt(torch.clamp(var, min=float(fb.rec["var_floor"][0])))
            x = torch.where(mask, d, pad)
        torch.cuda.synchronize()
        return x

    def c():
        set_request(fb)
        try:
            decode_feat(rec.ctypes.data, dense.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)
        finally:
            set_request(None)

    times = {"p": [], "b": [], "c": []}
    for fn in (p, b, c):
        fn()
    for _ in range(reps):
        for name, fn in (("p", p), ("b", b), ("c", c)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    c()
    assert (status[:, 0] == 0).all() and (frames == np.asarray(planned_frames)).all() and (fo == np.arange(n) * S * W).all()
    want = b()
    worst = float((dense[:n * S * W].view(want.shape) - want).abs().max())
    assert worst < 1e-3, worst
    out = {"feature_batch": [S, norm], "width": W, "layout": "frames" if frames_major else "bands", "files": n, "frames": int(frames.sum()),
           "reps": reps, "note": note, "packed_bytes": int(total_feat) * 4, "dense_bytes": n * S * W * 4, "worst_abs_vs_torch": worst}
    for k, label in (("p", "p_packed_feature_call"), ("b", "b_packed_then_torch_pad_and_norm"), ("c", "c_fused_feature_batch")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["c_le_b"] = bool(np.mean(times["c"]) <= np.mean(times["b"]))
    return out


def stft_batch_arg(text):
    """--stft-batch S[:NORM] -> (S, NORM): NORM one of none, whisper, refmax, cmn, cmvn (default none); S 0 is the longest planned track."""
    s, _, norm = text.partition(":")
    norm = norm or "none"
    if norm not in ("none", "whisper", "refmax", "cmn", "cmvn") or int(s) < 0:
        raise ValueError(f"--stft-batch takes S[:none|whisper|refmax|cmn|cmvn] with S >= 0, not {text!r}")
    return int(s), norm


class _PeakMemory:
    """The most device memory in use while the block runs, over what was in use before it: a thread polls the device's free bytes (the
    library allocates with hipMalloc, which torch's own counters do not see; ctypes calls release the interpreter)."""

    def __init__(self, torch):
        import threading
        self.torch, self.low, self.stop = torch, None, threading.Event()
        self.thread = threading.Thread(target=self.poll)

    def poll(self):
        while not self.stop.is_set():
            self.low = min(self.low, self.torch.cuda.mem_get_info()[0])
            time.sleep(0.0005)

    def __enter__(self):
        self.before = self.low = self.torch.cuda.mem_get_info()[0]
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.bytes = self.before - self.low


def compare_stft_batch(torch, pkg, decode_stft, set_request, stage_alone, feat_stage_alone, batch, rec, up, down, stride, norm, reps, note=""):
    """--stft-batch S[:NORM] (include/opusgpu.h STFT BATCHES): decode_stft(params, d_out, feat_offsets, frames, lengths, status) runs the
    whole-file STFT call of the batch; set_request(StftBatch or None) puts a request on the decoder or takes it off;
    stage_alone(spans, layout, StftBatch, d_grid, d_out) is opusgpu_tracks_stft_batch_device and feat_stage_alone(spans, width, layout,
    FeatureBatch, d_grid, d_out) opusgpu_tracks_feature_batch_device.  Legs, interleaved per repeat:
    (p) the packed call as it was; (b) (p) followed by the torch form a user writes today -- the ragged cells gathered into a padded
    [files, bins, S] or [files, S, bins] tensor (the gather index is made once, on the device, outside the timing), then the norm;
    (c) the dense call with the request (S, NORM) as asked; (g) the dense call without a norm at a stride of S rounded up to 64, plus
    one: the general path; (d) the same at the multiple of 64: the direct path; (s) the stage alone with (S, NORM) over (p)'s grid and
    (f) k_feat_batch alone (norm NONE, width 128) over a grid of zeros with as many floats.  Then one more run of (g) and (d) each
    with the device's free memory polled.  -> a dict for the JSON line."""
    n = batch.n_files
    planned = np.asarray(batch.info["track_samples"], dtype=np.int64)
    feat_offs, planes, total = pkg.stft_layout(planned, up, down, rec)
    bins, c = int(rec["n_fft"][0]) // 2 + 1, 2 if int(rec["power"][0]) == pkg.STFT_COMPLEX else 1
    frames_major = int(rec["layout"][0]) == pkg.MEL_FRAMES_MAJOR
    layout = "frames" if frames_major else "bands"
    F = pkg.stft_frames(rec, -(-planned * up // down))
    sb = pkg.stft_batch_request(F, bins, c, stride or None, None if norm == "none" else norm)
    S = sb.stride
    S64 = (S + 63) // 64 * 64
    sb_direct, sb_general = pkg.stft_batch_request(F, bins, c, S64), pkg.stft_batch_request(F, bins, c, S64 + 1)
    pad_value, normalized = float(sb.rec["pad_value"][0]), int(sb.rec["pad_mode"][0]) == pkg.FEAT_PAD_NORMALIZED
    packed = torch.empty(max(total, 1), dtype=torch.float32, device="cuda:0")
    dense = torch.empty(max(n * (S64 + 1) * bins * c, 1), dtype=torch.float32, device="cuda:0")
    lengths, fo, frames = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    dev = dict(device="cuda:0")
    f, k = torch.arange(S, **dev)[None, :, None], torch.arange(bins, **dev)[None, None, :]
    Fd = torch.tensor(F, **dev)[:, None, None]
    at = torch.tensor(feat_offs // c, **dev)[:, None, None] + (f * bins + k if frames_major else k * torch.tensor(planes, **dev)[:, None, None] + f)
    mask = (f < Fd).expand(at.shape)
    gather = torch.where(mask, at, torch.zeros((), dtype=torch.int64, **dev))
    if not frames_major:
        gather, mask = gather.transpose(1, 2).contiguous(), mask.transpose(1, 2).contiguous()
    else:
        mask = mask.contiguous()
    del at
    count = torch.clamp(Fd.to(torch.float32), min=1.0)
    fdim = 1 if frames_major else 2
    cells_of = (lambda t: torch.view_as_complex(t.view(-1, 2))) if c == 2 else (lambda t: t)
    pad = torch.full((), pad_value, **dev).to(torch.complex64 if c == 2 else torch.float32) * (1 + 1j if c == 2 else 1)
    zero, ninf = torch.zeros((), **dev), torch.full((), -float("inf"), **dev)

    def p():
        decode_stft(rec.ctypes.data, packed.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def b():
        p()
        x = torch.where(mask, cells_of(packed)[gather], pad)
        if norm in ("whisper", "refmax"):
            m = torch.where(mask, x, ninf).amax(dim=(1, 2), keepdim=True)
            y = (torch.maximum(x, m - 8.0) + 4.0) / 4.0 if norm == "whisper" else (torch.maximum(x, m - 8.0) - m) * 10.0
            x = y if normalized else torch.where(mask, y, pad)
        elif norm in ("cmn", "cmvn"):
            mean = torch.where(mask, x, zero).sum(dim=fdim, keepdim=True) / count
            d = x - mean
            if norm == "cmvn":
                var = torch.where(mask, d * d, zero).sum(dim=fdim, keepdim=True) / count
                d = d / torch.sqrt(torch.clamp(var, min=float(sb.rec["var_floor"][0])))
            x = torch.where(mask, d, pad)
        torch.cuda.synchronize()
        return x

    def dense_call(request):
        def run():
            set_request(request)
            try:
                decode_stft(rec.ctypes.data, dense.data_ptr(), fo.ctypes.data, frames.ctypes.data, lengths.ctypes.data, status.ctypes.data)
            finally:
                set_request(None)
        return run
    c_leg, g_leg, d_leg = dense_call(sb), dense_call(sb_general), dense_call(sb_direct)

    p()
    spans = np.zeros(n, dtype=pkg.STFT_BATCH_SPAN_DTYPE)
    spans["grid_offset"], spans["plane"], spans["frames"] = feat_offs, planes, frames

    def s():
        stage_alone(spans, layout, sb, packed.data_ptr(), dense.data_ptr())
    # k_feat_batch beside it: norm NONE at width 128 over a grid of zeros with as many floats in the tensor
    n_f = max(1, n * bins * c // 128)
    fspans = np.zeros(n_f, dtype=pkg.FEAT_SPAN_DTYPE)
    fplane = (S + 63) // 64 * 64
    fspans["grid_offset"], fspans["plane"], fspans["frames"] = np.arange(n_f, dtype=np.int64) * 128 * fplane, fplane, int(np.round(F.mean()))
    fgrid = torch.zeros(n_f * 128 * fplane + 64, dtype=torch.float32, **dev)
    fdense = torch.empty(n_f * 128 * S + 64, dtype=torch.float32, **dev)
    fb = pkg.feature_batch_request(fspans["frames"], 128, S)

    def f_leg():
        feat_stage_alone(fspans, 128, layout, fb, fgrid.data_ptr(), fdense.data_ptr())

    legs = (("p", p), ("b", b), ("c", c_leg), ("g", g_leg), ("d", d_leg), ("s", s), ("f", f_leg))
    times = {name: [] for name, _ in legs}
    for _, fn in legs:
        fn()
    for _ in range(reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    peaks = {}
    for name, fn in (("g", g_leg), ("d", d_leg)):
        torch.cuda.synchronize()
        with _PeakMemory(torch) as peak:
            fn()
        peaks[name] = peak.bytes
    # the results against each other: the two paths bit for bit over the real frames and the pad, (c) against torch
    g_leg()
    assert (status[:, 0] == 0).all() and (frames == F).all() and (fo == np.arange(n) * (S64 + 1) * bins * c).all()
    gen = dense[:n * (S64 + 1) * bins * c].view((n, S64 + 1, bins * c) if frames_major else (n, bins, S64 + 1, c)).clone()
    d_leg()
    dire = dense[:n * S64 * bins * c].view((n, S64, bins * c) if frames_major else (n, bins, S64, c))
    same = bool(torch.equal((gen[:, :S64] if frames_major else gen[:, :, :S64]).contiguous().view(torch.int32), dire.contiguous().view(torch.int32)))
    assert same, "the direct and the general path differ"
    c_leg()
    want = b()
    got = cells_of(dense[:n * S * bins * c]).view(want.shape)
    worst = float((got - want).abs().max())
    assert worst < 1e-3, worst
    real = int(frames.sum()) * bins * c * 4
    stage_bytes = real * (2 if norm in ("whisper", "refmax", "cmn", "cmvn") else 1) + n * S * bins * c * 4
    feat_bytes = int(fspans["frames"].sum()) * 128 * 4 + n_f * S * 128 * 4
    out = {"stft_batch": [S, norm], "bins": bins, "c": c, "layout": layout, "files": n, "frames": int(frames.sum()), "reps": reps, "note": note,
           "packed_bytes": int(total) * 4, "dense_bytes": n * S * bins * c * 4, "direct_stride": S64, "paths_equal": same,
           "worst_abs_vs_torch": worst, "peak_bytes_general": int(peaks["g"]), "peak_bytes_direct": int(peaks["d"]),
           "stage_bytes": stage_bytes, "feat_stage_bytes": feat_bytes}
    for key, label in (("p", "p_packed_call"), ("b", "b_packed_then_torch_pad_and_norm"), ("c", "c_dense_as_asked"), ("g", "g_dense_general_none"),
                       ("d", "d_dense_direct_none"), ("s", "s_stage_call"), ("f", "f_feat_stage_call_none_w128")):
        v = np.array(times[key])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["s_gb_per_s"] = round(stage_bytes / np.mean(times["s"]) / 1e6, 1)
    out["f_gb_per_s"] = round(feat_bytes / np.mean(times["f"]) / 1e6, 1)
    return out


# the parameter sets of --fbank: (maker, its arguments, up, down); those at 16 kHz are followed by --melspec kaldi at the same files
FBANK_SETS = {
    "wenet": ("kaldi_fbank", dict(sample_rate=16000, num_mel_bins=80), 1, 3),
    "mfcc": ("kaldi_mfcc", dict(sample_rate=16000, num_mel_bins=23, num_ceps=13), 1, 3),
    "mfcc8k": ("kaldi_mfcc", dict(sample_rate=8000, num_mel_bins=23, num_ceps=13), 1, 6),
    "wide": ("kaldi_fbank", dict(sample_rate=48000, num_mel_bins=128, window_type="blackman", high_freq=-400.0), 1, 1),
}

# the parameter sets of --stft, those of tests/test_tracks_stft.py: (stft_spec arguments, up, down)
STFT_SETS = {
    "tiny": (dict(sample_rate=8000, n_fft=64, hop=24, win_length=48, power=2, log="ln", floor=1e-10), 1, 6),
    "enh": (dict(sample_rate=16000, n_fft=512, hop=128, win_length=400, power=None), 1, 3),
    "vits": (dict(sample_rate=22050, n_fft=1024, hop=256, power=1), 147, 320),
    "wide": (dict(sample_rate=44100, n_fft=2048, hop=960, power=2, log="log10", floor=1e-10), 147, 160),
    "whisper_lin": (dict(sample_rate=16000, n_fft=400, hop=160, power=2, frames="whisper"), 1, 3),
    # those of tests/test_tracks_fft.py: algo="fft" (the sets above take it from --stft-algo)
    "fft_tiny": (dict(sample_rate=8000, n_fft=64, hop=24, win_length=48, power=2, log="ln", floor=1e-10, algo="fft"), 1, 6),
    "fft_enh": (dict(sample_rate=16000, n_fft=512, hop=128, win_length=400, power=None, algo="fft"), 1, 3),
    "fft_vits": (dict(sample_rate=22050, n_fft=1024, hop=256, power=1, algo="fft"), 147, 320),
    "fft_wide": (dict(sample_rate=44100, n_fft=2048, hop=960, power=2, log="log10", floor=1e-10, algo="fft"), 147, 160),
    "fft_sep": (dict(sample_rate=44100, n_fft=4096, hop=1024, power=None, algo="fft"), 147, 160),
    "fft_big": (dict(sample_rate=48000, n_fft=8192, hop=1000, win_length=6000, power=2, log="log10", floor=1e-10, frames="whisper", algo="fft"), 1, 1),
}


def stft_record(pkg, name, layout, algo=None):
    """The stft_spec record of --stft NAME --stft-layout LAYOUT [--stft-algo ALGO] -> (record, up, down)."""
    kw, up, down = STFT_SETS[name]
    if algo is not None:
        kw = dict(kw, algo=algo)
    return pkg.stft_spec(feature_layout=layout, **kw), up, down

# the parameter sets of --melspec: (mel_spec arguments, up, down)
SPEC_SETS = {
    "tts": (dict(sample_rate=22050, n_fft=1024, hop=256, n_mels=80, fmax=8000.0, power=1, log="ln", floor=1e-5), 147, 320),
    "kaldi": (dict(sample_rate=16000, n_fft=512, hop=160, win_length=400, n_mels=80, fmin=20.0, mel_scale="htk", norm=None, log="ln",
                   floor=1.1920929e-7), 1, 3),
    "clap": (dict(sample_rate=48000, n_fft=1024, hop=480, n_mels=64, fmin=50.0, fmax=14000.0, mel_scale="htk", norm=None), 1, 1),
    "music": (dict(sample_rate=44100, n_fft=2048, hop=441, win_length=1102, n_mels=128), 147, 160),
    # mf_sep and mf_big of tests/test_tracks_melfft.py: algo="fft" only, no dense record reaches these sizes
    "sep": (dict(sample_rate=44100, n_fft=4096, hop=1024, n_mels=128, algo="fft"), 147, 160),
    "big": (dict(sample_rate=48000, n_fft=8192, hop=1000, win_length=6000, n_mels=64, fmin=50.0, fmax=14000.0, mel_scale="htk", norm=None,
                 frames="whisper", algo="fft"), 1, 1),
}


def spec_record(pkg, name, layout="bands", algo=None):
    """The mel_spec record of --melspec NAME [--melspec-layout LAYOUT] [--melspec-algo ALGO] -> (record, up, down)."""
    kw, up, down = SPEC_SETS[name]
    if algo is not None:
        kw = dict(kw, algo=algo)
    return pkg.mel_spec(feature_layout=layout, **kw), up, down
