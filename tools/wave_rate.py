"""What tools/files_rate.py and tools/ms_files_rate.py share for --wave-batch (include/opusgpu.h WAVE BATCHES): the fused call under
a wave-batch request next to the packed float call followed by the collate a user writes in torch today, and the stage's three
kernels alone for a kernel trace."""
import time

import numpy as np

NORMS = ("none", "zmuv", "peak")


def wave_batch_arg(text):
    """--wave-batch S[:NORM] -> (S or None, NORM): S 0 is the longest planned track, NORM one of none, zmuv, peak (default zmuv)."""
    s, _, norm = text.partition(":")
    norm = norm or "zmuv"
    if norm not in NORMS or int(s) < 0:
        raise ValueError(f"--wave-batch takes S[:none|zmuv|peak] with S >= 0, not {text!r}")
    return int(s) or None, norm


def compare_wave_batch(torch, pkg, resampled, set_request, batch, up, down, channels, stride, norm, reps, note=""):
    """--wave-batch S[:NORM]: resampled(format, d_out, out_offsets, out_lengths, lengths, status) runs a whole-file call of the batch
    that ends in a resampling kernel, whose tracks have `channels` channels at up / down of 48 kHz; set_request(WaveBatch or None) puts
    a request on the decoder or takes it off.
    (p) the packed float32 call as it was; (b) (p) followed by the torch form a user writes today -- the ragged tracks gathered into a
    padded [files, S, channels] tensor (the gather index is made once, outside the timing), the masked mean and variance per track
    and (x - mean) / sqrt(var + 1e-7) for zmuv, or the masked amax |x| for peak, and the mask; (c) the same call with the request
    on, which writes that tensor and the mask.  Variants interleaved per repeat; medians, means and the spread are printed, no
    ratio is asked.  -> a dict for the JSON line."""
    n, C = batch.n_files, channels
    planned = -(-np.asarray(batch.info["track_samples"], dtype=np.int64) * up // down)
    wb = pkg.wave_batch_request(planned, C, stride, {"none": None, "zmuv": "zmuv", "peak": ("peak", 1.0)}[norm], None, True)
    S = wb.stride
    offs = np.concatenate([[0], np.cumsum((planned + 63) // 64 * 64)])
    packed = torch.empty(max(int(offs[-1]) * C, 1), dtype=torch.float32, device="cuda:0")
    dense = torch.empty(max(wb.floats, 1), dtype=torch.float32, device="cuda:0")
    lengths, oo, ol = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    m, c = np.arange(S)[None, :, None], np.arange(C)[None, None, :]
    at = (offs[:n, None, None] + m) * C + c
    valid = np.broadcast_to(m < planned[:, None, None], at.shape)
    gather = torch.tensor(np.where(valid, at, 0), device="cuda:0")
    mask = torch.tensor(np.ascontiguousarray(valid), device="cuda:0")
    count = torch.tensor(np.maximum(planned * C, 1).astype(np.float32)[:, None, None], device="cuda:0")
    zero = torch.zeros((), device="cuda:0")
    tail = [a.ctypes.data for a in (oo, ol, lengths, status)]

    def p():
        resampled(pkg.TRACKS_F32, packed.data_ptr(), *tail)

    def b():
        p()
        x = torch.where(mask, packed[gather], zero)
        if norm == "zmuv":
            mean = x.sum(dim=(1, 2), keepdim=True) / count
            d = torch.where(mask, x - mean, zero)
            var = (d * d).sum(dim=(1, 2), keepdim=True) / count
            x = d / torch.sqrt(var + 1e-7)
        elif norm == "peak":
            peak = x.abs().amax(dim=(1, 2), keepdim=True)
            x = x / torch.where(peak > 0, peak, torch.ones((), device="cuda:0"))
        attention = mask[:, :, 0].to(torch.uint8)
        torch.cuda.synchronize()
        return x, attention

    def c_():
        set_request(wb)
        try:
            resampled(pkg.TRACKS_F32, dense.data_ptr(), *tail)
        finally:
            set_request(None)

    times = {"p": [], "b": [], "c": []}
    for fn in (p, b, c_):
        fn()
    for _ in range(reps):
        for name, fn in (("p", p), ("b", b), ("c", c_)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    c_()
    assert (status[:, 0] == 0).all() and (ol == planned).all() and (oo == np.arange(n) * S).all()
    want, attention = b()
    got = dense[:n * S * C].view(n, S, C)
    worst = float((got - want).abs().max())
    assert worst < 1e-2, worst  # (torch sums float32: the tool shows agreement, tests/test_gpu_wave_batch.py holds the bits)
    got_mask = dense.view(torch.uint8)[wb.mask_offset:wb.mask_offset + n * S].view(n, S)
    assert bool((got_mask == attention).all())
    real = int(planned.sum()) * C
    out = {"wave_batch": [S, norm], "channels": C, "ratio": [int(up), int(down)], "files": n, "samples": int(planned.sum()), "reps": reps,
           "note": note, "packed_bytes": int(offs[-1]) * C * 4, "dense_bytes": n * S * C * 4 + n * S, "worst_abs_vs_torch": worst,
           "k_wave_stats_bytes": 0 if norm == "none" else 2 * real, "k_wave_batch_bytes": 2 * real + 4 * n * S * C + n * S}
    for k, label in (("p", "p_packed_f32_call"), ("b", "b_packed_then_torch_collate"), ("c", "c_fused_wave_batch")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["c_le_b"] = bool(np.median(times["c"]) <= np.median(times["b"]))
    return out


def wave_trim_arg(pkg, text):
    """--wave-trim TOPDB[:FL:HOP] -> a trim_spec() record under the track's loudest frame (frame 2048, hop 512 by default)."""
    parts = text.split(":")
    if len(parts) not in (1, 3):
        raise ValueError(f"--wave-trim takes TOPDB[:FL:HOP], not {text!r}")
    fl, hop = (int(parts[1]), int(parts[2])) if len(parts) == 3 else (2048, 512)
    return pkg.trim_spec(float(parts[0]), fl, hop)


def compare_wave_trim(torch, pkg, resampled, set_request, set_trim, batch, up, down, channels, stride, norm, trim, reps, note=""):
    """--wave-batch S[:NORM] --wave-trim TOPDB[:FL:HOP]: as compare_wave_batch, with set_trim(record or None) for the trim request.
    (a) the fused wave-batch call without a trim; (c) the same call with the trim request on (include/opusgpu.h WAVE TRIM); (b) the
    packed int16 call followed by the same trim, gather, normalisation and mask in torch -- frame energies from an int64 running sum
    of squares (the frame table is made once, outside the timing), the per-track maximum, threshold, first and last active frame by
    scatter reductions, then the collate of compare_wave_batch from the trimmed spans.  Variants interleaved per repeat; medians,
    means and the spread are printed, no ratio is asked.  -> a dict for the JSON line."""
    n, C = batch.n_files, channels
    planned = -(-np.asarray(batch.info["track_samples"], dtype=np.int64) * up // down)
    wb = pkg.wave_batch_request(planned, C, stride, {"none": None, "zmuv": "zmuv", "peak": ("peak", 1.0)}[norm], None, True)
    S = wb.stride
    fl, hop, margin, ratio = int(trim["frame_length"][0]), int(trim["hop"][0]), int(trim["margin"][0]), float(trim["ratio"][0])
    assert int(trim["mode"][0]) == pkg.WAVE_TRIM_REL
    offs = np.concatenate([[0], np.cumsum((planned + 63) // 64 * 64)])
    packed = torch.empty(max(int(offs[-1]) * C, 1), dtype=torch.int16, device="cuda:0")
    dense = torch.empty(max(wb.floats, 1), dtype=torch.float32, device="cuda:0")
    lengths, oo, ol = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    tail = [a.ctypes.data for a in (oo, ol, lengths, status)]
    frames = pkg.wave_trim_frames(planned, hop)
    track = np.repeat(np.arange(n), frames)
    f = np.arange(int(frames.sum())) - np.repeat(np.cumsum(frames) - frames, frames)
    dev = dict(device="cuda:0")
    lo = torch.tensor(offs[track] + np.clip(f * hop - fl // 2, 0, planned[track]), **dev)
    hi = torch.tensor(offs[track] + np.clip(f * hop + fl // 2, 0, planned[track]), **dev)
    track_d, f_d, L_d, offs_d = (torch.tensor(v, **dev) for v in (track, f, planned, offs[:n]))
    m_d, c_d = torch.arange(S, **dev), torch.arange(C, **dev)
    zero = torch.zeros((), **dev)

    def a_():
        set_request(wb)
        try:
            resampled(pkg.TRACKS_F32, dense.data_ptr(), *tail)
        finally:
            set_request(None)

    def b():
        resampled(pkg.TRACKS_S16, packed.data_ptr(), *tail)
        y = packed.view(-1, C).to(torch.int64)
        run = torch.cat([torch.zeros((1, C), dtype=torch.int64, **dev), (y * y).cumsum(0)])
        M = (run[hi] - run[lo]).amax(dim=1)
        emax = torch.zeros(n, dtype=torch.int64, **dev).scatter_reduce(0, track_d, M, "amax")
        thr = torch.floor(emax.to(torch.float64) * ratio).to(torch.int64)
        on = M > thr[track_d]
        first = torch.full((n,), 1 << 40, dtype=torch.int64, **dev).scatter_reduce(0, track_d[on], f_d[on], "amin")
        last = torch.full((n,), -1, dtype=torch.int64, **dev).scatter_reduce(0, track_d[on], f_d[on], "amax")
        some = last >= 0
        start = torch.where(some, torch.clamp(first * hop - margin, min=0), 0)
        count = torch.where(some, torch.minimum(L_d, (last + 1) * hop + margin) - start, 0)
        valid = (m_d[None, :] < count[:, None])[:, :, None].expand(n, S, C)
        at = ((offs_d + start)[:, None] + m_d[None, :])[:, :, None] * C + c_d
        x = torch.where(valid, packed[torch.where(valid, at, 0)].to(torch.float32) * 2.0 ** -15, zero)
        size = torch.clamp(count * C, min=1).to(torch.float32)[:, None, None]
        if norm == "zmuv":
            mean = x.sum(dim=(1, 2), keepdim=True) / size
            d = torch.where(valid, x - mean, zero)
            var = (d * d).sum(dim=(1, 2), keepdim=True) / size
            x = d / torch.sqrt(var + 1e-7)
        elif norm == "peak":
            peak = x.abs().amax(dim=(1, 2), keepdim=True)
            x = x / torch.where(peak > 0, peak, torch.ones((), **dev))
        attention = valid[:, :, 0].to(torch.uint8)
        torch.cuda.synchronize()
        return x, attention, start, count

    def c_():
        set_request(wb)
        try:
            set_trim(trim)
            resampled(pkg.TRACKS_F32, dense.data_ptr(), *tail)
        finally:
            set_trim(None)
            set_request(None)

    times = {"a": [], "b": [], "c": []}
    for fn in (a_, b, c_):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a_), ("b", b), ("c", c_)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    want, attention, start, count = b()
    c_()
    kept = count.cpu().numpy()
    assert (status[:, 0] == 0).all() and (ol == kept).all() and (oo == np.arange(n) * S).all()
    got = dense[:n * S * C].view(n, S, C)
    worst = float((got - want).abs().max())
    assert worst < 1e-2, worst  # (torch sums float32: the tool shows agreement, tests/test_gpu_wave_trim.py holds the bits)
    got_mask = dense.view(torch.uint8)[wb.mask_offset:wb.mask_offset + n * S].view(n, S)
    assert bool((got_mask == attention).all())
    real = int(planned.sum()) * C
    out = {"wave_batch": [S, norm], "wave_trim": [float(-10 * np.log10(ratio)), fl, hop], "channels": C, "ratio": [int(up), int(down)], "files": n,
           "samples": int(planned.sum()), "kept_samples": int(kept.sum()), "trimmed_tracks": int((kept < planned).sum()), "reps": reps, "note": note,
           "worst_abs_vs_torch": worst, "k_wave_trim_energy_bytes": 2 * real, "k_wave_stats_bytes": 0 if norm == "none" else 2 * int(kept.sum()) * C}
    for k, label in (("a", "a_fused_wave_batch"), ("b", "b_packed_s16_then_torch_trim_collate"), ("c", "c_fused_wave_batch_trimmed")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    return out


def kernels_alone(pkg, ctx, n, length, channels, stride, norm, format="f32", launches=5):
    """k_wave_stats, k_wave_fold and k_wave_batch alone over n tracks of `length` samples of random int16 at stride `stride`, `launches`
    times, for a `rocprofv3 --kernel-trace --stats` run -> the bytes each kernel moves per launch (read + written)."""
    C = channels
    plane = (length + 63) // 64 * 64
    spans = np.zeros(n, dtype=pkg.WAVE_SPAN_DTYPE)
    spans["in_offset"], spans["samples"], spans["scale"] = np.arange(n) * plane, length, 2.0 ** -15
    wb = pkg.wave_batch_request(np.full(n, length), C, stride, {"none": None, "zmuv": "zmuv", "peak": ("peak", 1.0)}[norm], None, True)
    tracks = np.random.default_rng(1).integers(-32768, 32768, n * plane * C, dtype=np.int16)
    d_in, d_out = ctx.dev_alloc(tracks.nbytes + 64), ctx.dev_alloc(4 * wb.floats)
    try:
        ctx.h2d(d_in, tracks)
        for _ in range(launches):
            ctx.tracks_wave_batch_device(spans, C, format, wb, d_in, d_out)
    finally:
        ctx.dev_free(d_in)
        ctx.dev_free(d_out)
    real = n * length * C
    return {"tracks": n, "samples": length, "channels": C, "stride": stride, "norm": norm, "format": format, "launches": launches,
            "k_wave_stats_bytes": 0 if norm == "none" else 2 * real, "k_wave_batch_bytes": 2 * real + 4 * n * stride * C + n * stride}
