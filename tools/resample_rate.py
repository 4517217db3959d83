"""What tools/files_rate.py and tools/ms_files_rate.py run for --rate: the whole decode call of a planned batch into torch tensors,
variants interleaved per repeat (include/opusgpu.h TRACK RATES):
(a) int16 tracks at 48 kHz, the call as it was; (b) (a) followed by the conversion a consumer runs on them in torch -- to float,
the downmix when --mono, and a float conv1d with stride D over the packed buffer with the same taps (ONE convolution over all
tracks: cheaper than the per-track ones a consumer needs to keep tracks apart, so (b) is a lower bound); (c) the new call, float32
tracks at the rate.  Means, medians, min / max; the condition is mean(c) <= mean(b) with (a)'s spread (max - min) as the margin.
With --mix (include/opusgpu.h CHANNEL MIX) the consumer's work in (b) is to float, `@ M.T`, the strided conv1d, and (c) is the
mixed call: decode_resampled then runs opusgpu_files_decode_mixed or opusgpu_ms_files_decode_mixed.
torch must be imported before the library is loaded: they then share one HIP runtime."""
import time

import numpy as np


def compare(torch, pkg, decode_s16, decode_resampled, batch, rate, mono, reps, note="", mix=None):
    """decode_s16(d_tracks, lengths, status) and decode_resampled(fmt, d_out, out_offsets, out_lengths, lengths, status) run the
    library's calls for the batch and return their codes' check.  mix: None or the int16 Q14 matrix [out, in] that
    decode_resampled applies.  -> a dict for the JSON line."""
    n, ch = batch.n_files, batch.channels
    D = pkg.TRACK_RATES[rate]
    ch_out = len(mix) if mix is not None else 1 if mono else ch
    total = max(int(batch.track_samples), 1)
    offs, out_total = pkg.resample_layout(batch.info["track_samples"], rate)
    s16 = torch.empty(total * ch, dtype=torch.int16, device="cuda:0")
    res = torch.empty(max(out_total, 1) * ch_out, dtype=torch.float32, device="cuda:0")
    lengths, out_offsets, out_lengths = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    if D > 1:
        h = torch.tensor(pkg.resample_taps(rate).astype(np.float32) / 32768, device="cuda:0").view(1, 1, -1)

    if mix is not None:
        m_t = torch.tensor(np.asarray(mix, dtype=np.float32).T / 16384, device="cuda:0")  # [in, out]

    def a():
        decode_s16(s16.data_ptr(), lengths.ctypes.data, status.ctypes.data)

    def b():
        a()
        if mix is not None:
            x = ((s16.view(-1, ch).to(torch.float32) * (1.0 / 32768)) @ m_t).t()  # [out, samples]
        else:
            x = s16.view(-1, ch).t().to(torch.float32) * (1.0 / 32768)  # [ch, samples]
        if mono:
            x = x.mean(0, keepdim=True)
        if D > 1:
            x = torch.nn.functional.conv1d(x.unsqueeze(1), h, stride=D, padding=(h.shape[-1] - 1) // 2).squeeze(1)
        torch.cuda.synchronize()
        return x

    def c():
        decode_resampled(pkg.TRACKS_F32, res.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data,
                         status.ctypes.data)

    times = {"a": [], "b": [], "c": []}
    for fn in (a, b, c):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a), ("b", b), ("c", c)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    assert (status[:, 0] == 0).all() and (lengths == batch.info["track_samples"]).all() and (out_offsets == offs).all()
    # one track of (c) against the float convolution of (b): the same filter up to float rounding and the int16 rounding of y
    x = b()
    fits = [j for j in range(n // 2, n) if batch.info["track_offset"][j] % D == 0 and out_lengths[j] > 26]  # (b)'s grid meets the track's
    worst = None  # no such track (few or short files): the timing stands, the cross-check is left out
    if fits:
        i = fits[0]
        o, oo, on = int(batch.info["track_offset"][i]), int(offs[i]), int(out_lengths[i])
        got = res[ch_out * oo:ch_out * (oo + on)].view(on, ch_out)
        want = x[:, o // D:o // D + on].t()
        inner = slice(13, on - 13)  # away from the track's ends, where (b) sees the neighbouring tracks
        worst = float((got[inner] - want[inner]).abs().max()) * 32768
        assert worst < (3.0 if mix is not None else 2.0), worst  # the mix rounds to int16 once more, in front of the filter
    out = {"rate": rate, "mono": bool(mono), "mix": None if mix is None else np.asarray(mix).tolist(), "files": n, "reps": reps, "note": note, "scratch_s16_bytes": total * ch * 2,
           "out_bytes": int(res.numel()) * 4, "worst_lsb_vs_float_conv": worst if fits else "not checked: no track on the grid of (b)"}
    for k, label in (("a", "a_s16"), ("b", "b_s16_then_torch"), ("c", "c_resampled")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    spread = max(times["a"]) - min(times["a"])
    out["a_spread_ms"] = round(spread, 3)
    out["condition_c_le_b_plus_spread"] = bool(np.mean(times["c"]) <= np.mean(times["b"]) + spread)
    return out
