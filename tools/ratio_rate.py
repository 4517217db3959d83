"""What tools/files_rate.py and tools/ms_files_rate.py run for --resample UP/DOWN: the whole decode call of a planned batch into
torch tensors, three variants interleaved per repeat (include/opusgpu.h TRACK RATIOS):
(a) the fused call, float32 tracks at 48000 up / down Hz; (b) rate=24000 on the same corpus, float32 -- the nearest call there was
before, the yardstick per output sample; (c) float32 tracks at 48 kHz followed by the resampling a consumer runs on them in torch:
a polyphase conv1d over the packed buffer, one output channel per m mod up, stride `down`, with the same taps (ONE convolution
over all tracks: cheaper than the per-track ones a consumer needs to keep tracks apart, so (c) is a lower bound).
Then the two kernels alone on the int16 tracks of the same batch: k_tracks_resample_ratio and k_tracks_resample<2> through their
device calls (each uploads its tables, launches and waits), per output sample.
torch must be imported before the library is loaded: they then share one HIP runtime."""
import time

import numpy as np


def polyphase_weight(pkg, up, down):
    """-> (float32 weight [up, 1, K], left padding) of the conv1d with stride `down` whose output channel r, position q, is output
    q up + r: sum_j h[p_r + j up] x[q down + b_r - j], p_r and b_r the phase and newest sample of output r."""
    h = pkg.resample_ratio_taps(up, down).astype(np.float64) / 32768
    lp, c = len(h), 12 * down
    T = -(-lp // up)
    t = np.arange(up) * down + c
    p, b = t % up, t // up
    pad = T - 1 - int(b[0])
    K = int(b[-1]) + pad + 1
    w = np.zeros((up, 1, K), dtype=np.float32)
    for r in range(up):
        for j in range(T):
            if p[r] + j * up < lp:
                w[r, 0, b[r] - j + pad] = h[p[r] + j * up]
    return w, pad


def compare(torch, pkg, decode_f32, decode_rate, decode_ratio, decode_s16, kernels, batch, up, down, mono, reps, note="", mix=None):
    """decode_f32(d_tracks, lengths, status), decode_rate(fmt, d_out, out_offsets, out_lengths, lengths, status) at 24000 and
    decode_ratio(the same arguments) at up / down, decode_s16(d_tracks, lengths, status): the library's calls for the batch, each
    returning its code's check; kernels = (ratio(spans, d_in, fmt, d_out), rate(spans, d_in, fmt, d_out)): the two device calls.
    mix: None or the int16 Q14 matrix [out, in] the resampling calls apply.  -> a dict for the JSON line."""
    n, ch = batch.n_files, batch.channels
    ch_out = len(mix) if mix is not None else 1 if mono else ch
    total = max(int(batch.track_samples), 1)
    q_offs, q_total = pkg.resample_ratio_layout(batch.info["track_samples"], up, down)
    r_offs, r_total = pkg.resample_layout(batch.info["track_samples"], 24000)
    f32 = torch.empty(total * ch, dtype=torch.float32, device="cuda:0")
    s16 = torch.empty(total * ch, dtype=torch.int16, device="cuda:0")
    res_q = torch.empty(max(q_total, 1) * ch_out, dtype=torch.float32, device="cuda:0")
    res_r = torch.empty(max(r_total, 1) * ch_out, dtype=torch.float32, device="cuda:0")
    lengths, out_offsets, out_lengths = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    w_np, pad = polyphase_weight(pkg, up, down)
    w = torch.tensor(w_np, device="cuda:0")
    if mix is not None:
        m_t = torch.tensor(np.asarray(mix, dtype=np.float32).T / 16384, device="cuda:0")  # [in, out]

    def a():
        decode_ratio(pkg.TRACKS_F32, res_q.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def b():
        decode_rate(pkg.TRACKS_F32, res_r.data_ptr(), out_offsets.ctypes.data, out_lengths.ctypes.data, lengths.ctypes.data, status.ctypes.data)

    def c():
        decode_f32(f32.data_ptr(), lengths.ctypes.data, status.ctypes.data)
        x = f32.view(-1, ch)
        x = (x @ m_t).t() if mix is not None else x.t()  # [channels, samples]
        if mono:
            x = x.mean(0, keepdim=True)
        x = torch.nn.functional.pad(x.unsqueeze(1), (pad, w.shape[-1]))
        y = torch.nn.functional.conv1d(x, w, stride=down).permute(0, 2, 1).reshape(x.shape[0], -1)  # [channels, outputs]
        torch.cuda.synchronize()
        return y

    times = {"a": [], "b": [], "c": []}
    for fn in (a, b, c):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a), ("b", b), ("c", c)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    a()
    assert (status[:, 0] == 0).all() and (lengths == batch.info["track_samples"]).all() and (out_offsets == q_offs).all()
    q_lengths = out_lengths.copy()
    # one track of (a) against the float convolution of (c): the same filter up to float rounding and the int16 rounding of y
    y = c()
    fits = [j for j in range(n // 2, n) if batch.info["track_offset"][j] % down == 0 and q_lengths[j] > 60]  # (c)'s grid meets the track's
    worst = None
    if fits:
        i = fits[0]
        o, oo, on = int(batch.info["track_offset"][i]) // down * up, int(q_offs[i]), int(q_lengths[i])
        got = res_q[ch_out * oo:ch_out * (oo + on)].view(on, ch_out)
        want = y[:, o:o + on].t()
        inner = slice(28, on - 28)  # away from the track's ends, where (c) sees the neighbouring tracks
        worst = float((got[inner] - want[inner]).abs().max()) * 32768
        assert worst < (3.0 if mix is not None else 2.0), worst
    # the kernels alone, on the int16 tracks of this batch
    decode_s16(s16.data_ptr(), lengths.ctypes.data, status.ctypes.data)
    spans_q, spans_r = (np.zeros(n, dtype=pkg.RESAMPLE_SPAN_DTYPE) for _ in range(2))
    for spans, offs, u, d in ((spans_q, q_offs, up, down), (spans_r, r_offs, 1, 2)):
        spans["in_offset"], spans["in_samples"], spans["out_offset"] = batch.info["track_offset"], lengths, offs
        spans["out_plane"], spans["scale"] = (-(-batch.info["track_samples"] * u // d) + 63) // 64 * 64, 2.0 ** -15
    ktimes = {"ratio": [], "rate": []}
    for _ in range(reps + 1):
        for name, fn, spans, res in (("ratio", kernels[0], spans_q, res_q), ("rate", kernels[1], spans_r, res_r)):
            t0 = time.perf_counter()
            fn(spans, s16.data_ptr(), pkg.TRACKS_F32, res.data_ptr())
            ktimes[name].append((time.perf_counter() - t0) * 1e3)
    out_q, out_r = int(q_lengths.sum()) * ch_out, int((-(-lengths // 2)).sum()) * ch_out
    out = {"resample": [up, down], "mono": bool(mono), "mix": None if mix is None else np.asarray(mix).tolist(), "files": n, "reps": reps,
           "note": note, "out_samples_ratio": out_q, "out_samples_24k": out_r,
           "worst_lsb_vs_float_conv": worst if fits else "not checked: no track on the grid of (c)"}
    for k, label in (("a", "a_fused_ratio"), ("b", "b_rate_24000"), ("c", "c_f32_48k_then_torch_polyphase")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3),
                      "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    out["call_ns_per_output_sample"] = {"a_fused_ratio": round(float(np.median(times["a"])) * 1e6 / max(out_q, 1), 4),
                                        "b_rate_24000": round(float(np.median(times["b"])) * 1e6 / max(out_r, 1), 4)}
    out["call_fused_to_24000_per_output_sample"] = round(out["call_ns_per_output_sample"]["a_fused_ratio"] /
                                                         max(out["call_ns_per_output_sample"]["b_rate_24000"], 1e-12), 3)
    kq, kr = float(np.median(ktimes["ratio"][1:])), float(np.median(ktimes["rate"][1:]))
    out["kernel_call_ms"] = {"k_tracks_resample_ratio": round(kq, 3), "k_tracks_resample_2": round(kr, 3)}
    out["kernel_call_fused_to_24000_per_output_sample"] = round((kq / max(out_q, 1)) / max(kr / max(out_r, 1), 1e-12), 3)
    return out
