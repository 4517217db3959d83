"""What tools/files_rate.py and tools/ms_files_rate.py run for --format: the whole decode call of a planned batch per track format
(include/opusgpu.h TRACK FORMATS) into torch tensors, variants interleaved per repeat:
(a) int16 tracks; (b) (a) followed by the conversion a consumer runs on them in torch -- .to(torch.float32) * scale, for planar the
de-interleave as well; (c) the fused format itself.  Medians, means, min / max; the condition is mean(fused) <= mean(b) with (a)'s
spread as the margin.  torch must be imported before the library is loaded: they then share one HIP runtime."""
import time

import numpy as np


def compare(torch, pkg, call, handle, chk, batch, fmt, reps, pipeline_note=""):
    """call: the *_files_decode_as entry of the library; fmt: "f32" or "f32_planar".  -> a dict for the JSON line."""
    n, ch = batch.n_files, batch.channels
    total = max(int(batch.track_samples), 1) * ch
    s16 = torch.empty(total, dtype=torch.int16, device="cuda:0")
    f32 = torch.empty(total, dtype=torch.float32, device="cuda:0")
    lengths = np.zeros(n, dtype=np.int64)
    status = np.zeros((n, 2), dtype=np.int32)
    planar = fmt == "f32_planar"

    def run(code, t):
        chk(call(handle, batch.h, code, None, t.data_ptr(), lengths.ctypes.data, status.ctypes.data), "files_decode_as")

    def a():
        run(pkg.TRACKS_S16, s16)

    def b():
        run(pkg.TRACKS_S16, s16)
        x = s16.to(torch.float32) * (1.0 / 32768)
        if planar:
            x = x.view(-1, ch).t().contiguous()
        torch.cuda.synchronize()
        return x

    def c():
        run(pkg.TRACKS_F32_PLANAR if planar else pkg.TRACKS_F32, f32)

    times = {"a": [], "b": [], "c": []}
    for fn in (a, b, c):
        fn()
    for _ in range(reps):
        for name, fn in (("a", a), ("b", b), ("c", c)):
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    assert (status[:, 0] == 0).all() and (lengths == batch.info["track_samples"]).all()
    # the fused tracks are the converted int16 ones, bit for bit (scale 2**-15; padding is not compared)
    o, ln = int(batch.info["track_offset"][n // 2]), int(lengths[n // 2])
    want = s16[ch * o:ch * (o + ln)].to(torch.float32) * (1.0 / 32768)
    if planar:  # channel c of the track: `ln` samples at c * plane, plane = the planned length rounded up to 64
        plane = (int(batch.info["track_samples"][n // 2]) + 63) // 64 * 64
        for c in range(ch):
            assert torch.equal(f32[ch * o + c * plane:ch * o + c * plane + ln], want[c::ch])
    else:
        assert torch.equal(f32[ch * o:ch * (o + ln)], want)
    out = {"format": fmt, "files": n, "reps": reps, "note": pipeline_note}
    for k, label in (("a", "a_s16"), ("b", "b_s16_then_torch"), ("c", "c_fused")):
        v = np.array(times[k])
        out[label] = {"mean_ms": round(float(v.mean()), 3), "median_ms": round(float(np.median(v)), 3), "min_max_ms": [round(float(v.min()), 3), round(float(v.max()), 3)]}
    spread = max(times["a"]) - min(times["a"])
    out["a_spread_ms"] = round(spread, 3)
    out["condition_fused_le_two_pass_plus_spread"] = bool(np.mean(times["c"]) <= np.mean(times["b"]) + spread)
    return out
