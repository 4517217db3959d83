"""What tools/files_rate.py --cuts and tools/ms_files_rate.py --cuts measure (include/opusgpu.h WHOLE FILES / CUTS): F long files
decoded whole, then C random cuts of S seconds out of each of them as F x C tracks, in one process; the planner's time for both;
the share of decoded frames that is pre-roll; and with a stride what the zeroed tails cost over the packed cut batch."""
import time

import numpy as np


def _timed(fn, reps):
    fn()  # warm: allocations, first launches
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def _stats(ms):
    return {"mean_s": round(float(np.mean(ms)), 4), "min_s": round(min(ms), 4), "max_s": round(max(ms), 4), "runs": len(ms)}


def compare(pkg, mem, make_batch, decode, blobs, cuts_per_file, seconds, strided, reps, whole_reps, plan_reps, what):
    """make_batch(**keywords of cuts / stride) -> a planned batch of `blobs`; decode(batch, d_tracks, lengths, status) runs it into
    device memory and waits; mem: a Context for the device buffers.  -> the JSON record."""
    n_files = len(blobs)

    def plan(**kw):
        best, b = None, None
        for _ in range(plan_reps):
            if b is not None:
                b.close()
            t0 = time.perf_counter()
            b = make_batch(**kw)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return b, best

    whole, whole_plan_s = plan()
    assert (whole.info["status"] == 0).all()
    count = int(round(seconds * 48000))
    rng = np.random.default_rng(11)
    cuts = []
    for i, ln in enumerate(whole.info["track_samples"]):
        assert ln > count, "the files are shorter than a cut"
        cuts += [(i, int(s), count) for s in rng.integers(0, int(ln) - count, cuts_per_file)]
    packed, cuts_plan_s = plan(cuts=cuts)
    assert (packed.info["track_samples"] == count).all()
    batches = [("whole_files", whole, whole_reps), ("cuts", packed, reps)]
    if strided:  # cuts of unequal length, half a cut to a whole one, packed and at the stride that holds the longest: tails to zero
        varied = [(i, s, int(rng.integers(count // 2, count + 1))) for i, s, _ in cuts]
        stride = (count + 63) // 64 * 64
        batches += [("cuts_varied", make_batch(cuts=varied), reps), ("cuts_varied_strided", make_batch(cuts=varied, stride=stride), reps)]
        tail = sum(stride - c[2] for c in varied)
    out = {"what": what, "files": n_files, "packets_per_file": int(whole.info["packets"][0]), "cuts_per_file": cuts_per_file,
           "cut_seconds": seconds, "cuts": len(cuts),
           "plan": {"whole_files_s": round(whole_plan_s, 4), "cuts_s": round(cuts_plan_s, 4),
                    "whole_ms_per_file": round(whole_plan_s / n_files * 1e3, 3), "cuts_ms_per_file": round(cuts_plan_s / n_files * 1e3, 3),
                    "cuts_over_whole": round(cuts_plan_s / whole_plan_s, 3), "files_per_s": round(n_files / cuts_plan_s, 1),
                    "cuts_per_s": round(len(cuts) / cuts_plan_s)},
           "preroll": {"lead_samples": int(packed.cut_info["lead"].sum()), "cut_samples": int(packed.info["track_samples"].sum()),
                       "discarded_share_of_samples": round(float(packed.cut_info["lead"].sum() / packed.info["track_samples"].sum()), 4),
                       "frames_decoded": int(packed.info["frames"].sum()), "exact_cuts": int(packed.cut_info["exact"].sum())}}
    for name, b, r in batches:
        if r <= 0:  # (--whole-reps 0: a kernel trace of the cut batches alone)
            b.close()
            continue
        n = b.n_files
        d = mem.dev_alloc(max(int(b.track_samples), 1) * b.channels * 2)
        lengths, status = np.zeros(n, dtype=np.int64), np.zeros((n, 2), dtype=np.int32)
        try:
            t = _timed(lambda: decode(b, d, lengths.ctypes.data, status.ctypes.data), r)
        finally:
            mem.dev_free(d)
        assert (status[:, 0] == 0).all() and (lengths == b.info["track_samples"]).all()
        audio_s = float(lengths.sum()) / 48000
        out[name] = dict(_stats(t), steps=b.n_steps, tracks=n, audio_seconds_out=round(audio_s, 1),
                         audio_seconds_per_second=round(audio_s / float(np.mean(t)), 1))
        b.close()
    if strided:
        out["stride"] = {"stride": stride, "tail_samples": int(tail), "tail_bytes_s16": int(tail) * packed.channels * 2,
                         "strided_minus_packed_s": round(out["cuts_varied_strided"]["mean_s"] - out["cuts_varied"]["mean_s"], 4)}
    return out
