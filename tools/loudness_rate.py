"""What a loudness request adds to a whole-file call (include/opusgpu.h, TRACK LOUDNESS): the call of one decode_files request
without the request, with loudness="measure" and, with a target, normalising -- interleaved, device-resident (the result stays in
HBM), host clock around the call, which waits for its own work.  The share is the added time over the time of the call with the
request.  Used by tools/files_rate.py --loudness and tools/ms_files_rate.py --loudness."""
import time

import numpy as np


def call_of(pkg, lib, prefix, handle, chk, batch, req, d_out):
    """The C call a FilesRequest means, into d_out: what decode_files does with it, without the copy to the host."""
    n = batch.n_files
    offsets, counts, lengths = (np.zeros(n, dtype=np.int64) for _ in range(3))
    status = np.zeros((n, 2), dtype=np.int32)
    head = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in req.args]
    if req.entry != "files_decode":
        head += ([] if req.kind == "features" else [req.fmt]) + [None if req.scale is None else req.scale.ctypes.data]
    tail = [a.ctypes.data for a in ((lengths, status) if req.kind == "tracks" else (offsets, counts, lengths, status))]
    fn, loud = getattr(lib, prefix + req.entry), getattr(req, "loudness", None)

    def run():
        if loud is not None:
            chk(getattr(lib, prefix + "set_loudness")(handle, loud.ctypes.data), "set_loudness")
        try:
            chk(fn(handle, batch.h, *head, d_out, *tail), prefix + req.entry)
        finally:
            if loud is not None:
                getattr(lib, prefix + "set_loudness")(handle, None)
    run.lengths = lengths
    run.keep = (offsets, counts, lengths, status, req)  # the call writes through their addresses: they live as long as `run`
    return run


def spread(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def compare(pkg, mem, lib, prefix, handle, chk, batch, multistream, reps, target, name, **kw):
    """kw: the keywords of decode_files that name the output.  mem: a Context for the result's buffer.  -> a dict for one JSON line."""
    variants = [("plain", {}), ("measure", {"loudness": "measure"})] + ([("normalize", {"loudness": float(target)})] if target is not None else [])
    reqs = [(v, pkg.files_request(batch, multistream, 0, **kw, **more)) for v, more in variants]
    need = max(max(r.total, 1) * r.channels * (2 if r.fmt == pkg.TRACKS_S16 else 4) for _, r in reqs)
    d_out = mem.dev_alloc(need + 256)
    try:
        runs = [(v, r.entry, call_of(pkg, lib, prefix, handle, chk, batch, r, d_out)) for v, r in reqs]
        for _, _, run in runs:
            run()  # warm: buffers that only grow, code objects
        times = {v: [] for v, _, _ in runs}
        for _ in range(reps):
            for v, _, run in runs:
                t0 = time.perf_counter()
                run()
                times[v].append((time.perf_counter() - t0) * 1e3)
    finally:
        mem.dev_free(d_out)
    out = {"case": name, "files": batch.n_files, "seconds_of_audio": round(float(runs[0][2].lengths.sum()) / 48000, 1), "reps": reps}
    for v, entry, _ in runs:
        out[v] = dict(spread(times[v]), entry=prefix + entry)
    for v in times:
        if v != "plain":
            added = float(np.median(times[v])) - float(np.median(times["plain"]))
            out[v]["added_ms"], out[v]["share"] = round(added, 3), round(added / float(np.median(times[v])), 4)
    return out
