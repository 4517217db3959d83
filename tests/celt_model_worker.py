"""Child process of tests/test_gpu_celt_model.py::test_reference_mode_through_the_single_kernel.  The parent puts OPUSGPU_SPLIT=0 into
the environment (og_debug.hpp reads its switches once per process), so that EVERY frame of a reference-mode step goes through
k_decode_step (og_step.hpp step_single_kernel) -- the general path that by default decodes only the parked Q4 frames.  Here the
reference-mode plans of tests/celt_model_plans.py run through it: ref_switch and ref_celt, PCM equal to the oracle's everywhere and
the PCM of every CELT-only frame within TOL_PCM of the float64 model.  Also home of through_decode_packets, which the parent uses
on the default routes.  (GPU box.)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def groups(plan):
    """the plan's streams by decoder channel count (a context holds streams of one count): {channels: [stream indices]}"""
    g = {}
    for i, st in enumerate(plan["streams"]):
        g.setdefault(st["channels"], []).append(i)
    return g


def through_decode_packets(ctx, plan, dec, rfc):
    """every stream of the plan through ctx.decode_packets, packet by packet -> per stream, per packet the PCM int16 [ret][channels];
    asserts return values and PCM equal to the oracle's"""
    got = [[None] * len(st["packets"]) for st in plan["streams"]]
    for channels, ids in sorted(groups(plan).items()):
        ctx.streams_alloc(len(ids), channels)
        ctx.set_mode(rfc)
        try:
            for f in range(len(plan["streams"][ids[0]]["packets"])):
                pcm, res = ctx.decode_packets(np.arange(len(ids)), [plan["streams"][i]["packets"][f] for i in ids], frame_capacity=3)
                for k, i in enumerate(ids):
                    want = dec[i][f]
                    assert res[k] == want["ret"], (plan["name"], "return value", i, f, int(res[k]), want["ret"])
                    assert (pcm[k, :want["ret"]] == want["pcm"]).all(), (plan["name"], "PCM differs from the oracle", i, f)
                    got[i][f] = pcm[k, :want["ret"]].copy()
        finally:
            ctx.set_mode(False)
    return got


def main():
    import conftest
    import oracle_py
    import celt_model_plans as P
    from test_celt_model import run, tol_pcm, worst

    assert os.environ.get("OPUSGPU_SPLIT") == "0", "the parent sets OPUSGPU_SPLIT=0: this worker is about k_decode_step"
    pkg = conftest.load_pkg()
    oracle = oracle_py.load()
    ctx = pkg.Context(0)
    try:
        for name, least in (("ref_switch", 16), ("ref_celt", 90)):
            plan, dec, mod, _, _ = run(oracle, name)
            got = through_decode_packets(ctx, plan, dec, False)
            res = P.compare(plan, dec, mod, pcm_of=got)
            w = worst(res["pcm"], tol_pcm)
            print(name, "k_decode_step CELT-only PCM: worst error / TOL_PCM", w, "over", len(res["pcm"]), "frames")
            assert len(res["pcm"]) >= least and w <= 1.0, (name, w, len(res["pcm"]))
    finally:
        ctx.close()
    print("celt model worker ok")


if __name__ == "__main__":
    main()
