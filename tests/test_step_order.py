"""The decode-step scheduler (csrc/og_step.hpp) on the CPU: its ordering rules, and its trace against the recorded one.

tests/emul/og_step_test.cpp compiles the scheduler against a recording double of the HIP runtime and of the launch wrappers; every
call becomes one trace line.  From a trace this test computes what happens before what -- same stream and earlier, record -> wait,
or a host synchronise -- and checks the rules the scheduler's comments state (each check names its comment).  It also compares the
traces with tests/golden/step_traces/*.txt, recorded from the scheduler as it was before it was restructured (one function, with
only the launch wrappers in place): which kernel, with which records, on which stream, behind which event.

What this cannot see is what only tests/test_gpu_stream_hazards.py sees: real overlap, and what the kernels themselves read and write.

og_debug() reads the environment once per process, so every set of switches runs in a child process: `python test_step_order.py
NAME` prints the traces of all scenarios under the switches of variant NAME.
"""
import ctypes
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "emul", "libog_step_test.so")
GOLDEN = os.path.join(HERE, "golden", "step_traces")
KEEPS = 8  # OPUSGPU_STEP_KEEPS_MODE
SETS = 3  # OG_SILK_SETS
N = 8192  # (two halves of OG_HALVES_MIN frames)

VARIANTS = {  # the defaults, and each "aside" / A-B switch off
    "default": {},
    "recon_aside0": {"OPUSGPU_HYBRID_RECON_ASIDE": "0"},
    "recon_aside2": {"OPUSGPU_HYBRID_RECON_ASIDE": "2"},
    "params_aside0": {"OPUSGPU_SILK_PARAMS_ASIDE": "0"},
    "parse_wide0": {"OPUSGPU_PARSE_WIDE": "0"},
    "halves0": {"OPUSGPU_HALVES": "0"},
    "fast_recon0": {"OPUSGPU_FAST_RECON": "0"},
    "split_hybrid0": {"OPUSGPU_SPLIT_HYBRID": "0"},
    "split0": {"OPUSGPU_SPLIT": "0"},
    "stall_recon": {"OPUSGPU_STALL_STREAM": "recon", "OPUSGPU_STALL_US": "100"},
}


def S(n, modes, stream=0, window=0, flags=0):
    return (n, modes, stream, window, flags)


# name -> (pipeline, rfc, steps, fail_step)
SCENARIOS = {
    "celt_pipe": (1, 0, [S(N, 7)] + [S(N - 64 * k, 4) for k in range(8)], -1),
    "celt_window": (1, 0, [S(N, 7), S(N, 4, window=7)] + [S(N - 512 * k, 4) for k in range(1, 7)] + [S(N, 4)], -1),
    "celt_window_fail": (1, 0, [S(N, 4, window=6)] + [S(N + 4096 * k, 4) for k in range(1, 6)], 3),
    "silk_pipe": (1, 0, [S(N - 64 * k, 1) for k in range(8)], -1),
    "hybrid_pipe": (1, 0, [S(N - 64 * k, 2) for k in range(8)], -1),
    "silk_hybrid_mix": (1, 0, [S(N, m) for m in (1, 2, 3, 2, 1, 2, 2, 3, 1)], -1),
    "keeps_mix": (1, 0, [S(N, 7 | KEEPS) for _ in range(7)], -1),
    # (the first three steps grow every set of SILK records, which drains by itself: the kind changes come behind them)
    "kinds": (1, 0, [S(N, 2)] * 3 + [S(N, m) for m in (4, 4, 2, 2, 7, 2, 4, 7, 4, 1, 1, 7, 7, 4)], -1),
    "kinds_keeps": (1, 0, [S(N, 2 | KEEPS)] * 3 + [S(N, m | KEEPS) for m in (4, 4, 2, 2, 4, 7, 7, 4, 2, 1, 4)] + [S(N, 7), S(N, 2 | KEEPS), S(N, 4 | KEEPS)], -1),
    "halves": (0, 0, [S(N, 7), S(N, 3), S(N, 4), S(N, 1), S(1000, 7), S(N + 100, 2), S(N, 7)], -1),
    "halves_pipeline_on": (1, 0, [S(N, 7), S(N, 7), S(N, 4), S(N, 7), S(N, 3, flags=1), S(N, 4, flags=1), S(N, 7)], -1),
    "slices": (1, 0, [S(N, 7, flags=3), S(N, 4, flags=3), S(N, 1, flags=3), S(N, 4), S(N, 7, flags=3)], -1),
    "stream_change_silk": (1, 0, [S(N, 2, s) for s in (0, 0, 0, 0, 1, 1, 1, 2, 0, 0)], -1),
    "stream_change_celt": (1, 0, [S(N, 4, s) for s in (1, 1, 1, 1, 2, 2, 2, 0, 0, 1)], -1),
    "rfc": (1, 1, [S(N, 7), S(N, 4), S(N, 7, 1)], -1),
    # short ones, every flow once or twice: their traces are the recorded ones (GOLDEN_OF; the stream changes behind the steps that
    # grow the sets of SILK records, as in "kinds")
    "g_celt": (1, 0, [S(N, 7), S(N, 4), S(N, 4), S(N, 4, window=4), S(N - 512, 4), S(N, 4), S(N - 64, 4)], -1),
    "g_window_fail": (1, 0, [S(N, 4, window=4), S(2 * N, 4), S(3 * N, 4), S(N, 4)], 2),
    "g_silk": (1, 0, [S(N, m) for m in (1, 2, 3, 2, 2)], -1),
    "g_kinds": (1, 0, [S(N, m) for m in (2 | KEEPS, 4 | KEEPS, 7 | KEEPS, 4, 2, 7)], -1),
    "g_in_order": (0, 0, [S(N, 7), S(N, 4), S(1000, 3), S(N, 7, flags=3)], -1),
    "g_stream_change": (1, 0, [S(N, 2, s) for s in (0, 0, 0, 1, 1)] + [S(N, 4, s) for s in (1, 2, 2)], -1),
    "g_rfc": (1, 1, [S(N, 7), S(N, 4, 1)], -1),
}
# variant -> the scenarios whose traces are recorded for it: all short ones at the defaults, and for a switch those it bears on
GOLDEN_OF = {
    "default": ["g_celt", "g_window_fail", "g_silk", "g_kinds", "g_in_order", "g_stream_change", "g_rfc"],
    "recon_aside0": ["g_silk"], "params_aside0": ["g_silk"], "split_hybrid0": ["g_silk"],
    "parse_wide0": ["g_celt"], "fast_recon0": ["g_celt"], "halves0": ["g_in_order"], "split0": ["g_in_order"],
}


def run_scenario(lib, name):
    pipeline, rfc, steps, fail = SCENARIOS[name]
    cols = [(ctypes.c_int * len(steps))(*[s[i] for s in steps]) for i in range(5)]
    lib.og_step_test_run.restype = ctypes.c_char_p
    return lib.og_step_test_run(pipeline, rfc, len(steps), *cols, fail).decode()


def traces_of(variant):
    """{scenario: [trace lines]} under the switches of `variant`, from a child process."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("OPUSGPU_")}
    env.update(VARIANTS[variant])
    out = subprocess.run([sys.executable, os.path.abspath(__file__), variant], env=env, check=True, capture_output=True, text=True).stdout
    traces, cur = {}, None
    for line in out.splitlines():
        if line.startswith("== "):
            cur = traces.setdefault(line[3:], [])
        elif line:
            cur.append(line)
    return traces


_cache = {}


def traces(variant):
    if variant not in _cache:
        _cache[variant] = traces_of(variant)
    return _cache[variant]


# ---- happens-before ---------------------------------------------------------------------------------------------------
class Trace:
    """launches: dicts (id, kernel, stream, step, f0, f1, grid, args, line); hb[id]: bit set of the launches that happen before it."""

    def __init__(self, lines):
        self.lines, self.launches, self.hb = lines, [], []
        self.waitvalues = []  # (line number, counter, target, stream, step of the last launch before it)
        self.writevalues = []
        self.stale_waits = []  # waits for an event whose record lies before a host drain (or that was never recorded)
        front, events, host, recorded_at, last_drain = {}, {}, 0, {}, -1
        run = set()  # streams of the current run of consecutive host synchronisations
        for ln, line in enumerate(lines):
            w = line.split()
            if w[0] == "sync":
                host |= front.get(w[1], 0)
                run.add(w[1])
                continue
            if {"parse", "recon"} <= run and w[0] != "grow":  # (in front of a grow: the buffers' users are waited for, nothing is forgotten)
                last_drain = ln - 1
            run = set()
            if w[0] in ("launch", "record", "wait", "waitvalue", "writevalue"):
                q = [x for x in w if x.startswith("stream=")][0][7:]
                front[q] = front.get(q, 0) | host  # (the host has waited for these before it queued this)
            if w[0] == "launch":
                kv = dict(x.split("=", 1) for x in w[2:] if "=" in x)
                f0, f1 = map(int, re.match(r"\[(\d+),(\d+)\)", kv["frames"]).groups())
                i = len(self.launches)
                self.launches.append(dict(id=i, kernel=w[1], stream=q, step=int(kv["step"]), f0=f0, f1=f1, grid=int(kv["grid"]), args=kv, line=ln))
                self.hb.append(front[q])
                front[q] |= 1 << i
            elif w[0] == "record":
                events[w[1]] = front[q]
                recorded_at[w[1]] = ln
            elif w[0] == "wait":
                if recorded_at.get(w[1], -1) <= last_drain:
                    self.stale_waits.append((ln, line))
                front[q] |= events.get(w[1], 0)
            elif w[0] == "waitvalue":
                c, v = w[1].split(">=")
                self.waitvalues.append((ln, c, int(v), q, self.launches[-1]["step"]))
            elif w[0] == "writevalue":
                c, v = w[1].split("=")
                self.writevalues.append((c, int(v)))

    def of(self, step, kernel=None, **args):
        return [l for l in self.launches if l["step"] == step and l["kernel"] != "k_stream_stall" and (kernel is None or re.fullmatch(kernel, l["kernel"]))
                and all(l["args"].get(k) == str(v) for k, v in args.items())]

    def steps(self):
        return sorted({l["step"] for l in self.launches})

    def before(self, a, b):
        return bool(self.hb[b["id"]] >> a["id"] & 1)

    def all_before(self, As, Bs, what):
        assert As and Bs, f"{what}: launches missing ({len(As)}, {len(Bs)})"
        for a in As:
            for b in Bs:
                assert self.before(a, b), f"{what}: nothing orders\n  {self.lines[a['line']]}\nbefore\n  {self.lines[b['line']]}"


def normalised(lines):
    """Runs of consecutive host synchronisations carry no order and no count: sorted, each stream once."""
    out, run = [], []
    for line in list(lines) + [""]:
        if line.startswith("sync "):
            run.append(line)
            continue
        out += sorted(set(run))
        run = []
        out.append(line)
    return out[:-1]


# ---- a. the rules -----------------------------------------------------------------------------------------------------
CELT_VARIANTS = ["default", "parse_wide0", "fast_recon0", "stall_recon"]
SILK_VARIANTS = ["default", "recon_aside0", "recon_aside2", "params_aside0", "parse_wide0", "fast_recon0", "stall_recon"]


def check_pipelined_celt(t, first_pipelined):
    """og_step.hpp, step_pipelined_celt: "The kernels of a step and what orders them" -- parse_stream [the last in-order step, post of
    step k-3], recon_stream [the parse, post of step k-2], step's stream [reconstruction of step k]."""
    steps = [k for k in t.steps() if k >= first_pipelined]
    assert len(steps) >= 6
    for k in steps:
        parse, recon, post = t.of(k, "k_celt_parse(64)?", early=1), t.of(k, "k_celt_recon(_fb)?"), t.of(k, "k_celt_post")
        assert len(parse) == 1 and len(post) == 1 and recon
        if k - 3 >= first_pipelined:
            t.all_before(t.of(k - 3, "k_celt_post"), parse, f"step {k}: parse behind its slot's last reader, post of step {k - 3}")
            assert parse[0]["args"]["recs"] == t.of(k - 3, "k_celt_post")[0]["args"]["recs"]
        for j in range(first_pipelined):
            t.all_before(t.of(j), parse, f"step {k}: parse behind the in-order step {j} (ev_front)")
        t.all_before(parse, recon, f"step {k}: reconstruction behind its parse")
        if k - 2 >= first_pipelined:
            t.all_before(t.of(k - 2, "k_celt_post"), recon, f"step {k}: reconstruction behind post of step {k - 2} (the ring: 2 x 960 of 2048)")
        t.all_before(recon, post, f"step {k}: post behind its reconstruction")
        for a, b in ((k - 1, k), (k - 2, k)):  # three sets of records: neighbours never share one
            if a >= first_pipelined:
                assert t.of(a, "k_celt_post")[0]["args"]["recs"] != post[0]["args"]["recs"]


@pytest.mark.parametrize("variant", CELT_VARIANTS)
def test_pipelined_celt_steps(variant):
    check_pipelined_celt(Trace(traces(variant)["celt_pipe"]), 1)
    check_pipelined_celt(Trace(traces(variant)["celt_window"]), 1)


@pytest.mark.parametrize("variant", ["default", "parse_wide0"])
def test_window_waits_for_the_next_steps_workgroups(variant):
    """og_step.hpp, PLACEMENT: in a window the reconstruction of step k waits until every workgroup of the parse of step k+1 has
    started, its post until the first round (at most 32 counted) of the reconstruction of step k+1 has."""
    t = Trace(traces(variant)["celt_window"])
    seen = 0
    for ln, counter, target, stream, k in t.waitvalues:
        if counter == "parse":
            nxt = t.of(k + 1, "k_celt_parse(64)?", early=1)[0]
            assert stream == "recon" and target == int(nxt["args"]["started"]), (ln, target, nxt)
        else:
            before, add = map(int, t.of(k + 1, "k_celt_recon_fb")[0]["args"]["started"].split("+"))
            assert stream == "ctx" and target == before + min(add, 32), (ln, target, before, add)
        seen += 1
    assert seen == 2 * 6  # steps 1 .. 6 of the window of 7; its last step and the single step behind it wait for no count


def test_window_error_releases_the_last_queued_steps_waits():
    """og_step.hpp, release_window_waits: "the placement waits of the last step queued ... are let go by writing the counts they
    wait for"."""
    t = Trace(traces("default")["celt_window_fail"])
    assert "rc %d" % -6 in t.lines or any(l.startswith("rc ") and l != "rc 0" for l in t.lines)
    last = {c: v for _, c, v, _, _ in t.waitvalues}  # the targets of the last step that queued its waits
    assert sorted(t.writevalues) == sorted(last.items()) and len(last) == 2
    assert t.lines.count("memset started") == 1 and t.lines.index("memset started") > max(i for i, l in enumerate(t.lines) if l.startswith("writevalue"))


def last_kernel(t, k):
    return [t.of(k)[-1]]


def check_pipelined_silk(t, steps, modes_of, keeps):
    """og_step.hpp, step_pipelined_silk: "PIPELINED SILK / HYBRID STEPS" and back_half's comment on `rq` (the history ring)."""
    assert len(steps) >= 6
    for k in steps:
        sparse, params, synth = t.of(k, "k_silk_parse64"), t.of(k, "k_silk_params"), t.of(k, "k_silk_synth(_nb)?")
        assert len(sparse) == 1 and len(params) == 1 and synth and sparse[0]["stream"] == "parse"
        if k - SETS in steps:
            t.all_before(t.of(k - SETS), sparse, f"step {k}: SILK parse behind the last kernel of step {k - SETS} (its set's last reader)")
            assert sparse[0]["args"]["silk"] == t.of(k - SETS, "k_silk_parse64")[0]["args"]["silk"]
        t.all_before(sparse, params, f"step {k}: parameters behind the SILK parse")
        t.all_before(sparse + params, synth, f"step {k}: synthesis behind parse and parameters")
        post = t.of(k, "k_celt_post")
        if modes_of(k) & 6:
            cparse, recon = t.of(k, "k_celt_parse(64)?"), t.of(k, "k_celt_recon(_fb)?")
            t.all_before(cparse, recon, f"step {k}: CELT reconstruction behind the CELT parse")
            if k - 2 in steps:
                t.all_before(last_kernel(t, k - 2), recon, f"step {k}: CELT reconstruction behind the last kernel of step {k - 2} (the history ring)")
            t.all_before(recon + synth, post, f"step {k}: post behind reconstruction and synthesis")
        if not keeps and modes_of(k) & 2 and k - 1 in steps and modes_of(k - 1) & 1:
            t.all_before(last_kernel(t, k - 1), sparse, f"step {k}: a hybrid step does not run ahead of step {k - 1}, which may have held SILK-only frames")
        for a in (k - 1, k - 2):  # OG_SILK_SETS sets: neighbours never share one
            if a in steps:
                assert t.of(a, "k_silk_parse64")[0]["args"]["silk"] != sparse[0]["args"]["silk"]


@pytest.mark.parametrize("variant", SILK_VARIANTS)
def test_pipelined_silk_and_hybrid_steps(variant):
    tr = traces(variant)
    for name in ("silk_pipe", "hybrid_pipe", "silk_hybrid_mix", "keeps_mix"):
        steps = SCENARIOS[name][2]
        check_pipelined_silk(Trace(tr[name]), list(range(len(steps))), lambda k: steps[k][1] & 7, bool(steps[0][1] & KEEPS))


def test_hybrid_reconstruction_runs_aside_by_default():
    """(the rule above bites: by default the reconstruction of a hybrid step is NOT on the step's stream)"""
    t = Trace(traces("default")["hybrid_pipe"])
    assert {l["stream"] for l in t.of(4, "k_celt_recon(_fb)?")} == {"recon"}
    assert {l["stream"] for l in Trace(traces("recon_aside0")["hybrid_pipe"]).of(4, "k_celt_recon(_fb)?")} == {"ctx"}


@pytest.mark.parametrize("variant", ["default", "fast_recon0", "split_hybrid0", "parse_wide0"])
@pytest.mark.parametrize("name", ["halves", "halves_pipeline_on"])
def test_two_halves_fork_and_join(variant, name):
    """og_step.hpp, step_in_order, TWO HALVES: "the caller's stream forks the second one and joins it"."""
    t = Trace(traces(variant)[name])
    forked = 0
    for k in t.steps():
        second = [l for l in t.of(k) if l["f0"] > 0]
        if not second:
            continue
        forked += 1
        assert {l["stream"] for l in second} == {"recon" if SCENARIOS[name][0] else "side"}
        earlier = [l for j in t.steps() if j < k for l in t.of(j)]
        later = [l for j in t.steps() if j > k for l in t.of(j) if l["stream"] == "ctx"]
        if earlier:
            t.all_before(earlier, second, f"step {k}: second chain forked behind everything earlier")
        if later:
            t.all_before(second, later, f"step {k}: second chain joined before anything later on the step's stream")
    assert forked >= 4


def expected_kind_drains(steps, pipelined_kind):
    """enter_step_kind's rules (og_step.hpp, the comment above it), step by step -> the steps in front of which the host drains."""
    last, last2_celt, out = 0, False, []
    for k, (n, modes, *_rest) in enumerate(steps):
        keeps, m = bool(modes & KEEPS), modes & 7
        kind = pipelined_kind(m, keeps)
        shares = (kind == 1 and last == 2 and last2_celt) or (kind == 2 and bool(m & 4) and last == 1)
        disjoint = keeps and kind != 0 and last != 0 and not shares
        if (kind == 2) != (last == 2) and not disjoint:
            out.append(k)
        last = kind
        if kind == 2:
            last2_celt = bool(m & 4)
    return out


def kind_default(m, keeps):
    return 1 if m == 4 else 2 if (m & 3) and (not (m & 4) or keeps) else 0


@pytest.mark.parametrize("name", ["kinds", "kinds_keeps"])
def test_kind_changes_drain_where_the_rules_say(name):
    steps = SCENARIOS[name][2]
    lines = traces("default")[name]
    t = Trace(lines)
    drains = []
    for k in range(3, len(steps)):  # (the first three steps grow the sets, which drains too)
        a, b = lines.index(next(l for l in lines if l.startswith(f"step {k} "))), t.of(k)[0]["line"]
        syncs = {l.split()[1] for l in lines[a:b] if l.startswith("sync ")}
        assert syncs in (set(), {"parse", "recon", "ctx"}), (k, syncs)
        if syncs:
            drains.append(k)
    assert drains == [k for k in expected_kind_drains(steps, kind_default) if k >= 3] and len(drains) >= 3
    assert not t.stale_waits, t.stale_waits


@pytest.mark.parametrize("name", ["stream_change_silk", "stream_change_celt"])
def test_stream_change_drains_and_forgets(name):
    """og_step.hpp, decode_step_impl: "consecutive steps on different streams: nothing orders them but the caller, so nothing may run
    ahead either" -- and no later step waits for an event recorded before that drain."""
    steps = SCENARIOS[name][2]
    lines = traces("default")[name]
    t = Trace(lines)
    for k in range(1, len(steps)):
        a, b = lines.index(next(l for l in lines if l.startswith(f"step {k} "))), t.of(k)[0]["line"]
        syncs = {l.split()[1] for l in lines[a:b] if l.startswith("sync ")}
        if steps[k][2] != steps[k - 1][2]:
            prev = "user%d" % steps[k - 1][2] if steps[k - 1][2] else "ctx"
            assert {"parse", "recon", prev} <= syncs, (k, syncs)
            t.all_before([l for j in range(k) for l in t.of(j)], t.of(k), f"step {k} on another stream: behind everything before it")
        elif k >= 4 and steps[k][2] == steps[k - 2][2] and name == "stream_change_celt":
            assert not syncs, (k, syncs)
    assert not t.stale_waits, t.stale_waits


# ---- b. the recorded traces -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(GOLDEN_OF))
def test_traces_equal_the_recorded_ones(variant):
    """One difference from the recorded behaviour is meant: the drain in front of a step on another stream now forgets the SILK
    steps' events too (StepPipeline::drained), so later steps no longer wait for events that completed before that drain.  Those
    lines -- `wait sdoneN` behind such a drain, stale by the rule of Trace -- are taken out of the recorded trace; nothing else is."""
    got = traces(variant)
    with open(os.path.join(GOLDEN, variant + ".txt")) as f:
        want, cur = {}, None
        for line in f.read().splitlines():
            if line.startswith("== "):
                cur = want.setdefault(line[3:], [])
            elif line:
                cur.append(line)
    assert sorted(want) == sorted(GOLDEN_OF[variant])
    for name in GOLDEN_OF[variant]:
        stale = {ln for ln, line in Trace(want[name]).stale_waits if re.match(r"wait sdone\d ", line)}
        if name != "g_stream_change":
            assert not stale, (name, stale)
        recorded = [l for i, l in enumerate(want[name]) if i not in stale]
        assert normalised(got[name]) == normalised(recorded), f"{variant} / {name}: the trace differs from the recorded one"


if __name__ == "__main__":
    lib = ctypes.CDLL(LIB)
    for name in SCENARIOS:
        print("== " + name)
        print(run_scenario(lib, name))
