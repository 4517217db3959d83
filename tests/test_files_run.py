"""The whole-file decode driver (csrc/og_files_run.hpp) on the CPU: what is uploaded before what, what a failing step leaves
queued, what is freed when, and what the caller's arrays hold afterwards.

tests/emul/og_files_run_test.cpp compiles the driver against a recording double of hipSetDevice / hipMalloc / hipFree / hipMemcpy
and of the operations that opusgpu_files_decode and opusgpu_ms_files_decode supply; every call becomes one trace line.  The batch is
hand-made: 3 files, 3 steps of 3, 2 and 1 slots -- the smallest with a shrinking step and a file that ends early; nothing in the
driver depends on the batch's size.  What the kernels do with the tables is tests/test_gpu_files.py's and test_gpu_ms_files.py's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "emul", "libog_files_run_test.so")
OPUSGPU_ALLOC_FAIL, OPUSGPU_ERR_HIP = -7, -101
SENTINEL = ["out %d length=-77 status=-77 bad_packet=-77" % i for i in range(3)]
PLANNED = ["out 0 length=1000 status=0 bad_packet=-1", "out 1 length=2000 status=-136 bad_packet=-1",
           "out 2 length=3000 status=0 bad_packet=-1"]
SLOTS = (3, 2, 1)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.dirname(LIB), "-s", os.path.basename(LIB)])
    so = C.CDLL(LIB)
    so.og_files_run_test.restype = C.c_char_p
    so.og_files_run_test.argtypes = [C.c_int] * 11
    so.og_files_fold_test.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    so.og_files_fold_test.restype = None
    return so


def run(lib, width=1, extra=1, shape=0, null_tracks=0, fail_malloc=0, fail_memcpy=0, fail_step=-1, fail_code=0, bad=(-1, 0, 0)):
    return lib.og_files_run_test(width, extra, shape, null_tracks, fail_malloc, fail_memcpy, fail_step, fail_code, *bad).decode().splitlines()


def field(line, name):
    return re.search(r"\b%s=(\S+)" % name, line).group(1)


def check_frees(trace):
    """(f) every allocation is freed, once, and nothing else is."""
    got = [ln.split()[1] for ln in trace if ln.startswith("malloc 0x")]
    assert sorted(got) == sorted(ln.split()[1] for ln in trace if ln.startswith("free "))
    assert len(set(got)) == len(got)
    return got


def first(trace, prefix):
    return next(i for i, ln in enumerate(trace) if ln.startswith(prefix))


@pytest.mark.parametrize("width,extra", [(1, 1), (2, 0)], ids=["stereo", "multistream"])
def test_uploads_then_steps_in_order(lib, width, extra):
    t = run(lib, width, extra)
    bufs = check_frees(t)
    assert len(bufs) == (6 if extra else 4)
    # the device buffers are the tables' sizes (+ 16): descriptors, segments, arena, track states, then the extras of the largest step
    sizes = [int(field(ln, "bytes")) for ln in t if ln.startswith("malloc 0x")]
    assert sizes == [6 * width * 16 + 16, 6 * 32 + 16, 48 + 16, 3 * 8 + 16] + ([3 * 1000 + 16, 3 * 4 + 16] if extra else [])
    # (a) the device is chosen first; all four uploads, into the first four buffers in that order, and the reset precede the first step
    assert t[0] == "setdevice 5"
    ups = [ln for ln in t if ln.startswith("memcpy h2d")]
    assert [field(ln, "dst") for ln in ups] == bufs[:4]
    assert [int(field(ln, "bytes")) for ln in ups] == [6 * width * 16, 6 * 32, 48, 24]
    s0 = first(t, "step ")
    assert all(t.index(ln) < s0 for ln in ups) and t.index("reset 3") < s0
    assert max(t.index(ln) for ln in ups) < t.index("reset 3")
    # (b) assemble k directly follows step k; the pointers advance by the preceding slots x width descriptors / segments
    loop = t[t.index("loop_begin") + 1:t.index("loop_end")]
    assert [ln.split()[:2] for ln in loop] == [[w, str(k)] for k in range(3) for w in ("step", "assemble")]
    at = 0
    for k, n in enumerate(SLOTS):
        st, asm = loop[2 * k], loop[2 * k + 1]
        assert int(field(st, "n")) == n and int(field(asm, "n")) == n
        assert int(field(st, "descs"), 16) == int(bufs[0], 16) + at * width * 16
        assert int(field(asm, "segs"), 16) == int(bufs[1], 16) + at * 32
        assert int(field(st, "first_offset")) == 100 * at and int(field(asm, "first_slot")) == at  # (what the uploads put there)
        assert field(st, "arena") == bufs[2] and field(asm, "state") == bufs[3]
        assert field(st, "extra") == field(asm, "extra") == (",".join(bufs[4:]) if extra else "(nil),(nil)")
        at += n
    assert [field(ln, "modes") for ln in loop[::2]] == ["12", "4", "2"]
    # then the drain, the read-back of the states, the frees, and the plan's outcome
    tail = t[t.index("loop_end") + 1:]
    assert tail[0] == "drain" and tail[1].startswith("memcpy d2h") and field(tail[1], "src") == bufs[3]
    assert all(ln.startswith("free ") for ln in tail[2:2 + len(bufs)])
    assert tail[2 + len(bufs):] == ["rc 0"] + PLANNED


def test_empty_step_queues_nothing(lib):
    """(c) a step without slots: neither a step nor an assembly, and the steps behind it find their tables where they are."""
    t = run(lib, shape=2)
    bufs = check_frees(t)
    loop = t[t.index("loop_begin") + 1:t.index("loop_end")]
    assert [ln.split()[:2] for ln in loop] == [[w, str(k)] for k in (0, 2, 3) for w in ("step", "assemble")]
    assert [int(field(ln, "descs"), 16) - int(bufs[0], 16) for ln in loop[::2]] == [0, 3 * 16, 5 * 16]
    assert t[-4:] == ["rc 0"] + PLANNED


def test_failing_step_ends_the_queue_and_still_drains(lib):
    """(d) step 1 fails: its assembly and step 2 are not queued, the drain happens, the step's code comes back, the out arrays are
    untouched (no read-back either)."""
    t = run(lib, fail_step=1, fail_code=-9)
    check_frees(t)
    loop = t[t.index("loop_begin") + 1:t.index("loop_end")]
    assert [ln.split()[:2] for ln in loop] == [["step", "0"], ["assemble", "0"], ["step", "1"]]
    after = t[t.index("loop_end") + 1:]
    assert after[0] == "drain" and not any(ln.startswith(("memcpy", "step", "assemble")) for ln in after)
    assert t[-4:] == ["rc -9"] + SENTINEL


@pytest.mark.parametrize("nth", range(1, 7))
def test_failing_allocation_frees_the_earlier_ones(lib, nth):
    """(e) the n-th hipMalloc fails: every earlier buffer is freed, nothing is uploaded or queued, OPUSGPU_ALLOC_FAIL."""
    t = run(lib, fail_malloc=nth)
    assert len(check_frees(t)) == nth - 1
    assert not any(ln.startswith(("memcpy", "reset", "step", "assemble", "drain", "loop")) for ln in t)
    assert "hip_failed %d hipMalloc(files)" % OPUSGPU_ALLOC_FAIL in t
    assert t[-4:] == ["rc %d" % OPUSGPU_ALLOC_FAIL] + SENTINEL


@pytest.mark.parametrize("nth", range(1, 6))
def test_failing_copy_frees_everything(lib, nth):
    """A failing upload (1 - 4) queues nothing; a failing read-back (5) comes behind the drain.  Either way: OPUSGPU_ERR_HIP, all
    buffers freed, the out arrays untouched."""
    t = run(lib, fail_memcpy=nth)
    assert len(check_frees(t)) == 6
    assert ("drain" in t) == (nth == 5) and ("reset 3" in t) == (nth == 5)
    assert any(ln.startswith("step ") for ln in t) == (nth == 5)
    assert t[-4:] == ["rc %d" % OPUSGPU_ERR_HIP] + SENTINEL


def test_batch_without_slots_touches_no_device_call(lib):
    """(g) no slot at all: no device call and no operation, a null d_tracks is accepted, the plan's lengths and statuses."""
    for null_tracks in (0, 1):
        assert run(lib, shape=1, null_tracks=null_tracks) == ["rc 0"] + PLANNED
    # ... with slots, a null d_tracks is refused before anything is touched
    assert run(lib, null_tracks=1) == ["rc -1"] + SENTINEL


def test_failed_track_in_the_state_records(lib):
    """The state records read back decide the outcome: file 0's first failing packet is 2 (planned start 600), code -18."""
    t = run(lib, bad=(0, 2, -18))
    assert t[-4:] == ["rc 0", "out 0 length=600 status=-18 bad_packet=2"] + PLANNED[1:]


def test_fold_track_outcome_known_answers(lib):
    """(h) written out by hand: file 0 clean (planned 1000 samples, plan status -136), file 1's packets start at 0, 480, 960."""
    def fold(first_bad, code, which=3):
        lengths, status = np.full(2, -77, np.int64), np.full(4, -77, np.int32)
        lib.og_files_fold_test(first_bad, code, which, lengths.ctypes.data, status.ctypes.data)
        return lengths.tolist(), status.tolist()

    assert fold(2**31 - 1, 0) == ([1000, 1440], [-136, -1, 0, -1])  # clean: the plan's track_samples and status, -1
    assert fold(1, -4) == ([1000, 480], [-136, -1, -4, 1])          # first_bad 1, code -4: packet_start[1], -4, 1
    assert fold(0, -18) == ([1000, 0], [-136, -1, -18, 0])
    # null out pointers are tolerated, each on its own
    assert fold(1, -4, which=1) == ([1000, 480], [-77] * 4)
    assert fold(1, -4, which=2) == ([-77, -77], [-136, -1, -4, 1])
    assert fold(1, -4, which=0) == ([-77, -77], [-77] * 4)
