"""Cross-step ordering of the pipelined decode flows, made deterministic.

A pipelined step puts its kernels on three streams (the caller's, the library's parse_stream and recon_stream; in-order steps cut
in two use a side stream), and consecutive steps overlap.  A missing event between two of them -- one step's kernel overwriting
state that a kernel of an earlier step has not read yet -- shows only when the streams drift apart, which at the sizes of the
other tests they seldom do.  Here OPUSGPU_STALL_STREAM / OPUSGPU_STALL_US (og_debug.hpp) put a stall kernel in front of every
kernel a step launches on one stream, so that stream falls behind the others by whole steps and every ordering the library
relies on must be carried by an event.  One child process per setting (the switches are read once per process), each with a
timeout: no stall, and a stall on each of the four streams.  Each child (stream_hazard_worker.py) queues 8 steps of every
pipelined flow -- declared CELT-only, SILK-only, hybrid-only and SILK + hybrid steps, one call per step and as a window, half of
them header-ordered as bench.py orders them; OPUSGPU_STEP_KEEPS_MODE steps; undeclared mode walks; in-order steps cut into
halves -- and compares every sample and return code with the oracle.

The stall length: with no stall the steps of these runs took 0.6 - 4.3 ms each at 2,048 streams and 4.8 - 9.1 ms at 8,192 (the
halves; the slower on a fresh context), measured on MI355X (the worker prints its times per step), so a stream held 20 ms in front
of each of its kernels falls behind the others by more than two steps of their work at every step -- farther than the rings and
record sets of the library reach back.  (Without the ordering of the CELT reconstruction beside the SILK synthesis behind step k - 2, the hybrid-only runs differ
from the oracle in more than half of their streams under a stall of the step's stream.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

STALL_US = 20000


@pytest.mark.parametrize("stall", [None, "step", "parse", "recon", "side"])
def test_pipelined_flows_with_a_stalled_stream(stall):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_hazard_worker.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("OPUSGPU_STALL_")}
    if stall:
        env.update(OPUSGPU_STALL_STREAM=stall, OPUSGPU_STALL_US=str(STALL_US))
    out = subprocess.run([sys.executable, worker], env=env, capture_output=True, text=True, timeout=300)
    fails = [line for line in out.stdout.splitlines() if line.startswith("FAIL")]
    assert out.returncode == 0 and not fails, f"stall on {stall or 'no stream'}:\n" + "\n".join(fails or [out.stdout[-2000:], out.stderr[-3000:]])
