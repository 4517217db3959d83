"""The packed-word forms of the 20 ms reconstruction kernel (og_celt_packed.hpp: the interleave gather by rows, Haar steps and the
stereo merge on packed words, ring and tail writes in 16-byte pieces -- what k_celt_recon_fb runs) against the general forms (what
the host emulation runs), word for word.  Driver tests/emul/og_tf_undo_packed_test.cpp, built here with g++ under ASan + UBSan; no GPU.

The classes of job -- (log2 of the interleave stride, Hadamard ordering, the three Haar step codes) with the band widths each can
have -- are derived HERE, from the oracle's tf_select_table and the rules of quant_band (celt.cpp:1548-1580) that pm_setup_jobs
follows, not copied from the kernel; the driver gets them on its command line.  For 20 ms frames the derivation gives:
  long blocks       stride 4 ordered with steps (2, 1); stride 8 ordered with steps (3, 2, 1)
  transient frames  no interleave with steps (1, 2, 3); stride 8 with step (1); stride 8 with no step; stride 16 with the step over
                    pairs of groups (code 4; its gather stays on the general path)
Two classes no 20 ms frame has are run as well, because the gather has a form for them: stride 2, ordered and not.

The driver runs every class on every band width that can have it (8, 16, 32, 48, 64, 96, 144, 176 between them), on random and
on extreme spectra (+-32767, -32768), then mixed frames; the stereo merge with its copy mode and inversion; the gather's alignment
claim over the band table; the ring pieces for every ring head that is a multiple of 8 and every frame size.  The bar is equality.
tests/test_gpu_tf_undo_packed.py runs the device forms themselves and shares the derivation."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "esp32-opus-player_amd", "csrc")
NO_CHANGE = (0, 0, (0, 0, 0))
EXTRA = {(1, 1, (1, 0, 0)): None, (1, 0, (0, 0, 0)): None}  # stride 2: every width


def tf_table():
    """tf_select_table of the oracle: [LM][4 * transient + 2 * tf_select + flag]"""
    text = open(os.path.join(ROOT, "oracle", "oc_celt.c")).read()
    body = re.search(r"tf_select_table\[4\]\[8\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    rows = [[int(v) for v in re.findall(r"-?\d+", r)] for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 4 and all(len(r) == 8 for r in rows)
    return rows


def band_widths(LM=3):
    import rc_craft
    eb = rc_craft.rom("rom_eband")
    return [(eb[i + 1] - eb[i]) << LM for i in range(21)]


def job_class(tf_change, N, B):
    """quant_band's time-frequency bookkeeping for a band of N coefficients in B blocks -> (ls, had, (s0, s1, s2)): the interleave's
    log2 stride (0: none), whether its rows are in Hadamard order, the Haar steps on the way back (0 none, else log2(stride) + 1)"""
    logBf = B.bit_length() - 1
    recombine, time_divide = max(tf_change, 0), 0
    logB, N_B = logBf - recombine, (N >> logBf) << recombine
    while N_B % 2 == 0 and tf_change < 0:
        logB, N_B, time_divide, tf_change = logB + 1, N_B >> 1, time_divide + 1, tf_change + 1
    ls = logB + recombine if logB > 0 else 0
    had = int(logB > 0 and B == 1)
    steps = [logB - 1 - k + 1 for k in range(time_divide)] + [k + 1 for k in range(recombine)]
    assert len(steps) <= 3
    return ls, had, tuple(steps + [0] * (3 - len(steps)))


def classes(LM=3):
    """class -> sorted band widths that can have it, over both kinds of frame and every tf_change the table gives them"""
    out = {}
    for transient in (0, 1):
        B = (1 << LM) if transient else 1
        for tf_change in tf_table()[LM][4 * transient:4 * transient + 4]:
            for N in set(band_widths(LM)):
                c = job_class(tf_change, N, B)
                if c != NO_CHANGE:
                    out.setdefault(c, set()).add(N)
    return {c: sorted(w) for c, w in out.items()}


def test_the_derived_classes():
    got = classes()
    print(got)
    assert set(got) == {(2, 1, (2, 1, 0)), (3, 1, (3, 2, 1)), (0, 0, (1, 2, 3)), (3, 0, (1, 0, 0)), (3, 0, (0, 0, 0)), (4, 0, (4, 0, 0))}
    assert sorted(set(band_widths())) == [8, 16, 32, 48, 64, 96, 144, 176]
    every = sorted(set(band_widths()))
    for c, w in got.items():  # stride 16 needs an even number of groups of 8; a stride-8 band left undivided an odd one, or tf_change 0
        assert w == ([n for n in every if n % 16 == 0] if c[0] == 4 else every), (c, w)


def test_packed_forms_equal_the_general_forms(tmp_path):
    exe = str(tmp_path / "og_tf_undo_packed_test")
    flags = open(os.path.join(CSRC, "BUILD_FLAGS")).read().split()
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wno-pedantic", "-Wno-attributes", *flags, "-I", CSRC,
                           os.path.join(EMUL_DIR, "og_tf_undo_packed_test.cpp"), "-o", exe])
    every = sorted(set(band_widths()))
    cl = dict(classes())
    cl.update({c: every for c in EXTRA})
    args = ["%d,%d,%d,%d,%d:%s" % (c[0], c[1], *c[2], "/".join(map(str, w))) for c, w in sorted(cl.items())]
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    m = dict(re.findall(r"(\w+) (\d+)", r.stdout.strip().split("\n")[-1]))
    m = {k: int(v) for k, v in m.items()}
    assert m["fails"] == 0
    assert m["classes"] == len(cl) == 8
    assert m["class_widths"] == sum(len(w) for w in cl.values())  # every class on every width it can have
    assert m["tf_words"] == len(cl) * 6 * 960 and m["mixed_words"] == 48 * 960 and m["merge_words"] == 64 * 960
    assert m["plain_groups"] > 0 and m["copy_groups"] > 0 and m["inv_groups"] > 0
    assert m["reads"] == 2 * 100 * (2 + 4 + 8)       # (band, channel, group) x rows of stride 2, 4, 8
    assert m["pieces"] == 256 * (30 + 60 + 120 + 240)  # ring heads x pieces of the four frame sizes
