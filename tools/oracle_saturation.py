#!/usr/bin/env python3
"""How often does each call of a saturating helper of oracle/oc_math.h clamp, per call site?  CPU only.

gcov (tools/oracle_branches.py) sees sat16, satsym, add_sat32, sub_sat32, lshift_sat32 and limit32 once each, under the header:
one counter per helper, none per call.  This tool counts per call site.  It builds the oracle into a temporary directory (never
into oracle/; oracle/Makefile is not used) from wrapper translation units: oc_math.h, then macros that put a counting wrapper
in front of the six helpers, then the .c file.  A wrapper sees the arguments, so it knows whether the call clamps and on which
side; the helper itself is called unchanged, so the build decodes what the oracle decodes.  A site is keyed by

    file | function | stripped source text of the line [@n for the n-th line with that text in the function] | helper

Line numbers are not part of a key: they move.  Two calls of the same helper on one line share a key (oc_silk.c cng: the two
sat16 of the comfort-noise mix).  "high" is a clamp at the upper bound, "low" at the lower one.

    python tools/oracle_saturation.py --baseline           # the random payload families of tools/oracle_branches.py
    python tools/oracle_saturation.py --corpus [--entry N] # tests/golden/saturation_paths.json: the claimed sites; fails unless each
                                                           # clamps on both sides (but for sides the fixture records as unreachable
                                                           # or open); one entry alone: fails unless it clamps exactly what it claims
    python tools/oracle_saturation.py --json FILE          # [{"channels": c, "packets": [hex, ...], "rfc": bool}, ...]
    ... --rfc                                              # RFC mode for every sequence; an empty packet ("") is a lost one
    ... --positions                                        # every clamp: sequence, packet, ordinal of the call among the
                                                           # site's calls within that packet, side

The positions report is what tests/golden/make_saturation_paths.py and tests/test_saturation_paths.py read to say WHERE in a
frame a clamp fell: the n-th call of the synthesis update within a packet is sample n of the coded channel's frame.
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_branches as ob  # noqa: E402

ORACLE = ob.ORACLE
FIXTURE = os.path.join(ROOT, "tests", "golden", "saturation_paths.json")
HELPERS = ["sat16", "satsym", "add_sat32", "sub_sat32", "lshift_sat32", "limit32"]
SITE_FILES = ["oc_silk.c", "oc_celt.c", "oc_celt_math.c", "oc_packet.c"]  # the files whose sites the fixture gives a verdict on
CFLAGS = ["-O1", "-fPIC", "-fwrapv", "-fno-strict-aliasing", "-w"]
MAX_SITES, MAX_POS = 128, 1 << 22

CENSUS_H = r"""
/* counting wrappers for the saturating helpers of oc_math.h; included behind it, in front of an oracle .c file */
#ifndef OC_SAT_CENSUS_H
#define OC_SAT_CENSUS_H
int oc_sat_site(const char *file, int line, const char *func, int helper);
void oc_sat_clamp(int id, int side);
extern long long oc_sat_calls[], oc_sat_ord[];
extern int oc_sat_wrap_id; /* the site whose add / subtraction / shift WRAPS instead of saturating (--wrap), or -1 */
#define CS_ID(h) __extension__({ static int cs_id_ = -1; if (cs_id_ < 0) cs_id_ = oc_sat_site(__FILE__, __LINE__, __func__, h); cs_id_; })
static inline void cs_note(int id, int side) { oc_sat_calls[id]++; if (side) oc_sat_clamp(id, side); oc_sat_ord[id]++; }
static inline i16 cs_sat16(int id, i32 x) { cs_note(id, x > 32767 ? 1 : x < -32768 ? 2 : 0); return sat16(x); }
static inline i32 cs_satsym(int id, i32 x, i32 a) { cs_note(id, x > a ? 1 : x < -a ? 2 : 0); return satsym(x, a); }
static inline i32 cs_add_sat32(int id, i32 a, i32 b) { i64 s = (i64)a + b; cs_note(id, s > INT32_MAX ? 1 : s < INT32_MIN ? 2 : 0); return id == oc_sat_wrap_id ? addw(a, b) : add_sat32(a, b); }
static inline i32 cs_sub_sat32(int id, i32 a, i32 b) { i64 s = (i64)a - b; cs_note(id, s > INT32_MAX ? 1 : s < INT32_MIN ? 2 : 0); return id == oc_sat_wrap_id ? subw(a, b) : sub_sat32(a, b); }
static inline i32 cs_lshift_sat32(int id, i32 a, int s) { cs_note(id, a > (INT32_MAX >> s) ? 1 : a < (INT32_MIN >> s) ? 2 : 0); return id == oc_sat_wrap_id ? shl32(a, s) : lshift_sat32(a, s); }
static inline i32 cs_limit32(int id, i32 a, i32 l1, i32 l2) {
    const i32 hi = l1 > l2 ? l1 : l2, lo = l1 > l2 ? l2 : l1;
    cs_note(id, a > hi ? 1 : a < lo ? 2 : 0);
    return limit32(a, l1, l2);
}
#define sat16(x) cs_sat16(CS_ID(0), x)
#define satsym(x, a) cs_satsym(CS_ID(1), x, a)
#define add_sat32(a, b) cs_add_sat32(CS_ID(2), a, b)
#define sub_sat32(a, b) cs_sub_sat32(CS_ID(3), a, b)
#define lshift_sat32(a, s) cs_lshift_sat32(CS_ID(4), a, s)
#define limit32(a, l1, l2) cs_limit32(CS_ID(5), a, l1, l2)
#endif
"""

CENSUS_C = r"""
#include <stdlib.h>
#include <string.h>
#define MAX_SITES %d
#define MAX_POS %d
struct site { const char *file, *func; int line, helper; };
static struct site sites[MAX_SITES];
static int n_sites;
long long oc_sat_calls[MAX_SITES], oc_sat_ord[MAX_SITES], oc_sat_hi[MAX_SITES], oc_sat_lo[MAX_SITES];
static int pos[MAX_POS][5], n_pos, want_pos, cur_seq, cur_packet;
int oc_sat_wrap_id = -1;
static int wrap_line = -1, wrap_helper = -1;
static char wrap_file[64];
static const char *base_name(const char *p) { const char *b = strrchr(p, '/'); return b ? b + 1 : p; }
void oc_sat_wrap(const char *file, int line, int helper) { /* before the first decode: sites register on their first call */
    strncpy(wrap_file, file, sizeof wrap_file - 1); wrap_line = line; wrap_helper = helper;
}
int oc_sat_site(const char *file, int line, const char *func, int helper) {
    int i;
    for (i = 0; i < n_sites; i++) /* (a static inline function of a header would come once per translation unit) */
        if (sites[i].line == line && sites[i].helper == helper && !strcmp(sites[i].file, file)) return i;
    if (n_sites == MAX_SITES) abort(); /* more call sites than the tables hold: raise MAX_SITES */
    if (line == wrap_line && helper == wrap_helper && !strcmp(base_name(file), wrap_file)) oc_sat_wrap_id = n_sites;
    sites[n_sites].file = file; sites[n_sites].func = func; sites[n_sites].line = line; sites[n_sites].helper = helper;
    return n_sites++;
}
void oc_sat_clamp(int id, int side) {
    if (side == 1) oc_sat_hi[id]++; else oc_sat_lo[id]++;
    if (want_pos && n_pos < MAX_POS && (want_pos == 1 || (side == 1 ? oc_sat_hi[id] : oc_sat_lo[id]) <= 4)) { /* 2: a site's first four a side */
        pos[n_pos][0] = id; pos[n_pos][1] = cur_seq; pos[n_pos][2] = cur_packet; pos[n_pos][3] = (int)oc_sat_ord[id]; pos[n_pos][4] = side;
        n_pos++;
    }
}
void oc_sat_positions(int on) { want_pos = on; }
void oc_sat_begin_packet(int seq, int packet) { cur_seq = seq; cur_packet = packet; memset(oc_sat_ord, 0, sizeof oc_sat_ord); }
int oc_sat_n_sites(void) { return n_sites; }
const char *oc_sat_site_file(int i) { return sites[i].file; }
const char *oc_sat_site_func(int i) { return sites[i].func; }
int oc_sat_site_line(int i) { return sites[i].line; }
int oc_sat_site_helper(int i) { return sites[i].helper; }
int oc_sat_n_pos(void) { return n_pos; }
const int *oc_sat_pos(void) { return &pos[0][0]; }
""" % (MAX_SITES, MAX_POS)

CALL = re.compile(r"\b(%s)\s*\(" % "|".join(HELPERS))
FUNC = re.compile(r"^[A-Za-z_][^;]*?\b(\w+)\s*\([^;]*$")


def static_sites():
    """Every call of a helper in oracle/*.c, called or not -> {(file, line number, helper): key}"""
    out = {}
    for src in ob.ALL_SRCS:
        text = open(os.path.join(ORACLE, src)).read().split("\n")
        fn, seen = "?", {}
        for no, raw in enumerate(text, 1):
            m = FUNC.match(raw)
            if m and not raw.startswith(("static inline", "typedef", "#")) and "=" not in raw.split("(")[0]:
                fn = m.group(1)
            code = raw.split("/*")[0]
            hs = sorted({h for h in CALL.findall(code)})
            if not hs:
                continue
            line = " ".join(raw.split())
            n = seen[(fn, line)] = seen.get((fn, line), 0) + 1
            for h in hs:
                out[(src, no, h)] = f"{src}|{fn}|{line}" + (f"@{n}" if n > 1 else "") + f"|{h}"
    return out


class CensusBuild:
    """The oracle behind the counting wrappers, in a temporary directory of its own."""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="oracle_sat_")
        with open(os.path.join(self.dir, "sat_census.h"), "w") as f:
            f.write(CENSUS_H)
        with open(os.path.join(self.dir, "sat_census.c"), "w") as f:
            f.write(CENSUS_C)
        objs = ["sat_census.o"]
        subprocess.check_call(["gcc", *CFLAGS, "-c", "sat_census.c", "-o", "sat_census.o"], cwd=self.dir)
        for src in ob.ALL_SRCS:
            with open(os.path.join(self.dir, "w_" + src), "w") as f:
                f.write('#include "oc_math.h"\n#include "sat_census.h"\n#include "%s"\n' % os.path.join(ORACLE, src))
            subprocess.check_call(["gcc", *CFLAGS, "-I", ORACLE, "-I", self.dir, "-c", "w_" + src, "-o", src[:-2] + ".o"], cwd=self.dir)
            objs.append(src[:-2] + ".o")
        self.lib = os.path.join(self.dir, "liboc_sat.so")
        subprocess.check_call(["gcc", "-shared", "-o", self.lib] + objs, cwd=self.dir)
        self.keys = static_sites()

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, args, job=None):
        """a child process that loads the build, does its work and prints the census as JSON -> census dict"""
        if job is not None:
            with open(os.path.join(self.dir, "job.json"), "w") as f:
                json.dump(job, f)
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--worker", self.lib] + [str(a) for a in args])
        return self.census(json.loads(out))

    def decode(self, sequences, rfc=False, positions=False, wrap=None):
        """wrap: a site key of add_sat32 / sub_sat32 / lshift_sat32 whose operation WRAPS in this run, as a wrong kernel's would (the
        counts are those of the arguments the wrapped run sees).
        -> {"results": per sequence [[return code, final range, crc32 of the PCM], ...], "sites": {key: [calls, high, low]},
        "positions": {key: [[sequence, packet, ordinal, side], ...]}} (side 1 = high, 2 = low)"""
        args = ["decode", os.path.join(self.dir, "job.json"), int(rfc), int(positions)]
        if wrap is not None:
            (src, line, h), = [site for site, k in self.keys.items() if k == wrap]
            args += [src, line, HELPERS.index(h)]
        return self.run(args, job=sequences)

    def nlsf_corners(self, wb, alphabet, lo, hi):
        """oc_test_nlsf2a (stage-1 index and residuals -> NLSF -> LPC) over vectors lo .. hi - 1 of the enumeration: n = stage-1 index
        * len(alphabet)^order + the residuals as digits of base len(alphabet), the first residual the lowest digit.  Positions: a
        site's first four clamps a side, with the vector's number as the sequence."""
        return self.run(["nlsf", int(wb), ",".join(map(str, alphabet)), int(lo), int(hi)])

    def census(self, raw):
        sites, positions, ids = {}, {}, []
        for file, line, func, helper, calls, hi, lo in raw["sites"]:
            src = os.path.basename(file)
            text = open(os.path.join(ORACLE, src)).read().split("\n")
            h = HELPERS[helper]
            while (src, line, h) not in self.keys and line > 1 and h + "(" not in text[line - 1]:
                line -= 1  # a call that spans lines: the compiler may name its last line, the key is the line with the name
            key = self.keys[(src, line, h)]
            assert key.split("|")[1] == func, (key, func)  # static_sites found the function the compiler names
            ids.append(key)
            c = sites.setdefault(key, [0, 0, 0])
            c[0], c[1], c[2] = c[0] + calls, c[1] + hi, c[2] + lo
        for i, seq, packet, ordinal, side in raw.get("positions", []):
            positions.setdefault(ids[i], []).append([seq, packet, ordinal, side])
        for key in self.keys.values():
            sites.setdefault(key, [0, 0, 0])
        return {"results": raw.get("results"), "sites": sites, "positions": positions, "lines": {k: ln for (_, ln, _), k in self.keys.items()}}


def _census_lib(path):
    lib = C.CDLL(path)
    for f in (lib.oc_sat_site_file, lib.oc_sat_site_func):
        f.restype, f.argtypes = C.c_char_p, [C.c_int]
    lib.oc_sat_pos.restype = C.POINTER(C.c_int)
    return lib


def dump_census(lib, results=None):
    n = lib.oc_sat_n_sites()
    calls, hi, lo = ((C.c_longlong * MAX_SITES).in_dll(lib, nm) for nm in ("oc_sat_calls", "oc_sat_hi", "oc_sat_lo"))
    sites = [[lib.oc_sat_site_file(i).decode(), lib.oc_sat_site_line(i), lib.oc_sat_site_func(i).decode(), lib.oc_sat_site_helper(i),
              calls[i], hi[i], lo[i]] for i in range(n)]
    p, npos = lib.oc_sat_pos(), lib.oc_sat_n_pos()
    json.dump({"results": results, "sites": sites, "positions": [[p[5 * k + j] for j in range(5)] for k in range(npos)]}, sys.stdout)


def worker(lib_path, what, *args):
    import zlib
    lib = _census_lib(lib_path)
    if what == "nlsf":
        wb, alpha, lo, hi = int(args[0]), [int(v) for v in args[1].split(",")], int(args[2]), int(args[3])
        order = 16 if wb else 10
        lib.oc_test_nlsf2a.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
        lib.oc_sat_positions(2)
        a = (C.c_int16 * 16)()
        for n in range(lo, hi):
            s1, rem = divmod(n, len(alpha) ** order)
            res = []
            for _ in range(order):
                rem, d = divmod(rem, len(alpha))
                res.append(alpha[d] & 0xFF)
            lib.oc_sat_begin_packet(n, 0)
            lib.oc_test_nlsf2a(bytes([s1] + res), wb, a)
        return dump_census(lib)
    job, rfc, positions = args[0], int(args[1]), int(args[2])
    if len(args) > 3:
        lib.oc_sat_wrap.argtypes = [C.c_char_p, C.c_int, C.c_int]
        lib.oc_sat_wrap(args[3].encode(), int(args[4]), int(args[5]))
    lib.oc_decoder_create.restype = C.c_void_p
    lib.oc_decoder_create.argtypes = [C.c_int]
    lib.oc_decoder_destroy.argtypes = [C.c_void_p]
    lib.oc_decoder_set_rfc.argtypes = [C.c_void_p, C.c_int]
    lib.oc_decode.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int]
    lib.oc_decoder_final_range.argtypes = [C.c_void_p]
    lib.oc_decoder_final_range.restype = C.c_uint32
    lib.oc_sat_positions(positions)
    res = []
    for n, seq in enumerate(json.load(open(job))):
        ch = seq["channels"]
        d = lib.oc_decoder_create(ch)
        lossy = rfc or seq.get("rfc")
        lib.oc_decoder_set_rfc(d, 1 if lossy else 0)
        buf = C.create_string_buffer((5760 + 960) * ch * 2)
        rows = []
        for k, hx in enumerate(seq["packets"]):
            p = bytes.fromhex(hx)
            lib.oc_sat_begin_packet(n, k)
            if lossy and not p:
                r = lib.oc_decode(d, None, 0, buf, 960)  # a lost packet: 20 ms concealed
            else:
                r = lib.oc_decode(d, p, len(p), buf, 5760)
            rows.append([r, lib.oc_decoder_final_range(d), zlib.crc32(buf.raw[:max(r, 0) * ch * 2])])
        lib.oc_decoder_destroy(d)
        res.append(rows)
    dump_census(lib, res)


def report(cen, only=None):
    print(f"{'line':>5} {'calls':>11} {'high':>9} {'low':>9}  key")
    for key in sorted(cen["sites"], key=lambda k: (k.split("|")[0], cen["lines"][k], k)):
        if only is None or key in only:
            calls, hi, lo = cen["sites"][key]
            print(f"{cen['lines'][key]:5d} {calls:11d} {hi:9d} {lo:9d}  {key}")


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], sys.argv[3], *sys.argv[4:])
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--baseline", action="store_true")
    g.add_argument("--corpus", action="store_true")
    g.add_argument("--json")
    ap.add_argument("--entry", type=int, help="with --corpus: this entry alone")
    ap.add_argument("--rfc", action="store_true", help="decode in RFC mode; an empty packet is a lost one")
    ap.add_argument("--positions", action="store_true", help="list every clamp")
    a = ap.parse_args()
    claimed = None
    if a.baseline:
        seqs = ob.baseline_sequences()
    elif a.json:
        seqs = json.load(open(a.json))
    else:
        fx = json.load(open(FIXTURE))
        ents = fx["entries"] if a.entry is None else [fx["entries"][a.entry]]
        seqs = [{"channels": e["channels"], "packets": e["packets"], "rfc": e["rfc"]} for e in ents]
        claimed = sorted({k for e in ents for k in e["keys"]})
        excused = {(k, side) for k, sides in fx["unreachable"].items() for side in sides}           # argued away in the fixture
        excused |= {(k, side) for k in fx["open"] for side in ("high", "low")}                        # ... or recorded as open
    with CensusBuild() as cb:
        cen = cb.decode(seqs, rfc=a.rfc, positions=a.positions)
    report(cen, claimed)
    if a.positions:
        for key in sorted(cen["positions"]):
            for seq, packet, ordinal, side in cen["positions"][key]:
                print(f"  {'high' if side == 1 else 'low '} sequence {seq} packet {packet} call {ordinal}  {key}")
    if claimed is not None:
        if a.entry is not None:  # one entry: exactly the clamps it claims
            short = [k for k in claimed if cen["sites"][k][1:] != ents[0]["keys"][k]]
            for k in short:
                print(f"CLAIMS {ents[0]['keys'][k]} " + k)
            return 1 if short else 0
        short = [(k, side) for k in claimed for n, side in ((1, "high"), (2, "low")) if not cen["sites"][k][n] and (k, side) not in excused]
        for k, side in short:
            print(f"NOT CLAMPED ON THE {side.upper()} SIDE " + k)
        return 1 if short else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
