"""How many of the reconstruction's waves a CU holds while the 64-frame parse kernel is resident on it (pipelined CELT steps:
k_celt_parse64 of step k+1 runs next to k_celt_recon_fb of step k, and the step is as long as the reconstruction).  No GPU needed:
the figures are read from the code objects inside libopusgpu.so, as tests/test_kernel_budget.py reads them, and from the library.

Two resources decide it, and easing one alone buys next to nothing:
  * registers -- a SIMD's 512, allocated in eights: the parse grid puts one parse wave on every SIMD, and five reconstruction
    waves must fit beside it (19 per CU want more than four on three of the four SIMDs);
  * LDS -- 128 granules of 1,280 bytes per CU: two parse workgroups per CU, five granules per reconstruction workgroup.
Also here: the bound that lets the parse kernel keep a band's dynalloc boost as a count in a byte (LaneArr::boost,
og_celt_parse.hpp), over every band, frame size and channel count."""
import ctypes as C
import os
import re
import sys

from test_kernel_budget import LIB, ROOT, _kernel_metadata

GRANULE, CU_GRANULES, SIMD_VGPRS = 1280, 128, 512


def _seen(*kernels):
    meta = _kernel_metadata()
    out = {}
    for mangled, v in meta.items():
        for k in kernels:
            if re.search(r"\d+" + k + r"(P|E|v|x|$)", mangled) or mangled == k:
                out[k] = v
    assert sorted(out) == sorted(kernels), sorted(meta)
    return out


def test_five_reconstruction_waves_fit_a_simd_beside_a_parse_wave():
    seen = _seen("k_celt_parse64", "k_celt_recon_fb")
    up8 = lambda v: (v + 7) // 8 * 8
    parse, recon = up8(seen["k_celt_parse64"][0]), up8(seen["k_celt_recon_fb"][0])
    print("allocated registers: parse64", parse, "recon_fb", recon, "scratch bytes", seen["k_celt_parse64"][1], seen["k_celt_recon_fb"][1])
    assert parse + 5 * recon <= SIMD_VGPRS, (parse, recon)
    assert seen["k_celt_recon_fb"][1] == 0, "the reconstruction spills"


def test_nineteen_reconstruction_workgroups_fit_a_cu_beside_two_parse_workgroups():
    seen = _seen("k_celt_parse64", "k_celt_recon_fb")
    lib = C.CDLL(LIB)
    lib.og_celt_parse64_lds_bytes.restype = C.c_int
    dynamic, static = lib.og_celt_parse64_lds_bytes(), seen["k_celt_parse64"][2]
    recon = -(-seen["k_celt_recon_fb"][2] // GRANULE)
    parse = -(-(dynamic + static) // GRANULE)
    print("LDS: parse64", dynamic, "+", static, "bytes =", parse, "granules; recon_fb", seen["k_celt_recon_fb"][2], "bytes =", recon)
    assert 0 < dynamic and seen["k_celt_recon_fb"][2] > 0  # (the reconstruction's working set is static: all of it is in the figure)
    assert recon <= 5
    assert parse <= 16
    assert (CU_GRANULES - 2 * parse) // 5 >= 19


def test_a_boost_count_fits_its_byte():
    """celt_parse_header's dynalloc loop adds the band's quanta while the boost is below the band's cap: ceil(cap / quanta) steps at
    the most.  The parse kernel keeps that count in a signed byte."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rom_tables as rom
    nb, worst = 21, (0,)
    assert len(rom.EBAND) == nb + 1 and len(rom.PULSE_CAPS) == 8 * nb
    for LM in range(4):
        for ch in (1, 2):
            for j in range(nb):
                n0 = (rom.EBAND[j + 1] - rom.EBAND[j]) << LM
                cap = (rom.PULSE_CAPS[nb * (2 * LM + ch - 1) + j] + 64) * ch * n0 >> 2
                width = ch * n0
                quanta = min(width << 3, max(6 << 3, width))
                assert quanta > 0
                worst = max(worst, (-(-cap // quanta), LM, ch, j))
    print("most boost steps (count, LM, channels, band):", worst)
    assert worst[0] == 66  # the figure og_celt.hpp quotes (dynalloc_quanta): band 14 of a stereo 20 ms frame
    assert worst[0] <= 127  # what a signed byte holds
