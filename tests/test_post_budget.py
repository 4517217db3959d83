"""What k_celt_post may take of a CU next to the reconstruction, read from the code objects inside libopusgpu.so as
tests/test_kernel_budget.py reads them (no GPU needed).

In a pipelined CELT step the de-emphasis of step k - 1 is resident for most of the reconstruction of step k, and every one of its
workgroups needs a contiguous piece of LDS that the critical kernel's 6.2 KB workgroups have to leave free: the kernel keeps ONE
transposition buffer, 9,216 bytes -- eight granules of 1,280 (thirteen before) -- and no scratch; its registers stay within the five
waves per SIMD it had.  The change that brought this must not have cost the reconstruction kernel anything: the same five granules,
at most 72 registers (seven waves per SIMD by registers, six by its launch bound), no scratch."""
import re

from test_kernel_budget import _kernel_metadata

GRANULE = 1280


def _seen(*kernels):
    meta = _kernel_metadata()
    out = {}
    for mangled, figures in meta.items():
        for k in kernels:
            if re.search(r"\d+" + k + r"(P|E|v|x|$)", mangled) or mangled == k:
                out[k] = figures  # (vgpr, scratch bytes, static LDS bytes)
    assert sorted(out) == sorted(kernels), (sorted(out), sorted(meta)[:6])
    return out


def test_the_de_emphasis_kernel_fits_eight_lds_granules():
    vgpr, scratch, lds = _seen("k_celt_post")["k_celt_post"]
    print("k_celt_post: registers", vgpr, "scratch bytes", scratch, "static LDS bytes", lds)
    assert 0 < lds <= 8 * GRANULE == 10240, lds
    assert scratch == 0, scratch
    assert vgpr <= 96, vgpr  # five waves per SIMD, as with thirteen granules


def test_the_reconstruction_kernel_kept_its_budget():
    vgpr, scratch, lds = _seen("k_celt_recon_fb")["k_celt_recon_fb"]
    print("k_celt_recon_fb: registers", vgpr, "scratch bytes", scratch, "static LDS bytes", lds)
    assert -(-lds // GRANULE) == 5, lds
    assert vgpr <= 72, vgpr
    assert scratch == 0, scratch
