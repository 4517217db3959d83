// og_parse64.hip -- k_celt_parse64: the CELT parse kernel with 64 frames per wave (og_parse_kernel.hpp says why there are two).
// A translation unit of its own because the frames per wave size the kernel's LDS arrays at compile time.
#include <hip/hip_runtime.h>
#define OG_PL_LANES 64
#define OG_PL_WAVES 2 // two such waves per workgroup share one copy of the ROM tables (3.3 KB): next to the reconstruction it is LDS x residency that counts
#define OG_PARSE_KERNEL_NAME k_celt_parse64
#define OG_PARSE_DYN_LDS 1
#define OG_PARSE_WAVES_PER_SIMD 3 // the register budget: 168 ...
// ... and 152 of them: a SIMD's 512 registers then hold this kernel's wave and FIVE of the reconstruction's 72 (152 + 5 x 72 = 512;
// at 168 they held four, with 56 registers idle).  The price is 13 spilled registers, 56 bytes of scratch, for 2 and 12.
#ifndef OG_PARSE_NUM_VGPR
#define OG_PARSE_NUM_VGPR 152
#endif
#include "og_parse_kernel.hpp"

extern "C" void og_launch_celt_parse64(hipStream_t s, int grid, const void *descs, const void *arena, void *streams, void *recs, int n,
                                       int n_streams, const void *handoff, int which, int groups, unsigned *started) {
    hipLaunchKernelGGL(k_celt_parse64, dim3(grid), dim3(64 * OG_PL_WAVES), OG_PARSE_LDS_BYTES, s, (const FrameDesc *)descs, (const u8 *)arena, (StreamState *)streams,
                       (ParseRec *)recs, n, n_streams, (const SilkHandoff *)handoff, which, groups, started);
}
extern "C" int og_celt_parse64_frames(void) { return OG_PL_FRAMES; }

// Next to the reconstruction (five granules of 1,280 bytes per workgroup) a CU holds (128 - 2 x this workgroup's granules) / 5 of
// that kernel's waves: 17 at 20 granules, 19 at 16.  The 256 bytes are the kernel's static LDS (the workgroup-wide vote's word).
static_assert(sizeof(ParseLds) == (size_t)OG_PL_LANES * (2 * NBANDS + 4 * NBANDS), "a parse wave's LDS: fine_quant, tf_prio and one word per band");
static_assert(sizeof(ParseLds) <= 8064 && OG_PARSE_LDS_BYTES + 256 <= 16 * 1280, "k_celt_parse64's workgroup no longer fits 16 LDS granules");
static_assert((128 - 2 * ((OG_PARSE_LDS_BYTES + 256 + 1279) / 1280)) / 5 >= 19, "fewer than 19 reconstruction workgroups per CU beside two parse workgroups");
extern "C" int og_celt_parse64_lds_bytes(void) { return (int)OG_PARSE_LDS_BYTES; } // (the dynamic part: what the launch asks for)
