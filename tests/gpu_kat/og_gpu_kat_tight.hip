// og_gpu_kat_tight.hip -- TEST-ONLY driver of the PVQ leaf pass as the reconstruction kernel of 20 ms frames runs it (og_recon.hip,
// k_celt_recon_fb): the tight LDS layout, the table in LDS with its short rows in the spectrum's tops, one leaf per lane
// (pvq_leaf_lane with a deferred rotation), then the wave's rotations by the whole wave (pvq_rotate_wave).  A translation unit of
// its own because the layout is chosen at compile time (og_state.hpp).  See og_gpu_kat.hip; tests/test_gpu_device_forms.py (c).
#define OG_RECON_TIGHT 1
#include <hip/hip_runtime.h>
#include "og_celt_recon.hpp"
#include "gk_host.hpp"

using namespace og;

// What a leaf may occupy: the part of each channel's spectrum that bands reach.  The tops behind it hold the table's rows 9 - 14 and
// the rotation's marker row during the leaf pass (og_state.hpp): neither cleared nor written here.
constexpr int GK_CH0_LO = V_X, GK_CH0_HI = X_TOP0, GK_CH1_LO = V_X + 960, GK_CH1_HI = X_TOP1;
constexpr int GK_ROW = GK_CH1_HI; // coefficients kept per wave: positions [0, GK_ROW) of the arena (the first channel's top is skipped)
static_assert(GK_CH0_LO == 0 && GK_CH0_HI <= GK_CH1_LO && GK_CH1_HI <= V_NORM, "two channel ranges inside X");

// One leaf: n | k | index | pos | B | gain | spread | live (0: the lane has no leaf).  64 per wave.
constexpr int GK_LEAF_WORDS = 8;

__global__ void __launch_bounds__(64) k_gk_leaves(const u32 *__restrict__ leaves, i16 *__restrict__ coef, u32 *__restrict__ mask) {
    const int lane = OG_LANE;
    const u32 *lf = leaves + ((size_t)blockIdx.x * 64 + lane) * GK_LEAF_WORDS;
    const int n = (int)lf[0], k = (int)lf[1], pos = (int)lf[3], B = (int)lf[4], spread = (int)lf[6];
    const u32 index = lf[2];
    const i32 gain = (i32)lf[5];
    const bool live = lf[7] != 0;
    // the spectrum is cleared before the leaf pass (the walk does not store zeros)
    OG_FOR_LANES(t, GK_CH0_HI - GK_CH0_LO) S.v[GK_CH0_LO + t] = 0;
    OG_FOR_LANES(t, GK_CH1_HI - GK_CH1_LO) S.v[GK_CH1_LO + t] = 0;
    pvq_tab_load();
    OG_FULL_SYNC();
    RotJob job;
    job.x = job.blen = job.logB = job.stride2 = 0;
    job.c = job.s = 0;
    job.on = false;
    u32 cm = 0;
    if (live) cm = pvq_leaf_lane(S.v, pvq_lds(), n, k, index, V_X + pos, B, gain, spread, &job);
    OG_LSYNC();
    pvq_rotate_wave(S.v, job, S.rot_marker());
    OG_FULL_SYNC();
    i16 *row = coef + (size_t)blockIdx.x * GK_ROW;
    OG_FOR_LANES(t, GK_CH0_HI - GK_CH0_LO) row[GK_CH0_LO + t] = S.v[GK_CH0_LO + t];
    OG_FOR_LANES(t, GK_CH1_HI - GK_CH1_LO) row[GK_CH1_LO + t] = S.v[GK_CH1_LO + t];
    mask[(size_t)blockIdx.x * 64 + lane] = cm;
}

// U(n, k) of the PVQ codebook sizes, saturated well above 2^32: V(n, k) = U(n, k) + U(n, k + 1) codewords
static unsigned long long gk_u(int n, int k) {
    static unsigned long long U[178][178];
    static bool made = false;
    if (!made) {
        const unsigned long long cap = 1ull << 40;
        for (int a = 0; a < 178; a++)
            for (int b = 0; b < 178; b++) {
                unsigned long long v = (a == 0 || b == 0) ? (unsigned long long)(a == 0 && b == 0) : U[a - 1][b] + U[a][b - 1] + U[a - 1][b - 1];
                U[a][b] = v > cap ? cap : v;
            }
        made = true;
    }
    return U[n][k];
}

// The domain of the leaf driver, wave by wave: every leaf a legal one (a 32-bit codebook whose walk stays in table rows 0 .. 14, an
// index inside it, a block count that is a power of two dividing N, a 16-bit gain), inside one channel's range, and no two
// leaves of a wave on the same coefficient.  Returns 0, or -(w + 1) for the first wave w with a leaf outside.
static int gk_leaves_domain(const u32 *leaves, int n_waves) {
    if (!leaves || n_waves < 0 || n_waves > (1 << 16)) return -1;
    for (int w = 0; w < n_waves; w++) {
        unsigned char used[GK_ROW];
        memset(used, 0, sizeof(used));
        for (int l = 0; l < 64; l++) {
            const u32 *lf = leaves + ((size_t)w * 64 + l) * GK_LEAF_WORDS;
            if (lf[7] == 0) continue;
            const u32 n = lf[0], k = lf[1], index = lf[2], pos = lf[3], B = lf[4], gain = lf[5], spread = lf[6];
            bool ok = lf[7] == 1 && n >= 2 && n <= 176 && k >= 1 && k <= 176 && (n <= 14 || k <= 14) && spread <= 3 && gain <= 32767;
            ok = ok && (B == 1 || B == 2 || B == 4 || B == 8 || B == 16) && n % B == 0;
            if (ok) {
                const unsigned long long v = gk_u((int)n, (int)k) + gk_u((int)n, (int)k + 1);
                ok = v <= 0xFFFFFFFFull && index < v;
            }
            ok = ok && ((pos >= (u32)GK_CH0_LO && pos + n <= (u32)GK_CH0_HI) || (pos >= (u32)GK_CH1_LO && pos + n <= (u32)GK_CH1_HI));
            if (!ok) return -(w + 1);
            for (u32 t = pos; t < pos + n; t++) {
                if (used[t]) return -(w + 1);
                used[t] = 1;
            }
        }
    }
    return 0;
}

extern "C" {
// {first, end} of the two ranges a leaf may lie in, and the length of a wave's row in gk_pvq_leaves' `coef`
void gk_leaf_layout(int out[5]) {
    out[0] = GK_CH0_LO;
    out[1] = GK_CH0_HI;
    out[2] = GK_CH1_LO;
    out[3] = GK_CH1_HI;
    out[4] = GK_ROW;
}
// the domain check alone (host code: no HIP call)
int gk_pvq_leaves_check(const u32 *leaves, int n_waves) { return gk_leaves_domain(leaves, n_waves); }
// leaves: n_waves x 64 x 8 words; coef: n_waves x GK_ROW int16 (a leaf's coefficients at its position); mask: n_waves x 64
int gk_pvq_leaves(const u32 *leaves, i16 *coef, u32 *mask, int n_waves) {
    const int dom = gk_leaves_domain(leaves, n_waves);
    if (dom != 0) return dom;
    if (!coef || !mask) return -1;
    if (n_waves == 0) return 0;
    const size_t lb = sizeof(u32) * GK_LEAF_WORDS * 64 * (size_t)n_waves, cb = sizeof(i16) * GK_ROW * (size_t)n_waves, mb = sizeof(u32) * 64 * (size_t)n_waves;
    GkBuf dl, dc, dm;
    GK_TRY(dl.alloc(lb));
    GK_TRY(dc.alloc(cb));
    GK_TRY(dm.alloc(mb));
    GK_TRY(hipMemcpy(dl.p, leaves, lb, hipMemcpyHostToDevice));
    GK_TRY(hipMemset(dc.p, 0, cb));
    GK_TRY(hipMemset(dm.p, 0xee, mb));
    hipLaunchKernelGGL(k_gk_leaves, dim3(n_waves), dim3(64), 0, 0, dl.as<u32>(), dc.as<i16>(), dm.as<u32>());
    GK_RAN();
    GK_TRY(hipMemcpy(coef, dc.p, cb, hipMemcpyDeviceToHost));
    GK_TRY(hipMemcpy(mask, dm.p, mb, hipMemcpyDeviceToHost));
    return 0;
}
}
