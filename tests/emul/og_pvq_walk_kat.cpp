// TEST-ONLY driver for tests/test_pvq_walk_sites.py: the reconstruction kernel's PVQ index walk (pvq_leaf_lane, og_celt_recon.hpp) in
// host emulation, in the LDS layout of k_celt_recon_fb, against the oracle's step-by-step cwrsi -- the pulses and their energy
// BEFORE the scaling (tapped), the scaled coefficients and the collapse mask; and the block-of-position arithmetic of the mask.
#define OG_HOST_EMUL 1
#define OG_RECON_TIGHT 1
#include <stdint.h>
static int16_t tap_y[256];
static int32_t tap_yy;
#define OG_PVQ_WALK_TAP(p, n, e)                       \
    do {                                               \
        for (int q_ = 0; q_ < (n); q_++) tap_y[q_] = (p)[q_]; \
        tap_yy = (e);                                  \
    } while (0)
#include "og_celt_recon.hpp"

extern "C" void og_emul_tap(int) {}
extern "C" {
int32_t oc_cwrsi(int n, int k, uint32_t i, int32_t *y);
uint32_t oc_test_pvq_leaf(int N, int K, uint32_t index, int spread, int B, int gain, int16_t *X);

// every index of idx[] x every block count in {1, 2, 4, 8} that divides n.  Returns the number of (index, B) cases that differ in
// anything (first one's index and what differed -- 1 pulses, 2 energy, 3 mask, 4 scaled coefficients -- in where[0..1]); *cases
// receives how many were compared.
long kat_walk(int n, int k, const uint32_t *idx, int nidx, uint32_t *where, long *cases) {
    static int32_t iy[256];
    static int16_t X[256];
    long bad = 0;
    og::pvq_tab_load();
    for (int t = 0; t < nidx; t++) {
        const int32_t ryy = oc_cwrsi(n, k, idx[t], iy);
        for (int B = 1; B <= 8; B <<= 1) {
            if (n % B) continue;
            const uint32_t rmask = oc_test_pvq_leaf(n, k, idx[t], 0, B, 32767, X);
            for (int q = 0; q < n; q++) og::S.v[og::V_X + q] = 0; // the walk relies on a cleared spectrum
            const uint32_t cm = og::pvq_leaf_lane(og::S.v, og::pvq_lds(), n, k, idx[t], og::V_X, B, 32767, 0);
            int what = 0;
            for (int q = 0; q < n && !what; q++)
                if (tap_y[q] != iy[q]) what = 1;
            if (!what && tap_yy != ryy) what = 2;
            if (!what && cm != rmask) what = 3;
            for (int q = 0; q < n && !what; q++)
                if (og::S.v[og::V_X + q] != X[q]) what = 4;
            if (what && !bad++) {
                where[0] = idx[t];
                where[1] = (uint32_t)(what | B << 8);
            }
            ++*cases;
        }
    }
    return bad;
}

// (j * M) >> 16 == j / blen and j * M < 2^24 for every j < 176, blen <= 176 and M = floor(65536 / blen) + 1 or + 2 (the GPU takes M
// from a reciprocal of one ulp: og_celt_recon.hpp); and the emulation's own M is the first of the two.  Returns the failures.
long kat_block_of(long *cases) {
    long bad = 0;
    for (int blen = 1; blen <= 176; blen++) {
        const uint32_t m0 = 65536u / (uint32_t)blen + 1u;
        if (og::pvq_block_mul(blen) != m0) bad++;
        for (uint32_t M = m0; M <= m0 + 1u; M++)
            for (int j = 0; j < 176; j++) {
                if ((uint32_t)j * M >= (1u << 24)) bad++;
                if (og::pvq_block_of(j, M) != j / blen) bad++;
                ++*cases;
            }
    }
    return bad;
}
}
