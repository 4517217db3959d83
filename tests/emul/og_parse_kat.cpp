// TEST-ONLY (tests/test_parse_search_kat.py builds this itself): the parse kernel's rewritten decode helpers next to the code
// they replace, in the one-lane host emulation.  Each function walks its whole input set and returns the number of
// mismatches (0 = identical), leaving the first one in `where`.
#define OG_HOST_EMUL 1
#include <string.h>
#include "og_decode.hpp"

using namespace og;

// a lane's range decoder over `len` bytes of `buf`, advanced by `skip` binary symbols so that rng / val / the raw-bit window
// are somewhere in the middle of their life
static void kat_rc(RcLane &rc, const uint8_t *buf, int len, int skip) {
    memset(&rc, 0, sizeof(rc));
    rc_lane_attach(rc, buf, (u32)len);
    rc_init(rc, (u32)len);
    for (int i = 0; i < skip; i++) {
        rc_bit_logp(rc, 1 + (unsigned)(i & 3));
        if (i & 1) rc_bits(rc, 1 + (unsigned)(i % 5));
    }
}
static bool same_rc(const RcLane &a, const RcLane &b) {
    return a.storage == b.storage && a.end_offs == b.end_offs && a.end_window == b.end_window && a.nend_bits == b.nend_bits &&
           a.nbits_total == b.nbits_total && a.offs == b.offs && a.rng == b.rng && a.val == b.val && a.ext == b.ext && a.rem == b.rem &&
           a.error == b.error;
}

extern "C" {
// isqrt24 against isqrt32 (celt.cpp:3086) for EVERY argument below 2^24
long kat_isqrt(unsigned *where) {
    long bad = 0;
    for (u32 v = 1; v < (1u << 24); v++)
        if (isqrt24(v) != isqrt32(v) && !bad++) *where = v;
    return bad;
}

// the lane flavour of ec_dec_uint against the template it overloads: every total in ft_lo .. ft_hi and the totals in `extra`
// (the PVQ codebook sizes), each from `states` decoder states over the packet
long kat_uint(const uint8_t *buf, int len, unsigned ft_lo, unsigned ft_hi, const unsigned *extra, int n_extra, int states, unsigned *where,
              long *n_errors) {
    long bad = 0;
    *n_errors = 0;
    const long n = (long)(ft_hi - ft_lo + 1) + n_extra;
    for (long k = 0; k < n; k++) {
        const u32 ft = k < (long)(ft_hi - ft_lo + 1) ? ft_lo + (u32)k : extra[k - (ft_hi - ft_lo + 1)];
        if (ft < 2) continue;
        for (int s = 0; s < states; s++) {
            RcLane a, b;
            kat_rc(a, buf, len, s * 7);
            kat_rc(b, buf, len, s * 7);
            const u32 va = rc_uint(a, ft), vb = rc_uint<RcLane>(b, ft);
            if ((va != vb || !same_rc(a, b)) && !bad++) *where = ft;
            *n_errors += b.error != 0; // (the template's own flag: raw bits that carried the value past the total)
        }
        // ... and the corner the sampled states hardly ever reach: the TOP range-coded value (val below one step of the total)
        // followed by the packet's raw bits and by raw bits that are all ones -- unless the total is a power of two the latter
        // carries the value past it: ec_dec_uint's error return and its clamp
        static uint8_t ones[64];
        memset(ones, 0xff, sizeof(ones));
        for (int k2 = 0; k2 < 2; k2++) {
            RcLane a;
            kat_rc(a, k2 ? ones : buf, k2 ? (int)sizeof(ones) : len, 3);
            const int ftb = ilog(ft - 1) > 8 ? ilog(ft - 1) - 8 : 0;
            a.val %= a.rng / (((ft - 1) >> ftb) + 1);
            RcLane b = a;
            const u32 va = rc_uint(a, ft), vb = rc_uint<RcLane>(b, ft);
            if ((va != vb || !same_rc(a, b)) && !bad++) *where = ft;
            *n_errors += b.error != 0;
        }
    }
    return bad;
}

// number of PVQ codebook sizes the parse decodes indices against, and the table itself
int kat_pulse_v(unsigned *out, int cap) {
    const int n = (int)(sizeof(rom_pulse_v) / sizeof(rom_pulse_v[0]));
    for (int i = 0; i < n && i < cap; i++) out[i] = rom_pulse_v[i];
    return n;
}

// split_theta_lane against compute_theta (mono, as the partition walk called it): every band x LM after the split (-1 .. 2)
// x half size N the walk can reach for them x b in 0 .. b_max x both angle models (B0 = 1: triangular, B0 = 2: uniform), the
// decoder state changing from call to call.  where = band | (LM + 1) << 8 | B0 << 12, where[1] = b.
long kat_theta(const uint8_t *buf, int len, int b_max, int states, unsigned *where) {
    long bad = 0;
    parse_tables_load();
    int n = 0;
    for (int band = 0; band < NBANDS; band++)
        for (int LM = -1; LM <= 2; LM++) {
            const int N = ((rom_eband[band + 1] - rom_eband[band]) << 3) >> (3 - LM); // the band at LM = 3, halved 3 - LM times
            if (N < 1) continue;
            for (int B0 = 1; B0 <= 2; B0++)
                for (int b = 0; b <= b_max; b++, n++) {
                    RcLane r1, r2;
                    kat_rc(r1, buf, len, (n % states) * 5);
                    kat_rc(r2, buf, len, (n % states) * 5);
                    Split s1, s2;
                    i32 b1 = b, b2 = b, fill = 0;
                    split_theta_lane(r1, band, s1, N, b1, B0, LM);
                    compute_theta<RomLds>(r2, band, 0, 0, 0, s2, N, b2, (B0 + 1) >> 1, B0, LM, 0, fill);
                    const bool ok = b1 == b2 && s1.inv == s2.inv && s1.imid == s2.imid && s1.iside == s2.iside && s1.delta == s2.delta &&
                                    s1.itheta == s2.itheta && s1.qalloc == s2.qalloc && same_rc(r1, r2);
                    if (!ok && !bad++) {
                        where[0] = (unsigned)band | (unsigned)(LM + 1) << 8 | (unsigned)B0 << 12;
                        where[1] = (unsigned)b;
                    }
                }
        }
    return bad;
}

// The same comparison with the DECODED VALUE walked as well: for every split-angle resolution qn that compute_qn can return
// over the walk's whole domain (every band x LM x b, found by search: out_qn[] lists them), both angle models, and EVERY value
// fm in 0 .. ft - 1 that ec_decode can return for the model's total ft, from `states` decoder states each.  The state is an
// ordinary one (kat_rc) whose `val` is then placed inside the interval of the wanted value: ec_decode computes
// ext = rng / ft, s = val / ext, fm = ft - min(s + 1, ft), so val = ext (ft - 1 - fm) + (val mod ext) decodes to exactly fm (and
// stays below rng).  Both functions then run their own decode from that state; compared are the six fields of the split, the
// budget left and the coder state afterwards -- i.e. (itheta, fl, fs) through rng / val.  Returns mismatches; *n_cases = calls
// compared, *n_qn = resolutions found.  where = qn | B0 << 12, where[1] = fm.
long kat_theta_values(const uint8_t *buf, int len, int states, unsigned *where, long *n_cases, int *out_qn, int *n_qn) {
    long bad = 0;
    *n_cases = 0;
    *n_qn = 0;
    parse_tables_load();
    static int arg_band[260], arg_LM[260], arg_N[260], arg_b[260];
    static bool have[260];
    memset(have, 0, sizeof(have));
    for (int band = 0; band < NBANDS; band++)
        for (int LM = -1; LM <= 2; LM++) {
            const int N = ((rom_eband[band + 1] - rom_eband[band]) << 3) >> (3 - LM);
            if (N < 1) continue;
            const int pulse_cap = RomLds::logn(band) + LM * (1 << BITRES), offset = (pulse_cap >> 1) - 4;
            for (int b = 0; b <= 16383; b++) {
                const int qn = compute_qn(N, b, offset, pulse_cap, 0);
                if (qn < 0 || qn >= 260) return -1; // (outside what the frame layout of this test expects)
                if (!have[qn]) {
                    have[qn] = true;
                    arg_band[qn] = band; arg_LM[qn] = LM; arg_N[qn] = N; arg_b[qn] = b;
                }
            }
        }
    for (int qn = 2; qn < 260; qn++) {
        if (!have[qn]) continue;
        out_qn[(*n_qn)++] = qn;
        for (int B0 = 1; B0 <= 2; B0++) {
            const int h = qn >> 1, ftb = B0 > 1 ? (ilog((u32)qn) > 8 ? ilog((u32)qn) - 8 : 0) : 0;
            const u32 ft = B0 > 1 ? (u32)(qn >> ftb) + 1 : (u32)((h + 1) * (h + 1)); // ec_dec_uint(qn + 1)'s total / the triangle's
            for (u32 fm = 0; fm < ft; fm++)
                for (int st = 0; st < states; st++) {
                    RcLane r1;
                    kat_rc(r1, buf, len, st * 5 + 1);
                    const u32 ext = r1.rng / ft;
                    r1.val = ext * (ft - 1 - fm) + r1.val % ext;
                    RcLane r2 = r1;
                    { // the state really decodes to fm
                        RcLane probe = r1;
                        if (rc_decode(probe, ft) != fm) return -2;
                    }
                    if (B0 > 1) { // compute_theta's uniform branch goes through the overload too: the template's body from the same state
                        RcLane u1 = r1, u2 = r1;
                        const u32 v1 = rc_uint(u1, (u32)qn + 1), v2 = rc_uint<RcLane>(u2, (u32)qn + 1);
                        if ((v1 != v2 || !same_rc(u1, u2)) && !bad++) {
                            where[0] = (unsigned)qn | 15u << 12;
                            where[1] = fm;
                        }
                    }
                    Split s1, s2;
                    i32 b1 = arg_b[qn], b2 = arg_b[qn], fill = 0;
                    split_theta_lane(r1, arg_band[qn], s1, arg_N[qn], b1, B0, arg_LM[qn]);
                    compute_theta<RomLds>(r2, arg_band[qn], 0, 0, 0, s2, arg_N[qn], b2, (B0 + 1) >> 1, B0, arg_LM[qn], 0, fill);
                    const bool ok = b1 == b2 && s1.inv == s2.inv && s1.imid == s2.imid && s1.iside == s2.iside && s1.delta == s2.delta &&
                                    s1.itheta == s2.itheta && s1.qalloc == s2.qalloc && same_rc(r1, r2);
                    ++*n_cases;
                    if (!ok && !bad++) {
                        where[0] = (unsigned)qn | (unsigned)B0 << 12;
                        where[1] = fm;
                    }
                }
        }
    }
    return bad;
}
}
