// og_gpu_kat.hip -- TEST-ONLY drivers that run the kernels' device-side forms one at a time (tests/test_gpu_device_forms.py).
//
// Every unit-level known answer of this project otherwise runs the kernel source in host emulation (OG_HOST_EMUL), and the code the
// GPU runs is the other side of an #if: hardware approximations (the bare square root and reciprocal), inline assembly (24-bit
// multiply-adds, the 64-bit product, packed 16-bit dot products and subtractions), DPP scans and reductions, tables held in registers
// and fetched over the lane crossbar, the wave-uniform range decoder.  This file includes the headers as the product's translation
// units do -- OG_HOST_EMUL is NOT defined -- and wraps each form in a __global__ driver with a host entry point that takes host
// pointers (gk_host.hpp says what an entry point does and returns).  The general LDS layout (og_api.hip's); the leaf pass and the
// wave rotation need the tight one and live in og_gpu_kat_tight.hip.  Nothing here is linked into libopusgpu.so.
#include <hip/hip_runtime.h>
#include "og_decode.hpp"
#include "gk_host.hpp"

using namespace og;

// ---- (a) lane primitives: one case per lane, five input words and two output words per case ----------------------------------
enum { GK_U3, GK_ISQRT, GK_BLOCK_MUL, GK_BLOCK_OF, GK_MUL16X32, GK_SMULWB, GK_ROT_DOT2, GK_ADD3, GK_PK_SUB, GK_RS_DOT2, GK_N_OPS };
constexpr int GK_IN = 5, GK_OUT = 2;

__global__ void __launch_bounds__(256) k_gk_prim(int op, const u32 *__restrict__ in, u32 *__restrict__ out, int n) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= n) return;
    const u32 a = in[GK_IN * t], b = in[GK_IN * t + 1], c = in[GK_IN * t + 2], d = in[GK_IN * t + 3], e = in[GK_IN * t + 4];
    u32 r0 = 0, r1 = 0;
    switch (op) {
    case GK_U3: r0 = pvq_u3(a); break;
    case GK_ISQRT: r0 = (u32)pvq_isqrt_near(a); break;
    case GK_BLOCK_MUL: r0 = pvq_block_mul((int)a); break;
    case GK_BLOCK_OF: // a = j, b = blen: the block of coefficient j with the multiplier the device itself makes for blen
        r1 = pvq_block_mul((int)b);
        r0 = (u32)pvq_block_of((int)a, r1);
        break;
    case GK_MUL16X32: r0 = (u32)mul16x32_q15((i32)a, (i32)b); break;
    case GK_SMULWB: r0 = (u32)smulwb((i32)a, (i32)b); break;
    case GK_ROT_DOT2: { // pair = (a, b), coefficients = (c, d), e = the rounding term
        const u32 pair = rot_pack((i32)a, (i32)b), coef = rot_pack((i32)c, (i32)d);
        r0 = (u32)rot_dot2(pair, coef, (i32)e);
        r1 = pair;
        break;
    }
    case GK_ADD3: r0 = (u32)og_add3((i32)a, (i32)b, (i32)c); break;
    case GK_PK_SUB: r0 = og_pk_sub_i16(a, b); break;
    case GK_RS_DOT2: r0 = (u32)rs_dot2(a, b, (i32)c); break;
    default: break;
    }
    out[GK_OUT * t] = r0;
    out[GK_OUT * t + 1] = r1;
}

// the domain of case `in[0..5)` of `op`: what the comments at the form's definition promise its callers keep to
static bool gk_prim_ok(int op, const u32 *in) {
    switch (op) {
    case GK_U3: return in[0] >= 1u && in[0] < 2048u;        // h < 2^11
    case GK_ISQRT: return in[0] <= 176u * 176u;            // tq <= 176^2
    case GK_BLOCK_MUL: return in[0] >= 1u && in[0] <= 176u; // blen
    case GK_BLOCK_OF: return in[0] < 176u && in[1] >= 1u && in[1] <= 176u;
    default: return op >= 0 && op < GK_N_OPS;
    }
}

static int gk_prim(int op, const u32 *in, u32 *out, int n) {
    if (!in || !out || n < 0 || n > (1 << 24) || op < 0 || op >= GK_N_OPS) return -1;
    for (int t = 0; t < n; t++)
        if (!gk_prim_ok(op, in + (size_t)GK_IN * t)) return -(t + 1);
    if (n == 0) return 0;
    GkBuf din, dout;
    GK_TRY(din.alloc(sizeof(u32) * GK_IN * n));
    GK_TRY(dout.alloc(sizeof(u32) * GK_OUT * n));
    GK_TRY(hipMemcpy(din.p, in, sizeof(u32) * GK_IN * n, hipMemcpyHostToDevice));
    GK_TRY(hipMemset(dout.p, 0xee, sizeof(u32) * GK_OUT * n));
    hipLaunchKernelGGL(k_gk_prim, dim3((n + 255) / 256), dim3(256), 0, 0, op, din.as<u32>(), dout.as<u32>(), n);
    GK_RAN();
    GK_TRY(hipMemcpy(out, dout.p, sizeof(u32) * GK_OUT * n, hipMemcpyDeviceToHost));
    return 0;
}

// in: n x 5 words (unused ones ignored), out: n x 2 words (the second one: see k_gk_prim)
extern "C" {
int gk_pvq_u3(const u32 *in, u32 *out, int n) { return gk_prim(GK_U3, in, out, n); }
int gk_pvq_isqrt_near(const u32 *in, u32 *out, int n) { return gk_prim(GK_ISQRT, in, out, n); }
int gk_pvq_block_mul(const u32 *in, u32 *out, int n) { return gk_prim(GK_BLOCK_MUL, in, out, n); }
int gk_pvq_block_of(const u32 *in, u32 *out, int n) { return gk_prim(GK_BLOCK_OF, in, out, n); }
int gk_mul16x32_q15(const u32 *in, u32 *out, int n) { return gk_prim(GK_MUL16X32, in, out, n); }
int gk_smulwb(const u32 *in, u32 *out, int n) { return gk_prim(GK_SMULWB, in, out, n); }
int gk_rot_dot2(const u32 *in, u32 *out, int n) { return gk_prim(GK_ROT_DOT2, in, out, n); }
int gk_add3(const u32 *in, u32 *out, int n) { return gk_prim(GK_ADD3, in, out, n); }
int gk_pk_sub_i16(const u32 *in, u32 *out, int n) { return gk_prim(GK_PK_SUB, in, out, n); }
int gk_rs_dot2(const u32 *in, u32 *out, int n) { return gk_prim(GK_RS_DOT2, in, out, n); }
}

// ---- (b) wave helpers: one vector of 64 values per workgroup (one wave, every lane active), every lane's result kept --------------
enum { GK_WAVE_SUM, GK_WAVE_OR, GK_SCAN_ADD, GK_SCAN_MAX, GK_N_WAVE_OPS };

__global__ void __launch_bounds__(64) k_gk_wave(int op, const i32 *__restrict__ in, i32 *__restrict__ out) {
    const size_t at = (size_t)blockIdx.x * 64 + threadIdx.x;
    const i32 v = in[at];
    i32 r;
    if (op == GK_WAVE_SUM) r = wave_sum(v);
    else if (op == GK_WAVE_OR) r = (i32)wave_or((u32)v);
    else if (op == GK_SCAN_ADD) r = wave_scan_add(v);
    else r = wave_scan_max(v);
    out[at] = r;
}

static int gk_wave(int op, const i32 *in, i32 *out, int n_vec) {
    if (!in || !out || n_vec < 0 || n_vec > (1 << 16)) return -1;
    if (op == GK_SCAN_MAX) // (the prefix maximum is defined for values >= 0: a lane without a source reads 0)
        for (int t = 0; t < n_vec * 64; t++)
            if (in[t] < 0) return -(t / 64 + 1);
    if (n_vec == 0) return 0;
    const size_t bytes = sizeof(i32) * 64 * (size_t)n_vec;
    GkBuf din, dout;
    GK_TRY(din.alloc(bytes));
    GK_TRY(dout.alloc(bytes));
    GK_TRY(hipMemcpy(din.p, in, bytes, hipMemcpyHostToDevice));
    GK_TRY(hipMemset(dout.p, 0xee, bytes));
    hipLaunchKernelGGL(k_gk_wave, dim3(n_vec), dim3(64), 0, 0, op, din.as<i32>(), dout.as<i32>());
    GK_RAN();
    GK_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// in, out: n vectors of 64 words
extern "C" {
int gk_wave_sum(const i32 *in, i32 *out, int n) { return gk_wave(GK_WAVE_SUM, in, out, n); }
int gk_wave_or(const i32 *in, i32 *out, int n) { return gk_wave(GK_WAVE_OR, in, out, n); }
int gk_wave_scan_add(const i32 *in, i32 *out, int n) { return gk_wave(GK_SCAN_ADD, in, out, n); }
int gk_wave_scan_max(const i32 *in, i32 *out, int n) { return gk_wave(GK_SCAN_MAX, in, out, n); }
}

// ---- (d) the U table in registers (og_celt_bands.hpp: PvqTab): look-ups over the lane crossbar and the ballot search ------------
// A query is four words: 0 | a | b | - for u(a, b), 1 | row | k | i for row_search(row, k, i).  Queries are wave-uniform, as the
// single-kernel path's are; a workgroup (one wave) takes every gridDim.x-th one.
constexpr int GK_UTAB_GRID = 64;
__global__ void __launch_bounds__(64) k_gk_utab(const u32 *__restrict__ q, u32 *__restrict__ out, int n) {
    PvqTab T;
    T.load();
    for (int t = (int)blockIdx.x; t < n; t += (int)gridDim.x) {
        const int op = OG_UNI(q[4 * t]), a = OG_UNI(q[4 * t + 1]), b = OG_UNI(q[4 * t + 2]);
        const u32 i = (u32)OG_UNI(q[4 * t + 3]);
        const u32 r = op == 0 ? T.u(a, b) : (u32)T.row_search(a, b, i);
        if (OG_LANE == 0) out[t] = r;
    }
}

extern "C" int gk_pvq_tab(const u32 *q, u32 *out, int n) {
    if (!q || !out || n < 0 || n > (1 << 22)) return -1;
    for (int t = 0; t < n; t++) {
        const u32 op = q[4 * t], a = q[4 * t + 1], b = q[4 * t + 2];
        // u(a, b): the registers hold rows 0 .. 15 and columns 0 .. 191; row_search: rows 1 .. 14 (U(n, 0) = 0 ends the search)
        const bool ok = op == 0 ? (a < 192u && b < 192u && (a < 16u || b < 16u)) : (op == 1 && a >= 1u && a <= 14u && b < 192u);
        if (!ok) return -(t + 1);
    }
    if (n == 0) return 0;
    GkBuf dq, dout;
    GK_TRY(dq.alloc(sizeof(u32) * 4 * n));
    GK_TRY(dout.alloc(sizeof(u32) * n));
    GK_TRY(hipMemcpy(dq.p, q, sizeof(u32) * 4 * n, hipMemcpyHostToDevice));
    GK_TRY(hipMemset(dout.p, 0xee, sizeof(u32) * n));
    hipLaunchKernelGGL(k_gk_utab, dim3(GK_UTAB_GRID), dim3(64), 0, 0, dq.as<u32>(), dout.as<u32>(), n);
    GK_RAN();
    GK_TRY(hipMemcpy(out, dout.p, sizeof(u32) * n, hipMemcpyDeviceToHost));
    return 0;
}

// ---- (e) the wave-uniform inverse-CDF decoder (og_range.hpp: rc_icdf on an Rc) ----------------------------------------------------
// `tabs`: table bytes, a case's table at its offset with 64 readable entries behind it (lane l looks at entry l).  A case is four
// words in: table offset | rng | val | rem, and six out: symbol | val | rng | offs | rem | nbits_total.  The packet every case
// renormalises from is the same `pkt` (GK_ICDF_PKT bytes, read from the start), nbits_total starts at GK_ICDF_NBITS.
constexpr int GK_ICDF_PKT = 8, GK_ICDF_NBITS = 100, GK_ICDF_GRID = 256;
__global__ void __launch_bounds__(64) k_gk_icdf(const u8 *__restrict__ tabs, const u32 *__restrict__ cases, const u8 *__restrict__ pkt,
                                                u32 *__restrict__ out, int n, unsigned ftb) {
    if (OG_LANE < GK_ICDF_PKT) S.pkt[OG_LANE] = pkt[OG_LANE];
    OG_FULL_SYNC();
    for (int t = (int)blockIdx.x; t < n; t += (int)gridDim.x) {
        Rc rc;
        rc.storage = GK_ICDF_PKT;
        rc.end_offs = rc.end_window = 0;
        rc.nend_bits = 0;
        rc.nbits_total = GK_ICDF_NBITS;
        rc.offs = 0;
        rc.rng = (u32)OG_UNI(cases[4 * t + 1]);
        rc.val = (u32)OG_UNI(cases[4 * t + 2]);
        rc.ext = 0;
        rc.rem = OG_UNI(cases[4 * t + 3]);
        rc.error = 0;
        const int ret = rc_icdf(rc, tabs + OG_UNI(cases[4 * t]), ftb);
        if (OG_LANE == 0) {
            u32 *o = out + 6 * (size_t)t;
            o[0] = (u32)ret;
            o[1] = rc.val;
            o[2] = rc.rng;
            o[3] = rc.offs;
            o[4] = (u32)rc.rem;
            o[5] = (u32)rc.nbits_total;
        }
    }
}

extern "C" int gk_rc_icdf(const u8 *tabs, int tabs_len, const u32 *cases, const u8 *pkt, u32 *out, int n, unsigned ftb) {
    if (!tabs || !cases || !pkt || !out || n < 0 || n > (1 << 22) || tabs_len < 64 || tabs_len > (1 << 24) || ftb < 1 || ftb > 8) return -1;
    for (int t = 0; t < n; t++) {
        const u32 off = cases[4 * t], rng = cases[4 * t + 1], val = cases[4 * t + 2], rem = cases[4 * t + 3];
        // a decoder state between two symbols: 2^23 < rng <= 2^31, val < rng; the table's 64 entries inside `tabs`, a zero among them
        // (the symbol the search always ends at)
        bool ok = off <= (u32)tabs_len - 64u && rng > (1u << 23) && rng <= (1u << 31) && val < rng && rem < 256u;
        if (ok) {
            bool zero = false;
            for (int l = 0; l < 64; l++) zero |= tabs[off + l] == 0;
            ok = zero;
        }
        if (!ok) return -(t + 1);
    }
    if (n == 0) return 0;
    GkBuf dt, dc, dp, dout;
    GK_TRY(dt.alloc((size_t)tabs_len));
    GK_TRY(dc.alloc(sizeof(u32) * 4 * n));
    GK_TRY(dp.alloc(GK_ICDF_PKT));
    GK_TRY(dout.alloc(sizeof(u32) * 6 * n));
    GK_TRY(hipMemcpy(dt.p, tabs, (size_t)tabs_len, hipMemcpyHostToDevice));
    GK_TRY(hipMemcpy(dc.p, cases, sizeof(u32) * 4 * n, hipMemcpyHostToDevice));
    GK_TRY(hipMemcpy(dp.p, pkt, GK_ICDF_PKT, hipMemcpyHostToDevice));
    GK_TRY(hipMemset(dout.p, 0xee, sizeof(u32) * 6 * n));
    hipLaunchKernelGGL(k_gk_icdf, dim3(GK_ICDF_GRID), dim3(64), 0, 0, dt.as<u8>(), dc.as<u32>(), dp.as<u8>(), dout.as<u32>(), n, ftb);
    GK_RAN();
    GK_TRY(hipMemcpy(out, dout.p, sizeof(u32) * 6 * n, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int gk_rc_icdf_pkt_len(void) { return GK_ICDF_PKT; }
extern "C" int gk_rc_icdf_nbits(void) { return GK_ICDF_NBITS; }

// ---- (e) the lane-private decoder's packet byte (og_range.hpp: rc_next_byte on an RcLane) ------------------------------------------
// Lane l reads a packet of `len` bytes that starts l bytes into `data`: every alignment of the 16-byte forward window four times
// over.  Each lane asks for len + 2 bytes (the two behind the packet read as zero) and keeps them all: out[l][len + 2].
constexpr int GK_BYTES_SLACK = 16; // the windows are aligned pieces: they reach up to 15 bytes in front of and behind a packet
__global__ void __launch_bounds__(64) k_gk_lane_bytes(const u8 *__restrict__ data, int len, u8 *__restrict__ out) {
    RcLane rc;
    rc_lane_attach(rc, data + OG_LANE, (u32)len);
    rc.storage = (u32)len;
    rc.offs = 0;
    for (int j = 0; j < len + 2; j++) out[OG_LANE * (len + 2) + j] = (u8)rc_next_byte(rc);
}

extern "C" int gk_rc_lane_bytes(const u8 *data, int len, u8 *out) { // data: len + 63 bytes
    if (!data || !out || len < 1 || len > 1275) return -1;
    const size_t span = (size_t)len + 63, alloc = span + 2 * GK_BYTES_SLACK, out_bytes = (size_t)64 * (len + 2);
    GkBuf dd, dout;
    GK_TRY(dd.alloc(alloc)); // (hipMalloc aligns to more than 16 bytes: the packets start GK_BYTES_SLACK in)
    GK_TRY(dout.alloc(out_bytes));
    GK_TRY(hipMemset(dd.p, 0x5a, alloc)); // what lies around the packets is NOT zero: a byte fetched from there shows
    GK_TRY(hipMemcpy(dd.as<u8>() + GK_BYTES_SLACK, data, span, hipMemcpyHostToDevice));
    GK_TRY(hipMemset(dout.p, 0xee, out_bytes));
    hipLaunchKernelGGL(k_gk_lane_bytes, dim3(1), dim3(64), 0, 0, dd.as<u8>() + GK_BYTES_SLACK, len, dout.as<u8>());
    GK_RAN();
    GK_TRY(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
    return 0;
}
