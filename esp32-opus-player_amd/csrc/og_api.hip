// og_api.hip -- HIP kernels and the C ABI (include/opusgpu.h) of libopusgpu.so, gfx950 only.
//
// Launch shape: one workgroup == one wavefront (64 threads) == one 20 ms frame of one stream.  A
// decode step over n streams launches n workgroups (n >> 256 CUs x 8 waves for the BASELINE configs),
// each touching only its own stream record, so there is no inter-workgroup communication at all and
// block -> XCD placement cannot matter for correctness; the per-stream records are private, so L2
// affinity is not a concern either.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <condition_variable>
#include <functional>
#include <memory>
#include <new>
#include <mutex>
#include <thread>
#include <vector>
#include "og_decode.hpp"
#include "og_host_framing.hpp"
#include "og_output.hpp"
#include "og_debug.hpp"

using namespace og;

static_assert(sizeof(opusgpu_frame_desc) == sizeof(FrameDesc), "descriptor layout");

// ---- kernels --------------------------------------------------------------------------------------
// OPUSGPU_STALL_STREAM / OPUSGPU_STALL_US (og_debug.hpp): one wave that holds its stream for `ticks` of the device wall clock.  It
// writes no memory, and `max_spins` ends its loop whatever the clock reads.
#define OG_STALL_MAX_SPINS (1 << 20) // (each spin sleeps >= 512 cycles: 100 ms, the longest stall asked for, is < 470,000 spins at 2.4 GHz)
__global__ void __launch_bounds__(64) k_stream_stall(long long ticks, int max_spins) {
    const long long t0 = wall_clock64();
    for (int i = 0; i < max_spins && wall_clock64() - t0 < ticks; i++) __builtin_amdgcn_s_sleep(8);
}
__global__ void __launch_bounds__(64) k_stream_init(StreamState *st, int first, int count, int channels, int full) {
    const int s = first + (int)blockIdx.x;
    if ((int)blockIdx.x >= count) return;
    if (full)
        stream_init(&st[s], channels);
    else
        stream_reset(&st[s]);
}

// Ogg page checksums (ogg_page_checksum_set src/ogg.cpp:439-480: CRC-32, polynomial 0x04c11db7, MSB first, zero start,
// no final inversion, the four checksum bytes taken as zero), ONE PAGE PER LANE, eight 256-entry tables in LDS.
// A lane walking its own page with its own loads would make every wave-level load touch 64 cache lines and come back to
// each line eight times, long after L1 has dropped it (measured: 0.55 TB/s).  Instead the wave moves whole 64-byte lines:
// per step, four lanes fetch one line of one page (a load instruction covers 16 pages) into an LDS tile, then every lane
// consumes its own 64-byte row eight bytes at a time.  The chunks are the MEMORY's 64-byte lines, not the page's: a
// zero-start CRC ignores leading zero bytes, so a page that starts z bytes into a line is taken as z zeros followed by the
// page; every 16-byte load is aligned (pages ending on line boundaries measured 18-25 % faster than pages at arbitrary
// offsets when the chunks were counted from the page's end instead), no load passes the 16-byte block that holds the
// page's last byte, and only the last chunk of a page is partial (eight-byte steps, then at most seven single bytes).
// status: 1 match, 0 mismatch, OPUSGPU_PAGE_BAD_CAPTURE malformed.
// Chunk size and prefetch depth were measured (786,432 pages, shuffled / grouped sizes; the same
// build varies by up to 10 % between runs on the grouped input, so only the last line is a real difference):
//   64-byte chunks, one chunk ahead   2.70 - 2.72 / 3.08 - 3.45 TB/s   HBM traffic (FETCH_SIZE) 1.53 / 1.69 x the page bytes
//   64-byte chunks, two chunks ahead  2.60 / 3.19
//   128-byte chunks, two ahead        2.40 / 2.93        traffic 1.18 x (the second half of a 128-byte line is no longer
//                                                        fetched again after the L2 dropped it), but 12 instead of 20
//                                                        waves per CU, and the table lookups in LDS are what binds
enum {
    CRC_CHUNK = 64,               // bytes of a page per step
    CRC_DEPTH = 1,                // chunks requested ahead of the one being worked on (1 or 2)
    CRC_LPL = CRC_CHUNK / 16,     // lanes per line: each fetches 16 bytes
    CRC_PPI = 64 / CRC_LPL,       // pages covered by one load instruction of the wave
    CRC_NL = 64 / CRC_PPI,        // load instructions per chunk of the wave's 64 pages
    CRC_ROW = CRC_CHUNK / 4 + 1,  // tile row stride in words (+ 1 word: conflict-free column walks)
    CRC_STEPS = CRC_CHUNK / 8     // slice-by-8 steps per full chunk
};
__global__ void __launch_bounds__(256) k_pages_crc(const u8 *__restrict__ blob, const long long *__restrict__ offs,
                                                    const i32 *__restrict__ lens, i32 *__restrict__ status, int n,
                                                    const u32 *__restrict__ tables) {
    __shared__ u32 T[8][256];
    __shared__ u32 tile[4][64 * CRC_ROW];
    __shared__ long long pg_start[4][64]; // blob offset of the first (virtual) byte of the page's first chunk: offs - z
    __shared__ i32 pg_meta[4][64];        // z | chunks << 8
    for (int i = (int)threadIdx.x; i < 8 * 256; i += 256) T[i >> 8][i & 255] = tables[i];
    const int wv = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    // ---- per lane: is this a complete page, and how long is it?
    int total = 0, st = OPUSGPU_PAGE_BAD_CAPTURE;
    u32 want = 0;
    long long at0 = 0;
    if (p < n) {
        // The lanes' pages lie far apart, so every load here is a memory round trip of its own: the 27 header bytes come as
        // two 16-byte loads and the lacing values 16 at a time (byte loads only where a wide one could pass the page's end).
        const u8 *pg = blob + offs[p];
        const int len = lens[p];
        if (len >= 27) {
            u32 h[8];
            if (len >= 32) {
                const uint4 a = *reinterpret_cast<const uint4 *>(pg), b = *reinterpret_cast<const uint4 *>(pg + 16);
                h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w; h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;
            } else {
                for (int i = 0; i < 8; i++) h[i] = 0;
                for (int i = 0; i < 27; i++) h[i >> 2] |= (u32)pg[i] << (8 * (i & 3));
            }
            const int nseg = (int)(h[6] >> 16) & 255, hdr = 27 + nseg; // byte 26
            if (h[0] == 0x5367674fu /* "OggS" */ && (h[1] & 255u) == 0 && len >= hdr) {
                u32 body = 0;
                for (int i = 0; i < nseg; i += 16) {
                    u32 v[4];
                    if (27 + i + 16 <= len) {
                        const uint4 q = *reinterpret_cast<const uint4 *>(pg + 27 + i);
                        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                    } else {
                        v[0] = v[1] = v[2] = v[3] = 0;
                        for (int b = 0; b < 16 && i + b < nseg; b++) v[b >> 2] |= (u32)pg[27 + i + b] << (8 * (b & 3));
                    }
                    const int keep = nseg - i; // lacing values in this group: the rest of the 16 bytes is page body
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const int kd = keep - 4 * d;
                        const u32 m = kd >= 4 ? 0xffffffffu : kd <= 0 ? 0u : (1u << (8 * kd)) - 1u;
                        body = __builtin_amdgcn_sad_u8(v[d] & m, 0u, body); // sum of the four bytes
                    }
                }
                if (len >= hdr + (int)body) {
                    total = hdr + (int)body;
                    st = 0;
                    want = h[5] >> 16 | h[6] << 16; // bytes 22 .. 25, little-endian
                }
            }
        }
        at0 = offs[p];
    }
    // z: where in its 64-byte line the page starts (by ADDRESS: the blob itself may start anywhere)
    const int z = st < 0 ? 0 : (int)((reinterpret_cast<unsigned long long>(blob) + (unsigned long long)at0) & (unsigned long long)(CRC_CHUNK - 1));
    const int nfull = (z + total) / CRC_CHUNK, tail = (z + total) % CRC_CHUNK, chunks = nfull + (tail != 0);
    pg_start[wv][lane] = at0 - z;
    pg_meta[wv][lane] = z | total << 8; // total <= 27 + 255 + 255 * 255
    __syncthreads();
    int max_chunks = chunks;
    for (int d = 32; d; d >>= 1) max_chunks = max(max_chunks, __shfl_xor(max_chunks, d, 64));
    u32 crc = 0;
    const int grp = lane / CRC_LPL, quarter = lane % CRC_LPL; // this lane fetches 16-byte part `quarter` of the line of page CRC_PPI i + grp
    // chunk k of the wave's 64 pages into registers: CRC_LPL lanes per line, CRC_NL lines per lane
    auto fetch = [&](int k, u32 (&w)[CRC_NL][4]) {
#pragma unroll
        for (int i = 0; i < CRC_NL; i++) {
            const int q = CRC_PPI * i + grp;
            const i32 meta = pg_meta[wv][q];
            const int idx = CRC_CHUNK * k + 16 * quarter - (meta & 255); // page byte index of the quarter's first byte
            w[i][0] = w[i][1] = w[i][2] = w[i][3] = 0u;
            if (idx > -16 && idx < (meta >> 8)) { // the quarter holds at least one byte of the page
                const uint4 v = *reinterpret_cast<const uint4 *>(
                    __builtin_assume_aligned(blob + (pg_start[wv][q] + CRC_CHUNK * k + 16 * quarter), 16));
                w[i][0] = v.x; w[i][1] = v.y; w[i][2] = v.z; w[i][3] = v.w;
                if (idx < 26) { // near the page start: what precedes the page counts as zeros; so do bytes 22 .. 25 (the checksum)
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        u32 m = 0;
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            const int ib = idx + 4 * d + c;
                            if (ib >= 0 && !(ib >= 22 && ib <= 25)) m |= 0xffu << (8 * c);
                        }
                        w[i][d] &= m;
                    }
                }
            }
        }
    };
    // one chunk of the wave's pages from registers through the tile into the lanes' checksums
    auto consume = [&](int k, u32 (&w)[CRC_NL][4]) {
#pragma unroll
        for (int i = 0; i < CRC_NL; i++) {
            u32 *dst = &tile[wv][(CRC_PPI * i + grp) * CRC_ROW + 4 * quarter];
            dst[0] = w[i][0]; dst[1] = w[i][1]; dst[2] = w[i][2]; dst[3] = w[i][3];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the registers are free again: request a later chunk before this one is worked on, so that its memory latency
        // runs under the CRC work
        if (k + CRC_DEPTH < max_chunks) fetch(k + CRC_DEPTH, w);
        // ---- every lane consumes its own row: all of it, or (last chunk) the bytes up to the page's end
        const u32 *rowp = &tile[wv][lane * CRC_ROW];
        const int steps = k < nfull ? CRC_STEPS : k == nfull ? tail >> 3 : 0;
#pragma unroll
        for (int j = 0; j < CRC_STEPS; j++) {
            if (j < steps) {
                const u32 lo = rowp[2 * j], hi = rowp[2 * j + 1]; // message bytes b0 .. b3 | b4 .. b7, first byte lowest
                const u32 a = crc ^ ((lo & 0xffu) << 24 | (lo & 0xff00u) << 8 | (lo >> 8 & 0xff00u) | lo >> 24);
                crc = T[7][a >> 24] ^ T[6][(a >> 16) & 255] ^ T[5][(a >> 8) & 255] ^ T[4][a & 255] ^ T[3][hi & 255] ^
                      T[2][(hi >> 8) & 255] ^ T[1][(hi >> 16) & 255] ^ T[0][hi >> 24];
            }
        }
        if (k == nfull && (tail & 7)) {
            const int base = tail & ~7;
            for (int b = 0; b < (tail & 7); b++) {
                const int i = base + b;
                crc = crc << 8 ^ T[0][crc >> 24 ^ (rowp[i >> 2] >> (8 * (i & 3)) & 255u)];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    u32 wa[CRC_NL][4], wb[CRC_NL][4]; // chunks on their way (wb: only with CRC_DEPTH == 2)
    if (max_chunks > 0) fetch(0, wa);
    if (CRC_DEPTH == 2) {
        if (max_chunks > 1) fetch(1, wb);
        for (int k = 0; k < max_chunks; k += 2) {
            consume(k, wa);
            if (k + 1 < max_chunks) consume(k + 1, wb);
        }
    } else {
        for (int k = 0; k < max_chunks; k++) consume(k, wa);
    }
    if (p < n) status[p] = st < 0 ? st : (i32)(crc == want);
}

// Output stage (og_output.hpp): a thread makes four consecutive I2S words of one block.  Plain streaming work: 4 bytes in,
// 4 bytes out per word in the usual 16-bit stereo case, which takes the 16-byte path when the caller's layout allows it.
static_assert(sizeof(opusgpu_output_cfg) == sizeof(OutputCfg) && sizeof(OutputCfg) == 4, "output cfg layout");
__global__ void __launch_bounds__(256) k_output_stage(const i16 *__restrict__ pcm, long long pcm_stride, const i32 *__restrict__ valid_of,
                                                       int valid_all, int block_samples, const OutputCfg *__restrict__ cfg_of,
                                                       OutputCfg cfg_all, u32 *__restrict__ out, long long out_stride,
                                                       int units_per_block, long long n_units, int vec_ok) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_units) return;
    const int b = (int)(t / units_per_block), w0 = 4 * (int)(t - (long long)b * units_per_block);
    const OutputCfg c = cfg_of ? cfg_of[b] : cfg_all;
    int valid = valid_of ? valid_of[b] : valid_all; // a decode result: negative = the frame failed, nothing to play
    valid = valid > block_samples ? block_samples : valid;
    const int count = output_words(c, valid);
    if (w0 >= count) return;
    const i16 *blk = pcm + (size_t)b * pcm_stride;
    u32 *dst = out + (size_t)b * out_stride + w0;
    if (vec_ok && c.bits == 16 && c.channels == 2 && w0 + 4 <= count) {
        const uint4 v = *reinterpret_cast<const uint4 *>(blk + 2 * w0); // four stereo samples
        const u32 in[4] = {v.x, v.y, v.z, v.w};
        u32 o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            i32 l = (i32)(i16)(in[j] & 0xffffu), r = (i32)(i16)(in[j] >> 16);
            if (c.force_mono) l = r = (i32)(i16)((l + r) / 2);
            o[j] = output_pack(l, r, false, (i32)c.volume);
        }
        *reinterpret_cast<uint4 *>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        for (int j = 0; j < 4 && w0 + j < count; j++) dst[j] = output_word(blk, w0 + j, c);
    }
}

#ifndef OG_WAVES_PER_SIMD
#define OG_WAVES_PER_SIMD 1
#endif
#define OG_RECON_WAVES 2
#define OG_SILK_WAVES 2
__global__ void __launch_bounds__(64, OG_WAVES_PER_SIMD) k_decode_step(const FrameDesc *__restrict__ descs, const u8 *__restrict__ arena,
                                                   StreamState *st, i16 *pcm, i32 *result, int n, int n_streams,
                                                   int pcm_stride, int skip_celt, SilkHandoff *handoff, const SilkRec *srecs,
                                                   int q4_only) {
    // First pass (or the only one): one workgroup per slot.  Second pass of the split path (q4_only): it almost never has a
    // frame, so a workgroup looks at 64 slots -- one per lane -- and decodes the few that were parked for it one after the
    // other: 1 / 64 of the workgroups to start and end for nothing.
    unsigned long long todo = 1ull;
    int base = (int)blockIdx.x;
    if (q4_only) {
        base = (int)blockIdx.x * 64;
        const int f0 = base + (int)threadIdx.x;
        bool mine = false;
        if (f0 < n) {
            const FrameDesc d0 = descs[f0];
            mine = d0.stream >= 0 && d0.stream < n_streams && !desc_rfc(d0.flags) && desc_mode(d0.flags) == MODE_SILK && handoff[f0].valid == 2;
        }
        todo = __ballot(mine);
    }
    while (todo) {
        const int f = base + (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        if (f >= n) return;
        const FrameDesc d = descs[f];
        int ret;
        if (d.stream < 0 || d.stream >= n_streams) {
            ret = BAD_ARG;
        } else if (desc_rfc(d.flags)) {
            continue; // RFC-mode frames belong to k_decode_rfc (og_rfc.hip)
        } else if (skip_celt && desc_mode(d.flags) == MODE_CELT) {
            continue; // CELT-only frames take the split path (k_celt_parse + k_celt_recon)
        } else {
            StreamState *s = &st[d.stream];
#ifdef OG_PROF_SINGLE // profiling builds: time the sections of the single-kernel path
            OG_PROF_INIT();
#endif
            ret = decode_frame_wave<true>(s, arena + d.offset, d.len, desc_mode(d.flags), desc_bandwidth(d.flags),
                                          desc_channels(d.flags), pcm + (size_t)f * pcm_stride, handoff ? &handoff[f] : nullptr,
                                          srecs ? &srecs[f] : nullptr, q4_only, desc_mode_after(d.flags));
#ifdef OG_PROF_SINGLE
            OG_PROF_FLUSH();
#endif
            if (ret == CONTINUE_SPLIT) continue; // the split path finishes this frame and reports its result
        }
        if (threadIdx.x == 0) result[f] = ret;
        __syncthreads();
    }
}

// SILK-only and hybrid frames on the split path, arithmetic half: k_silk_synth (og_silk_synth.hip) and, for narrowband SILK-only
// frames, k_silk_synth_nb (og_silk_nb.hip) -- translation units of their own: their LDS working set has a layout of its own
extern "C" void og_launch_silk_synth(hipStream_t s, const void *descs, const void *arena, void *streams, void *pcm, void *result, int n,
                                     int n_streams, int pcm_stride, void *handoff, const void *srecs, int nb_elsewhere);
extern "C" void og_launch_silk_synth_nb(hipStream_t s, const void *descs, const void *arena, void *streams, void *pcm, void *result, int n,
                                        int n_streams, int pcm_stride, void *handoff, const void *srecs, int nb_elsewhere);

// SILK-only and hybrid frames, entropy half: ONE FRAME PER LANE (og_silk_parse.hpp).  Lane l < LANES of workgroup g decodes the side
// information and pulses of frame LANES g + l into srecs[frame] and leaves the coder state in handoff[frame].  Twice, like the CELT
// parse: k_silk_parse with 32 frames per wave (the upper lanes idle) for small in-order steps, k_silk_parse64 with 64 for pipelined
// steps and large batches (og_silk_parse.hpp, OG_SP_LANES).
#define OG_SPARSE_WAVES 4
// `shadow` (null in in-order steps): the per-stream copies of what the entropy half needs of the past, kept by this kernel for
// pipelined SILK / hybrid steps (SilkShadow, og_silk_parse.hpp); `epoch`: the context's current one.
template <int LANES>
OG_DEV void silk_parse_kernel_body(const FrameDesc *__restrict__ descs, const u8 *__restrict__ arena, const StreamState *st, SilkRec *srecs,
                                   SilkHandoff *handoff, int n, int n_streams, SilkShadow *shadow, u32 epoch) {
    silk_tables_load();
    if ((int)threadIdx.x >= LANES) return;
    const int f = (int)blockIdx.x * LANES + (int)threadIdx.x;
    if (f >= n) return;
    const FrameDesc d = descs[f];
    const int mode = desc_mode(d.flags);
    if (d.stream < 0 || d.stream >= n_streams || mode == MODE_CELT || desc_rfc(d.flags)) return;
#ifdef OG_PROF_SPARSE // profiling builds: time the sections of the SILK parse kernel (full batches only)
    OG_PROF_INIT();
#endif
    SilkShadow *const sh = shadow ? &shadow[d.stream] : nullptr;
    const SilkPast past(&st[d.stream], sh, epoch);
    silk_parse_lane(past, arena + d.offset, d.len, mode, desc_bandwidth(d.flags), desc_channels(d.flags), &srecs[f], &handoff[f], sh, epoch,
                    desc_mode_after(d.flags));
#ifdef OG_PROF_SPARSE
    OG_PROF_FLUSH();
#endif
}
__global__ void __launch_bounds__(64, OG_SPARSE_WAVES) k_silk_parse(const FrameDesc *__restrict__ descs, const u8 *__restrict__ arena,
                                                      const StreamState *st, SilkRec *srecs, SilkHandoff *handoff, int n,
                                                      int n_streams, SilkShadow *shadow, u32 epoch) {
    silk_parse_kernel_body<32>(descs, arena, st, srecs, handoff, n, n_streams, shadow, epoch);
}
__global__ void __launch_bounds__(64, OG_SPARSE_WAVES) k_silk_parse64(const FrameDesc *__restrict__ descs, const u8 *__restrict__ arena,
                                                        const StreamState *st, SilkRec *srecs, SilkHandoff *handoff, int n,
                                                        int n_streams, SilkShadow *shadow, u32 epoch) {
    silk_parse_kernel_body<64>(descs, arena, st, srecs, handoff, n, n_streams, shadow, epoch);
}

// ... and their parameter half (silk_decode_parameters), ONE (FRAME, CHANNEL) PER LANE: lane l of workgroup g takes channel l / 32
// of frame 32 g + l % 32 -- the record's indices in, the dequantised parameters out, and for pipelined steps the entropy half's
// past of the stream's next frame (`shadow`).  Behind k_silk_parse on the same stream.
#define OG_SPARAMS_WAVES 4
__global__ void __launch_bounds__(64, OG_SPARAMS_WAVES) k_silk_params(const FrameDesc *__restrict__ descs, const StreamState *st, SilkRec *srecs,
                                                                       int n, int n_streams, SilkShadow *shadow, u32 epoch) {
    constexpr int FR = OG_PAR_LANES / 2;
    const int ch = (int)threadIdx.x / FR, f = (int)blockIdx.x * FR + (int)threadIdx.x % FR;
    bool act = f < n;
    FrameDesc d = {0, 0, 0, 0};
    if (act) {
        d = descs[f];
        act = !(d.stream < 0 || d.stream >= n_streams || desc_mode(d.flags) == MODE_CELT || desc_rfc(d.flags));
    }
    SilkShadow *const sh = act && shadow ? &shadow[d.stream] : nullptr;
    const SilkParPast past(act ? &st[d.stream] : st, sh, epoch);
    const int mode = desc_mode(d.flags), channels = desc_channels(d.flags);
    SilkParTask t;
    t.skip = 1;
    if (act) silk_params_channel(past, mode, desc_bandwidth(d.flags), channels, &srecs[f], ch, t);
    OG_FULL_SYNC(); // every lane has read what it needs of the past: now the lanes of a frame may overwrite it
    if (act) silk_params_shadow(past, t, channels, &srecs[f], ch, sh, epoch);
}

#define OG_PARSE_KERNEL_NAME k_celt_parse
#include "og_parse_kernel.hpp"
// ... and with 64 frames per wave, for pipelined steps (og_parse64.hip)
extern "C" void og_launch_celt_parse64(hipStream_t s, int grid, const void *descs, const void *arena, void *streams, void *recs, int n,
                                       int n_streams, const void *handoff, int which, int groups, unsigned *started);
extern "C" int og_celt_parse64_frames(void); // frames per group of that kernel

// Split CELT path, second half: one frame per wave, driven by the parse record.
// (20 ms CELT-only frames are reconstructed by k_celt_recon_fb, og_recon.hip; `rest_only`: skip what that kernel took)
// `empties`: that kernel also finishes the frames without leaves (a pipelined CELT-only step: nothing is left for k_celt_recon)
extern "C" void og_launch_celt_recon_fb(hipStream_t s, const void *descs, void *streams, const void *recs, void *rout, int n,
                                        int n_streams, int hybrid, unsigned *started, int empties);
extern "C" int og_celt_recon_fb_signals(int n); // how often a launch over n frames bumps `started`
// RFC mode (opt-in): every frame of a step, at its true duration, incl. the loss path (og_rfc.hip)
extern "C" void og_launch_decode_rfc(hipStream_t s, const void *descs, const void *arena, void *streams, void *pcm, void *result, int n,
                                     int n_streams, int pcm_stride);
__global__ void __launch_bounds__(64, OG_RECON_WAVES) k_celt_recon(const FrameDesc *__restrict__ descs, StreamState *st,
                                                                      const ParseRec *recs, ReconOut *rout, int n,
                                                                      int n_streams, int hybrid, int rest_only) {
    // rest_only (k_celt_recon_fb ran before): what is left -- frames without leaves (RF_BAD_CELT, RF_SKIP); a record cannot overflow,
    // tests/test_kernel_paths.py -- is almost nothing, so a workgroup
    // looks at 64 slots, one per lane, and reconstructs the few left to it one after the other (see k_decode_step)
    unsigned long long todo = 1ull;
    int base = (int)blockIdx.x;
    if (rest_only) {
        base = (int)blockIdx.x * 64;
        const int f0 = base + (int)threadIdx.x;
        bool mine = false;
        if (f0 < n) {
            const FrameDesc d0 = descs[f0];
            const int m0 = desc_mode(d0.flags);
            if (d0.stream >= 0 && d0.stream < n_streams && (m0 == MODE_CELT || (m0 == MODE_HYBRID && hybrid)) && !desc_rfc(d0.flags)) {
                const u32 fl = recs[f0].flags; // (the lane's own look at recon_fast_eligible's conditions)
                const bool fast = !(fl & (RF_SKIP | RF_BAD_CELT)) && ((fl >> RF_LM_SHIFT) & 3) == 3 && recs[f0].n_words < REC_MAX_WORDS &&
                                  recs[f0].n_leaves <= FAST_MAX_LEAVES;
                mine = !fast && !(m0 == MODE_HYBRID && (fl & RF_SKIP));
            }
        }
        todo = __ballot(mine);
    }
    while (todo) {
        const int f = base + (int)__builtin_ctzll(todo);
        todo &= todo - 1;
        if (f >= n) return;
        const FrameDesc d = descs[f];
        const int mode = desc_mode(d.flags);
        if (d.stream < 0 || d.stream >= n_streams || !(mode == MODE_CELT || (mode == MODE_HYBRID && hybrid)) || desc_rfc(d.flags)) continue;
        if (mode == MODE_HYBRID && (recs[f].flags & RF_SKIP)) continue; // the single-kernel path already reported this frame
#if !defined(OG_PROF_PARSE) && !defined(OG_PROF_SINGLE) && !defined(OG_PROF_SPARSE) && !defined(OG_PROF_SSYNTH)
        OG_PROF_INIT();
#endif
        const int pos = OG_UNI(st[d.stream].celt.ring_pos); // where the frame's first sample goes
        const int ret = celt_recon_wave(&st[d.stream], &recs[f], mode, desc_channels(d.flags), rest_only ? RECON_REST_ONLY : RECON_ALL, desc_mode_after(d.flags));
        if (ret != RECON_NOT_MINE && threadIdx.x == 0) rout[f] = ReconOut{ret, pos};
#if !defined(OG_PROF_PARSE) && !defined(OG_PROF_SINGLE) && !defined(OG_PROF_SPARSE) && !defined(OG_PROF_SSYNTH)
        OG_PROF_FLUSH();
#endif
        __syncthreads();
    }
}

// Split CELT path, third step: de-emphasis (a rounding IIR: strictly serial per channel) and int16 PCM, one
// (frame, channel) per lane, from the samples k_celt_recon appended to the history ring.
// It also hands the reconstruction's result codes (ReconOut) to the caller's array, and -- for a step whose caller named the
// modes it contains (`modes`: bit 0 SILK-only, bit 1 hybrid, bit 2 CELT-only; the kernels of absent modes were not launched,
// `others_ran` = 0 if that includes the kernels that report stream-index errors) -- reports what those kernels would have.
// two int16 lanes of a word added with saturation (v_pk_add_i16 ... clamp)
static __device__ __forceinline__ i32 pk_add_sat_i16(i32 a, i32 b) {
    typedef short s2 __attribute__((ext_vector_type(2)));
    const s2 r = __builtin_elementwise_add_sat(__builtin_bit_cast(s2, a), __builtin_bit_cast(s2, b));
    return __builtin_bit_cast(i32, r);
}
// a wave-uniform pointer, held in scalar registers: a lane's address is then this plus a 32-bit offset of its own, and a loop that walks
// such addresses carries the one offset, not a pointer per access
template <class T>
static __device__ __forceinline__ T *uniform_ptr(T *p) {
    const unsigned long long a = (unsigned long long)p;
    return (T *)((unsigned long long)(u32)__builtin_amdgcn_readfirstlane((int)(u32)a) |
                 (unsigned long long)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(a >> 32)) << 32);
}
// (five waves per SIMD, at most 96 registers, as before the row descriptions left LDS for registers -- 89 now, 92 then; the bound is
// there so that a change which needs more shows as scratch in tests/test_post_budget.py, not as a lost wave)
#define OG_POST_WAVES 5
__global__ void __launch_bounds__(64, OG_POST_WAVES) k_celt_post(const FrameDesc *__restrict__ descs, StreamState *st, const ParseRec *recs,
                                                  const ReconOut *__restrict__ rout, i32 *__restrict__ result, i16 *pcm, int n,
                                                  int n_streams, int channels, int pcm_stride, const SilkHandoff *handoff,
                                                  int modes, int others_ran) {
    // Fast path (two-channel decoder, every row of the wave live, ring positions on a 32-sample boundary): the 64 rows'
    // next 32 samples are fetched as full 128-byte lines by the whole wave (lane = an eighth of a row's line), transposed
    // through LDS to one row per lane for the recurrence, and the PCM goes out the same way (lane = 16 bytes of a frame's
    // interleaved output, a frame's 128 bytes by eight neighbouring lanes; a hybrid frame's SILK PCM comes in likewise).  Anything
    // else takes the row-per-lane path with its 16-byte accesses (celt_post_lane).
    // (Round 3 moved 64-byte pieces: the memory system fetches 128-byte lines, and the other half of a row's line had left the L2
    // again by the time its turn came -- 36 KB of traffic per hybrid frame for 15 KB needed, in a kernel that does nothing but move.)
    constexpr int CS = 32, PCS = CS / 4, RSTEP = 64 / PCS; // samples per chunk and row; 16-byte pieces per row; rows between a lane's pieces
    static_assert(RSTEP % 2 == 0, "a lane's rows are all of one channel");
    // ONE buffer, 9,216 bytes, eight LDS granules of 1,280 (round 13: 16 KB, thirteen -- an output buffer of 5 KB and 2 KB of row
    // descriptions besides; what a lane needs of other rows it now asks their lanes for, once, before the loop).  A row's int16
    // outputs go over the first half of the row's own int32 inputs: the recurrence has read a group of eight inputs into registers
    // before it stores the group's four packed words, and they land at or below the words just read.
    // Banks: the recurrence reads and writes 16 bytes per lane, rows 36 words apart -- 36 i mod 64 is a different multiple of four
    // for each of a group's 16 lanes: no conflict.  The PCM stage reads 8 bytes per lane from the left and from the right row, which
    // the compiler fuses into one ds_read2_b64 (32 banks, 16 contiguous lanes per access = two frames): words 72 r0 + 2 q + {0, 1} for
    // two values of r0 -- two runs of 16 banks that start 8 apart, so banks 8 .. 15 are asked twice: two-way, as it was from the
    // output buffer (rows of 20 words, frames 40 words apart: 40 mod 32 = 8, the same pattern).
    // (Next to kernels that are short of LDS.  Measured by padding in round 5: 5 KB more cost the CELT step 0.8 %, mixed pages 0.6 %.
    // Measured in round 14, 16,384 -> 9,216 bytes: the pipelined CELT step 2.5 % shorter, this kernel through 0.25 ms before the
    // reconstruction it runs beside instead of with it; hybrid-256k and mixed pages within their spread.  DESIGN.md 6m.)
    __shared__ __attribute__((aligned(16))) i32 tin[64][CS + 4]; // CS samples per row, rows padded by 16 bytes
    const int lane = (int)threadIdx.x;
    const int t = (int)blockIdx.x * 64 + lane;
    const int f = channels == 2 ? t >> 1 : t, c = channels == 2 ? t & 1 : 0;
    bool live = false, emit = false;
    StreamState *ss = nullptr;
    const i16 *silk = nullptr;
    int silk_n = 0;
    int pos = 0, stream = 0;
    if (f < n) {
        const FrameDesc d = descs[f];
        stream = d.stream;
        const int mode = desc_mode(d.flags);
        const bool stream_ok = d.stream >= 0 && d.stream < n_streams;
        if (!(modes >> (d.flags & 3) & 1) || (!stream_ok && !others_ran)) { // (a frame the caller's mode set left out is an error, not a skip)
            if (c == 0) result[f] = BAD_ARG;
        } else if (stream_ok && (mode == MODE_CELT || (mode == MODE_HYBRID && handoff)) && !desc_rfc(d.flags)) {
            const u32 rf = recs[f].flags;
            if (!(mode == MODE_HYBRID && (rf & RF_SKIP))) { // (those the single-kernel path has reported already)
                const ReconOut ro = rout[f];
                if (c == 0) result[f] = ro.ret;
                if (!(rf & (RF_SKIP | RF_BAD_CELT))) {
                    live = true;
                    ss = &st[d.stream];
                    emit = ro.ret >= 0;
                    pos = ro.pos & RING_MASK;
                    if (mode == MODE_HYBRID) {
                        silk = handoff[f].pcm;
                        silk_n = 960 * desc_channels(d.flags);
                    }
                }
            }
        }
    }
    i16 *out = pcm + (size_t)(f < n ? f : 0) * pcm_stride;
    // (... and the stream states within 2^32 16-byte pieces of each other, 64 GB: the fast path keeps a ring's place as one word)
    const bool fast = channels == 2 && (size_t)n_streams * sizeof(StreamState) <= (size_t)16 << 32 && __all(live && emit && (pos & (CS - 1)) == 0);
    if (!fast) {
        if (live) celt_post_lane(&ss->celt, c, channels, 960, pos, emit ? out : nullptr, silk, silk_n);
        return;
    }
    // this lane's share of the cooperative traffic: piece q of rows r0, r0 + RSTEP, .. -- their rings and positions from the lanes
    // that own them (row r: channel r & 1 = r0 & 1 of frame r >> 1 of the wave; every row is live here, so its stream index is good).
    // Kept small, for the 32 registers of pieces in flight beside them: a ring as its distance from `st` in 16-byte pieces (one word,
    // not a pointer), the positions in chunks of CS samples, four to a word; the lines that follow put the addresses together.
    const int q = lane % PCS, r0 = lane / PCS;
    constexpr u32 STATE16 = sizeof(StreamState) / 16, RING16 = (offsetof(StreamState, celt) + offsetof(CeltState, ring)) / 16, CHAN16 = RING * 4 / 16;
    static_assert(sizeof(StreamState) % 16 == 0 && (offsetof(StreamState, celt) + offsetof(CeltState, ring)) % 16 == 0 && RING / CS <= 256, "ring pieces");
    u32 row16[PCS], at_chunk[PCS / 4] = {};
#pragma unroll
    for (int k = 0; k < PCS; k++) {
        row16[k] = (u32)__shfl(stream, r0 + RSTEP * k) * STATE16 + RING16 + (u32)(r0 & 1) * CHAN16 + (u32)q;
        at_chunk[k / 4] |= (u32)(__shfl(pos, r0 + RSTEP * k) / CS) << (8 * (k % 4));
    }
    // piece q of chunk `chunk` of the frame in row k of this lane's: 16 bytes, on a 16-byte boundary
    auto piece = [&](int k, int chunk) -> og_v4i {
        const u32 at = ((at_chunk[k / 4] >> (8 * (k % 4)) & 255u) + (u32)chunk) & (u32)(RING / CS - 1);
        return *reinterpret_cast<const og_v4i *>(reinterpret_cast<const char *>(st) + (size_t)(row16[k] + at * (CS * 4 / 16)) * 16);
    };
    // ... and of the PCM's: piece q of frames r0, r0 + RSTEP, .. -- how much SILK PCM each has, in units of 960 (0: not a hybrid frame)
    const size_t f_wave = (size_t)blockIdx.x * 32; // the wave's first frame
    const u32 lane_pcm = 2u * (u32)(r0 * pcm_stride + 8 * q), lane_sk = (u32)r0 * (u32)sizeof(SilkHandoff) + 16u * (u32)q; // bytes
    u32 sk_960 = 0;
#pragma unroll
    for (int k = 0; k < PCS / 2; k++) sk_960 |= (u32)(__shfl(silk_n, 2 * (r0 + RSTEP * k)) / 960) << (8 * k);
    og_v4i v[PCS];
#pragma unroll
    for (int k = 0; k < PCS; k++) v[k] = piece(k, 0);
    i32 m = st[stream].celt.deemph[c];
    for (int ch = 0; ch < 960 / CS; ch++) {
        if (ch) __syncthreads(); // (the PCM stage of the chunk before has read its rows)
#pragma unroll
        for (int k = 0; k < PCS; k++) *reinterpret_cast<og_v4i *>(&tin[r0 + RSTEP * k][4 * q]) = v[k];
        if (ch + 1 < 960 / CS) {
#pragma unroll
            for (int k = 0; k < PCS; k++) v[k] = piece(k, ch + 1);
        }
        __syncthreads();
        // the recurrence on this lane's own row (celt.cpp:1965-2055, sig2word16 celt.h:413)
#pragma unroll
        for (int g8 = 0; g8 < CS / 8; g8++) {
            i16 o[8];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const og_v4i sv = *reinterpret_cast<const og_v4i *>(&tin[lane][8 * g8 + 4 * h]);
                // (a hybrid frame's SILK PCM is added where the PCM leaves, below: there a frame's pieces are read by neighbouring
                // lanes as whole lines; read here, one row per lane, every 16 bytes would come from a line of their own)
                i32 tt = sv.x + m;
                m = mul16x32_q15(27853, tt);
                o[4 * h + 0] = (i16)sat16(pshr32(tt, 12));
                tt = sv.y + m;
                m = mul16x32_q15(27853, tt);
                o[4 * h + 1] = (i16)sat16(pshr32(tt, 12));
                tt = sv.z + m;
                m = mul16x32_q15(27853, tt);
                o[4 * h + 2] = (i16)sat16(pshr32(tt, 12));
                tt = sv.w + m;
                m = mul16x32_q15(27853, tt);
                o[4 * h + 3] = (i16)sat16(pshr32(tt, 12));
            }
            og_v4i w;
            w.x = (i32)((u32)(u16)o[0] | (u32)(u16)o[1] << 16);
            w.y = (i32)((u32)(u16)o[2] | (u32)(u16)o[3] << 16);
            w.z = (i32)((u32)(u16)o[4] | (u32)(u16)o[5] << 16);
            w.w = (i32)((u32)(u16)o[6] | (u32)(u16)o[7] << 16);
            *reinterpret_cast<og_v4i *>(&tin[lane][4 * g8]) = w; // (outputs 8 g8 .. 8 g8 + 7, over inputs 4 g8 .. 4 g8 + 3: read above)
        }
        __syncthreads();
        // PCM: frame fr's CS samples x 2 channels = 128 contiguous bytes; this lane writes piece q (samples 4q .. 4q+3) of frames
        // r0, r0 + RSTEP, ..
#pragma unroll
        for (int k = 0; k < PCS / 2; k++) {
            const int fr = r0 + RSTEP * k; // frame within the wave: rows 2 fr (left) and 2 fr + 1 (right)
            const og_v2u L = *reinterpret_cast<const og_v2u *>(&tin[2 * fr][2 * q]); // (int16 outputs 4 q .. 4 q + 3 of the row)
            const og_v2u R = *reinterpret_cast<const og_v2u *>(&tin[2 * fr + 1][2 * q]);
            og_v4i w;
            w.x = (i32)((L.x & 0xffffu) | R.x << 16);
            w.y = (i32)(L.x >> 16 | (R.x & 0xffff0000u));
            w.z = (i32)((L.y & 0xffffu) | R.y << 16);
            w.w = (i32)(L.y >> 16 | (R.y & 0xffff0000u));
            const int at = (CS * ch + 4 * q) * 2; // the piece's place in the frame's interleaved PCM -- and in its SILK PCM (Q3: by linear index)
            // (addresses as a wave-uniform base -- frame RSTEP k of the wave, sample CS ch -- plus the lane's 32-bit offset: one register
            // for all of them, where a pointer per frame was two each, carried through the loop)
            if (at < 960 * (int)(sk_960 >> (8 * k) & 255u)) { // SAT16(celt + silk), two samples per saturating packed add
                const char *const sk = uniform_ptr(reinterpret_cast<const char *>(handoff[f_wave + RSTEP * k].pcm + 2 * CS * ch));
                const og_v4i a = *reinterpret_cast<const og_v4i *>(sk + lane_sk);
                w.x = pk_add_sat_i16(w.x, a.x);
                w.y = pk_add_sat_i16(w.y, a.y);
                w.z = pk_add_sat_i16(w.z, a.z);
                w.w = pk_add_sat_i16(w.w, a.w);
            }
            char *const to = uniform_ptr(reinterpret_cast<char *>(pcm + (f_wave + RSTEP * k) * pcm_stride + 2 * CS * ch));
            *reinterpret_cast<og_v4i *>(to + lane_pcm) = w;
        }
    }
    st[stream].celt.deemph[c] = m;
}

#include "og_step.hpp"

// ---- the launches of the scheduler (og_step.hpp): frames [f0, f0 + cnt) of step `st` on stream q ---------------------
const size_t og_parse_rec_bytes = sizeof(ParseRec), og_recon_out_bytes = sizeof(ReconOut), og_silk_handoff_bytes = sizeof(SilkHandoff),
             og_silk_rec_bytes = sizeof(SilkRec);
namespace {
struct StepRange { // the step's tables at frame f0 (hand-off and SILK records: null when the step has none)
    const FrameDesc *dd;
    i16 *pp;
    i32 *rr;
    ParseRec *recs;
    ReconOut *rout;
    SilkHandoff *hh;
    SilkRec *srecs;
    StepRange(const Step &st, size_t f0)
        : dd((const FrameDesc *)st.descs + f0), pp((i16 *)st.pcm + f0 * (size_t)st.pcm_stride), rr((i32 *)st.result + f0),
          recs((ParseRec *)st.recs + f0), rout((ReconOut *)st.rout + f0), hh(st.handoff ? (SilkHandoff *)st.handoff + f0 : nullptr),
          srecs(st.srecs ? (SilkRec *)st.srecs + f0 : nullptr) {}
};
} // namespace
void launch_stream_stall(opusgpu_ctx *ctx, hipStream_t q) {
    hipLaunchKernelGGL(k_stream_stall, dim3(1), dim3(64), 0, q, ctx->stall_ticks, (int)OG_STALL_MAX_SPINS);
}
void launch_decode_rfc(opusgpu_ctx *ctx, hipStream_t q, const Step &st) {
    og_launch_decode_rfc(q, st.descs, st.arena, ctx->d_streams, st.pcm, st.result, st.n, ctx->n_streams, st.pcm_stride);
}
void launch_decode_step(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, int pass) {
    const StepRange r(st, f0);
    hipLaunchKernelGGL(k_decode_step, dim3(pass == 2 ? (cnt + 63) / 64 : cnt), dim3(64), 0, q, r.dd, (const u8 *)st.arena, ctx->d_streams, r.pp,
                       r.rr, cnt, ctx->n_streams, st.pcm_stride, pass ? 1 : 0, pass == 2 ? r.hh : nullptr,
                       (const SilkRec *)(pass == 2 ? r.srecs : nullptr), pass == 2 ? 1 : 0);
}
void launch_silk_parse(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch) {
    const StepRange r(st, f0);
    hipLaunchKernelGGL(k_silk_parse, dim3((cnt + 31) / 32), dim3(64), 0, q, r.dd, (const u8 *)st.arena, (const StreamState *)ctx->d_streams,
                       r.srecs, r.hh, cnt, ctx->n_streams, (SilkShadow *)shadow, epoch);
}
void launch_silk_parse64(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch) {
    const StepRange r(st, f0);
    hipLaunchKernelGGL(k_silk_parse64, dim3((cnt + 63) / 64), dim3(64), 0, q, r.dd, (const u8 *)st.arena, (const StreamState *)ctx->d_streams,
                       r.srecs, r.hh, cnt, ctx->n_streams, (SilkShadow *)shadow, epoch);
}
void launch_silk_params(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, void *shadow, uint32_t epoch) {
    const StepRange r(st, f0);
    hipLaunchKernelGGL(k_silk_params, dim3((cnt + OG_PAR_LANES / 2 - 1) / (OG_PAR_LANES / 2)), dim3(64), 0, q, r.dd,
                       (const StreamState *)ctx->d_streams, r.srecs, cnt, ctx->n_streams, (SilkShadow *)shadow, epoch);
}
int celt_parse_early_grid(const opusgpu_ctx *ctx, int cnt, bool wide) {
    const int per = (wide ? og_celt_parse64_frames() : OG_PL_FRAMES) * ctx->parse_groups;
    return (cnt + per - 1) / per;
}
void launch_celt_parse(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool wide, bool early) {
    const StepRange r(st, f0);
    const int which = early ? (int)PARSE_CELT_ONLY : (int)PARSE_ALL, groups = early ? ctx->parse_groups : 1;
    const int per = wide ? og_celt_parse64_frames() : OG_PL_FRAMES;
    const int grid = early ? celt_parse_early_grid(ctx, cnt, wide) : (cnt + per - 1) / per;
    u32 *const started = early ? ctx->sp.d_started : nullptr;
    if (wide)
        og_launch_celt_parse64(q, grid, r.dd, st.arena, ctx->d_streams, r.recs, cnt, ctx->n_streams, r.hh, which, groups, started);
    else
        hipLaunchKernelGGL(k_celt_parse, dim3(grid), dim3(64 * OG_PL_WAVES), 0, q, r.dd, (const u8 *)st.arena, ctx->d_streams, r.recs, cnt,
                           ctx->n_streams, (const SilkHandoff *)r.hh, which, groups, started);
}
void launch_celt_recon_fb(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool counts_in) {
    const StepRange r(st, f0);
    // A pipelined CELT-only step (the only caller that counts in; no hand-off, so no hybrid frames): the frames the kernel of 20 ms
    // frames leaves are CELT frames of at most one byte, which it finishes itself (`empties`, og_recon.hip) -- the leftover launch
    // behind it was a link of 1,024 workgroups with nothing to do in the chain from one reconstruction to the next.
    // Every other step keeps that launch: hybrid frames, in-order steps (OPUSGPU_REST_IN_FB=0: pipelined CELT-only steps too).
    ctx->recon_fb_took_rest = counts_in && !r.hh && st.modes == 4 && og_debug().rest_in_fb;
    og_launch_celt_recon_fb(q, r.dd, ctx->d_streams, r.recs, r.rout, cnt, ctx->n_streams, r.hh ? 1 : 0, counts_in ? ctx->sp.d_started + 16 : nullptr,
                            ctx->recon_fb_took_rest ? 1 : 0);
}
void launch_celt_recon(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt) {
    if (ctx->fast_recon && ctx->recon_fb_took_rest) { // (launch_celt_recon_fb, called right before this for the same frames)
        ctx->recon_fb_took_rest = false;
        return;
    }
    const StepRange r(st, f0);
    hipLaunchKernelGGL(k_celt_recon, dim3(ctx->fast_recon ? (cnt + 63) / 64 : cnt), dim3(64), 0, q, r.dd, ctx->d_streams, (const ParseRec *)r.recs,
                       r.rout, cnt, ctx->n_streams, r.hh ? 1 : 0, ctx->fast_recon);
}
void launch_celt_post(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, bool others) {
    const StepRange r(st, f0);
    hipLaunchKernelGGL(k_celt_post, dim3((cnt * ctx->channels + 63) / 64), dim3(64), 0, q, r.dd, ctx->d_streams, (const ParseRec *)r.recs,
                       (const ReconOut *)r.rout, r.rr, r.pp, cnt, ctx->n_streams, ctx->channels, st.pcm_stride, (const SilkHandoff *)r.hh, st.modes,
                       others ? 1 : 0);
}
void launch_silk_synth(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt, int nb_done) {
    const StepRange r(st, f0);
    og_launch_silk_synth(q, r.dd, st.arena, ctx->d_streams, r.pp, r.rr, cnt, ctx->n_streams, st.pcm_stride, r.hh, r.srecs, nb_done);
}
void launch_silk_synth_nb(opusgpu_ctx *ctx, hipStream_t q, const Step &st, size_t f0, int cnt) {
    const StepRange r(st, f0);
    og_launch_silk_synth_nb(q, r.dd, st.arena, ctx->d_streams, r.pp, r.rr, cnt, ctx->n_streams, st.pcm_stride, r.hh, r.srecs, 1);
}


extern "C" {


int opusgpu_version(void) { return 100; }

int opusgpu_ctx_create(int device, opusgpu_ctx **out) {
    if (!out || device < 0) return OPUSGPU_BAD_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device >= count) return OPUSGPU_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return OPUSGPU_ERR_NO_DEVICE;
    // the code object is gfx950-only: make sure the kernel image is loadable on this device
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(k_decode_step)) != hipSuccess) {
        (void)hipGetLastError();
        return OPUSGPU_ERR_NO_DEVICE;
    }
    opusgpu_ctx *ctx = new (std::nothrow) opusgpu_ctx();
    if (!ctx) return OPUSGPU_ALLOC_FAIL;
    ctx->device = device;
    ctx->split_celt = og_debug().split; // (og_debug.hpp: A/B switches, read from the environment once per process)
    ctx->split_hybrid = og_debug().split_hybrid;
    ctx->fast_recon = og_debug().fast_recon;
    ctx->parse_groups = og_debug().parse_groups;
    ctx->host_parts = og_debug().host_parts;
    if (og_debug().stall_us) {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
            (void)hipGetLastError();
            delete ctx;
            return OPUSGPU_ERR_HIP;
        }
        ctx->stall_ticks = (long long)og_debug().stall_us * khz / 1000;
    }
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return OPUSGPU_ERR_HIP;
    }
    *out = ctx;
    return OPUSGPU_OK;
}

void opusgpu_ctx_destroy(opusgpu_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(ctx->d_streams);
    (void)hipFree(ctx->d_descs);
    (void)hipFree(ctx->d_arena);
    (void)hipFree(ctx->d_pcm);
    (void)hipFree(ctx->d_result);
    pipeline_destroy(ctx);
    for (int i = 0; i < 6; i++) {
        (void)hipFree(ctx->d_recs[i]);
        (void)hipFree(ctx->d_rout[i]);
    }
    for (int i = 0; i < OG_SILK_SETS; i++) {
        (void)hipFree(ctx->d_handoff[i]);
        (void)hipFree(ctx->d_srecs[i]);
    }
    (void)hipFree(ctx->d_shadow);
    (void)hipHostFree(ctx->h_pcm);
    (void)hipHostFree(ctx->h_res);
    (void)hipHostFree(ctx->h_arena);
    (void)hipHostFree(ctx->h_descs);
    (void)hipFree(ctx->d_crc_tables);
    for (hipEvent_t e : ctx->ev_piece)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_part)
        if (e) (void)hipEventDestroy(e);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *opusgpu_last_error(const opusgpu_ctx *ctx) { return ctx ? ctx->err : "no context"; }
int opusgpu_set_mode(opusgpu_ctx *ctx, int mode) {
    if (!ctx || (mode != OPUSGPU_MODE_REFERENCE && mode != OPUSGPU_MODE_RFC)) return OPUSGPU_BAD_ARG;
    ctx->mode = mode;
    return OPUSGPU_OK;
}
int opusgpu_get_mode(const opusgpu_ctx *ctx) { return ctx ? ctx->mode : OPUSGPU_MODE_REFERENCE; }
int opusgpu_set_pipeline(opusgpu_ctx *ctx, int on) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (on)
        if (int rc = pipeline_create(ctx)) return rc;
    if ((on != 0) != (ctx->pipeline != 0)) { // switching: from an idle device (steps of either kind may be queued on any stream)
        HIPCHK(ctx, hipDeviceSynchronize());
        ctx->sp.drained();
        ctx->sp.last_kind = 0;
        ctx->sp.shadow_epoch++;
    }
    ctx->pipeline = on ? 1 : 0;
    return OPUSGPU_OK;
}
int opusgpu_get_pipeline(const opusgpu_ctx *ctx) { return ctx ? ctx->pipeline : 0; }
size_t opusgpu_stream_state_bytes(void) { return sizeof(StreamState); }
int opusgpu_stream_count(const opusgpu_ctx *ctx) { return ctx ? ctx->n_streams : 0; }
int opusgpu_stream_channels(const opusgpu_ctx *ctx) { return ctx ? ctx->channels : 0; }

int opusgpu_streams_reset(opusgpu_ctx *ctx, int first, int count, int full) {
    if (!ctx || first < 0 || count < 0 || first + count > ctx->n_streams) return OPUSGPU_BAD_ARG;
    if (count == 0) return OPUSGPU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = sync_in_flight(ctx)) return rc; // whatever pipelined steps still have in flight works on the state this resets
    ctx->sp.drained();                           // (the reset below, on the context's stream, is synchronous)
    ctx->sp.shadow_epoch++; // (the parse kernel's copies of these streams' past are stale now)
    hipLaunchKernelGGL(k_stream_init, dim3(count), dim3(64), 0, ctx->stream, ctx->d_streams, first, count, ctx->channels,
                       full ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    // (both kinds of reset forget the last packet -- src/opus_decoder.cpp:382-390 clears frame_size and the like -- a loss right
    // after one conceals 20 ms, of zeros)
    for (int i = first; i < first + count; i++) ctx->last_count[i] = ctx->last_flags[i] = 0;
    return OPUSGPU_OK;
}

int opusgpu_streams_alloc(opusgpu_ctx *ctx, int n_streams, int channels) {
    if (!ctx || n_streams <= 0 || (channels != 1 && channels != 2)) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = sync_in_flight(ctx)) return rc; // pipelined steps still in flight work on the state that is about to be freed
    if (ctx->d_streams) {
        HIPCHK(ctx, hipFree(ctx->d_streams));
        ctx->d_streams = nullptr;
        ctx->n_streams = 0;
    }
    hipError_t e = hipMalloc((void **)&ctx->d_streams, sizeof(StreamState) * (size_t)n_streams);
    if (e != hipSuccess) return fail(ctx, OPUSGPU_ALLOC_FAIL, "hipMalloc(streams)", e);
    if (ctx->d_shadow) HIPCHK(ctx, hipFree(ctx->d_shadow));
    ctx->d_shadow = nullptr;
    e = hipMalloc(&ctx->d_shadow, sizeof(SilkShadow) * (size_t)n_streams);
    if (e != hipSuccess) return fail(ctx, OPUSGPU_ALLOC_FAIL, "hipMalloc(shadow)", e);
    HIPCHK(ctx, hipMemset(ctx->d_shadow, 0, sizeof(SilkShadow) * (size_t)n_streams)); // (epoch 0: never current)
    ctx->sp.shadow_epoch++;
    ctx->n_streams = n_streams;
    ctx->channels = channels;
    ctx->last_count.assign((size_t)n_streams, 0);
    ctx->last_flags.assign((size_t)n_streams, 0);
    return opusgpu_streams_reset(ctx, 0, n_streams, 1);
}

int opusgpu_dev_alloc(opusgpu_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (16 bytes more than asked for: an arena made with this call then has the tail the kernels' 16-byte packet fetches may touch)
    if (bytes > SIZE_MAX - 16) return OPUSGPU_ALLOC_FAIL;
    hipError_t e = hipMalloc(dptr, bytes + 16);
    if (e != hipSuccess) return fail(ctx, OPUSGPU_ALLOC_FAIL, "hipMalloc", e);
    return OPUSGPU_OK;
}
int opusgpu_dev_free(opusgpu_ctx *ctx, void *dptr) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipFree(dptr));
    return OPUSGPU_OK;
}
int opusgpu_memcpy_h2d(opusgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return OPUSGPU_OK;
}
int opusgpu_memcpy_d2h(opusgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = sync_in_flight(ctx)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return OPUSGPU_OK;
}


int opusgpu_decode_step_device(opusgpu_ctx *ctx, int n, const void *d_descs, const void *d_arena, void *d_pcm,
                               void *d_result, void *hip_stream) {
    return decode_step_impl(ctx, n, d_descs, d_arena, d_pcm, d_result, hip_stream, true);
}
int opusgpu_decode_step_device_modes(opusgpu_ctx *ctx, int n, const void *d_descs, const void *d_arena, void *d_pcm,
                                     void *d_result, void *hip_stream, int modes) {
    if (modes <= 0 || modes > 15 || (modes & 7) == 0) return OPUSGPU_BAD_ARG;
    return decode_step_impl(ctx, n, d_descs, d_arena, d_pcm, d_result, hip_stream, true, modes);
}
int opusgpu_decode_steps_device(opusgpu_ctx *ctx, int n_steps, const int32_t *n, const void *const *d_descs, const void *const *d_arena,
                                void *const *d_pcm, void *const *d_result, void *hip_stream, int modes) {
    if (!ctx || n_steps < 0 || modes < 0 || modes > 7) return OPUSGPU_BAD_ARG;
    if (n_steps == 0) return OPUSGPU_OK;
    if (!n || !d_descs || !d_arena || !d_pcm || !d_result) return OPUSGPU_BAD_ARG;
    // Everything that can refuse a step is looked at BEFORE the first launch: step k of a window holds its reconstruction and its
    // de-emphasis until workgroups of step k + 1 have started (hipStreamWaitValue32 below), so a call that stopped between the two
    // would leave waits nothing satisfies.
    if (!ctx->d_streams) return OPUSGPU_BAD_ARG;
    int max_n = 0;
    for (int k = 0; k < n_steps; k++) {
        if (n[k] < 0) return OPUSGPU_BAD_ARG;
        if (n[k] > 0 && (!d_descs[k] || !d_arena[k] || ((uintptr_t)d_arena[k] & 15) || !d_pcm[k] || !d_result[k])) return OPUSGPU_BAD_ARG;
        max_n = OG_MAX(max_n, n[k]);
    }
    if (max_n == 0) return OPUSGPU_OK;
    return decode_window(ctx, n_steps, n, max_n, d_descs, d_arena, d_pcm, d_result, hip_stream, modes ? modes : 7);
}

#ifdef OG_PROF
// profiling builds only: per-section wave-cycle totals of k_celt_recon (see OG_MARK), optionally cleared after the read
extern "C" int og_recon_fb_prof(unsigned long long *out64, int reset);
extern "C" int og_rfc_prof(unsigned long long *out64, int reset);
extern "C" int og_ssynth_prof(unsigned long long *out64, int reset);
extern "C" int og_ssynth_nb_prof(unsigned long long *out64, int reset);
int opusgpu_debug_prof(unsigned long long *out64, int reset) {
    unsigned long long fb[64], rf[64];
    if (og_recon_fb_prof(fb, reset) != 0 || og_rfc_prof(rf, reset) != 0) return -1;
    for (int i = 0; i < 64; i++) fb[i] += rf[i];
    if (og_ssynth_prof(rf, reset) != 0) return -1;
    for (int i = 0; i < 64; i++) fb[i] += rf[i];
    if (og_ssynth_nb_prof(rf, reset) != 0) return -1;
    for (int i = 0; i < 64; i++) fb[i] += rf[i];
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * 64) != hipSuccess) return -1;
    for (int i = 0; i < 64; i++) out64[i] += fb[i];
    if (reset) {
        unsigned long long z[64] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

int opusgpu_pages_crc_device(opusgpu_ctx *ctx, int n_pages, const void *d_blob, const void *d_offsets, const void *d_lens,
                             void *d_status, void *hip_stream) {
    if (!ctx || n_pages < 0) return OPUSGPU_BAD_ARG;
    if (n_pages == 0) return OPUSGPU_OK;
    if (!d_blob || !d_offsets || !d_lens || !d_status) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    if (!ctx->d_crc_tables) { // t[0] = the byte table; t[j][i] = t[j-1][i] advanced by one zero byte
        static u32 t[8][256];
        for (u32 i = 0; i < 256; i++) {
            u32 r = i << 24;
            for (int k = 0; k < 8; k++) r = (r & 0x80000000u) ? (r << 1) ^ 0x04c11db7u : r << 1;
            t[0][i] = r;
        }
        for (int j = 1; j < 8; j++)
            for (u32 i = 0; i < 256; i++) t[j][i] = (t[j - 1][i] << 8) ^ t[0][t[j - 1][i] >> 24];
        if (hipMalloc((void **)&ctx->d_crc_tables, sizeof(t)) != hipSuccess) return OPUSGPU_ALLOC_FAIL;
        HIPCHK(ctx, hipMemcpy(ctx->d_crc_tables, t, sizeof(t), hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_pages_crc, dim3((n_pages + 255) / 256), dim3(256), 0, s, (const u8 *)d_blob, (const long long *)d_offsets,
                       (const i32 *)d_lens, (i32 *)d_status, n_pages, (const u32 *)ctx->d_crc_tables);
    HIPCHK(ctx, hipGetLastError());
    return OPUSGPU_OK;
}

int opusgpu_output_stage_device(opusgpu_ctx *ctx, int n_blocks, int block_samples, const void *d_pcm, long long pcm_stride,
                                const void *d_valid, int valid_all, const void *d_cfgs, opusgpu_output_cfg cfg, void *d_i2s,
                                long long i2s_stride, void *hip_stream) {
    if (!ctx || n_blocks < 0 || block_samples < 0) return OPUSGPU_BAD_ARG;
    if (n_blocks == 0 || block_samples == 0) return OPUSGPU_OK;
    if (!d_pcm || !d_i2s || pcm_stride < 0 || i2s_stride < 0) return OPUSGPU_BAD_ARG;
    if (!d_valid && (valid_all < 0 || valid_all > block_samples)) return OPUSGPU_BAD_ARG;
    // the reference's setters refuse anything else (setBitsPerSample / setChannels, src/main.cpp:119-132)
    if (!d_cfgs && ((cfg.bits != 8 && cfg.bits != 16) || (cfg.channels != 1 && cfg.channels != 2))) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    // words a block can make: 8-bit mono plays two per sample; with per-block settings any block might
    const int max_words = (d_cfgs || (cfg.bits == 8 && cfg.channels == 1)) ? 2 * block_samples : block_samples;
    const int units = (max_words + 3) / 4;
    const long long n_units = (long long)units * n_blocks;
    const int vec_ok = ((uintptr_t)d_pcm % 16 == 0 && pcm_stride % 8 == 0 && (uintptr_t)d_i2s % 16 == 0 && i2s_stride % 4 == 0) ? 1 : 0;
    OutputCfg c;
    memcpy(&c, &cfg, sizeof c);
    hipLaunchKernelGGL(k_output_stage, dim3((unsigned)((n_units + 255) / 256)), dim3(256), 0, s, (const i16 *)d_pcm, pcm_stride,
                       (const i32 *)d_valid, valid_all, block_samples, (const OutputCfg *)d_cfgs, c, (u32 *)d_i2s, i2s_stride, units,
                       n_units, vec_ok);
    HIPCHK(ctx, hipGetLastError());
    return OPUSGPU_OK;
}

int opusgpu_synchronize(opusgpu_ctx *ctx) {
    if (!ctx) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return OPUSGPU_OK;
}

int opusgpu_event_create(opusgpu_ctx *ctx, void **event) {
    if (!ctx || !event) return OPUSGPU_BAD_ARG;
    hipEvent_t e;
    HIPCHK(ctx, hipEventCreate(&e));
    *event = (void *)e;
    return OPUSGPU_OK;
}
int opusgpu_event_record(opusgpu_ctx *ctx, void *event) {
    if (!ctx || !event) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipEventRecord((hipEvent_t)event, ctx->stream));
    return OPUSGPU_OK;
}
int opusgpu_event_elapsed_ms(opusgpu_ctx *ctx, void *start, void *stop, float *ms) {
    if (!ctx || !start || !stop || !ms) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipEventSynchronize((hipEvent_t)stop));
    HIPCHK(ctx, hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return OPUSGPU_OK;
}
int opusgpu_event_destroy(opusgpu_ctx *ctx, void *event) {
    if (!ctx || !event) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipEventDestroy((hipEvent_t)event));
    return OPUSGPU_OK;
}

// ---- uploads NEXT TO the decode (the ingest of the next batch of pages under the decode of this one).
// The upload runs on the context's copy stream, never on the decode stream: a host thread demuxes batch b + 1 and queues its
// tables and packet bytes here while the caller's thread has batch b's steps in flight; the fence event orders the two.
static std::mutex g_copy_stream_mutex;
static int copy_stream_of(opusgpu_ctx *ctx, hipStream_t *out) {
    std::lock_guard<std::mutex> lock(g_copy_stream_mutex);
    if (!ctx->copy_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    *out = ctx->copy_stream;
    return OPUSGPU_OK;
}
int opusgpu_upload_async(opusgpu_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx || (bytes && (!dst || !src))) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t cs;
    if (int rc = copy_stream_of(ctx, &cs)) return rc;
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs));
    return OPUSGPU_OK;
}
int opusgpu_upload_fence(opusgpu_ctx *ctx, void *event) {
    if (!ctx || !event) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t cs;
    if (int rc = copy_stream_of(ctx, &cs)) return rc;
    HIPCHK(ctx, hipEventRecord((hipEvent_t)event, cs));
    return OPUSGPU_OK;
}
int opusgpu_stream_wait_event(opusgpu_ctx *ctx, void *event, void *hip_stream) {
    if (!ctx || !event) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamWaitEvent(hip_stream ? (hipStream_t)hip_stream : ctx->stream, (hipEvent_t)event, 0));
    // the context's own stream: the streams pipelined steps run ahead on wait too -- what is behind the event (an upload of step
    // tables, opusgpu_upload_fence) is then as good as resident for every kernel of the steps queued after this call
    if ((!hip_stream || (hipStream_t)hip_stream == ctx->stream) && ctx->sp.parse_stream) {
        HIPCHK(ctx, hipStreamWaitEvent(ctx->sp.parse_stream, (hipEvent_t)event, 0));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->sp.recon_stream, (hipEvent_t)event, 0));
    }
    return OPUSGPU_OK;
}
int opusgpu_event_synchronize(opusgpu_ctx *ctx, void *event) {
    if (!ctx || !event) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipEventSynchronize((hipEvent_t)event));
    return OPUSGPU_OK;
}
// Caller-owned host buffers made DMA-able in place (page-locked): uploads from and PCM copies into registered memory run at
// the full PCIe rate without the staging copy (opusgpu_decode_packets notices registered PCM buffers by itself).
int opusgpu_host_register(opusgpu_ctx *ctx, void *ptr, size_t bytes) {
    if (!ctx || !ptr || !bytes) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return fail(ctx, OPUSGPU_ALLOC_FAIL, "hipHostRegister", e);
    std::lock_guard<std::mutex> lock(ctx->registered_mutex);
    ctx->registered.emplace_back((uintptr_t)ptr, bytes);
    return OPUSGPU_OK;
}
int opusgpu_host_unregister(opusgpu_ctx *ctx, void *ptr) {
    if (!ctx || !ptr) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    {
        std::lock_guard<std::mutex> lock(ctx->registered_mutex);
        for (size_t i = 0; i < ctx->registered.size(); i++)
            if (ctx->registered[i].first == (uintptr_t)ptr) {
                ctx->registered.erase(ctx->registered.begin() + i);
                break;
            }
    }
    HIPCHK(ctx, hipHostUnregister(ptr));
    return OPUSGPU_OK;
}

int opusgpu_stream_state_get(opusgpu_ctx *ctx, int index, void *dst, size_t bytes) {
    if (!ctx || !dst || index < 0 || index >= ctx->n_streams || bytes > sizeof(StreamState)) return OPUSGPU_BAD_ARG;
    return opusgpu_memcpy_d2h(ctx, dst, &ctx->d_streams[index], bytes);
}

int opusgpu_stream_pitch_get(opusgpu_ctx *ctx, int index, int32_t out[4]) {
    if (!ctx || !out || index < 0 || index >= ctx->n_streams) return OPUSGPU_BAD_ARG;
    int32_t head[2], ch0[3]; // (channels, prev_mode); (lagPrev .. fs_kHz are not adjacent: three small copies, one synchronisation)
    if (int rc = opusgpu_memcpy_d2h(ctx, head, &ctx->d_streams[index], sizeof(head))) return rc;
    const SilkChannel *c = &ctx->d_streams[index].silk.ch[0];
    HIPCHK(ctx, hipMemcpy(&ch0[0], &c->prevSignalType, 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&ch0[1], &c->lagPrev, 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&ch0[2], &c->fs_kHz, 4, hipMemcpyDeviceToHost));
    out[0] = head[1];
    out[1] = ch0[0];
    out[2] = ch0[1];
    out[3] = ch0[2];
    return OPUSGPU_OK;
}

int opusgpu_debug_stage_taps(opusgpu_ctx *ctx, int slot, opusgpu_stage_taps *out) {
    if (!ctx || !out || slot < 0 || slot >= ctx->last_n || !ctx->last_descs) return OPUSGPU_BAD_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = sync_in_flight(ctx)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memset(out, 0, sizeof(*out));
    FrameDesc d;
    HIPCHK(ctx, hipMemcpy(&d, (const FrameDesc *)ctx->last_descs + slot, sizeof(d), hipMemcpyDeviceToHost));
    if (d.stream < 0 || d.stream >= ctx->n_streams) return OPUSGPU_BAD_ARG;
    const int mode = MODE_SILK + (d.flags & 3);
    std::unique_ptr<StreamState> st(new (std::nothrow) StreamState);
    if (!st) return OPUSGPU_ALLOC_FAIL;
    HIPCHK(ctx, hipMemcpy(st.get(), &ctx->d_streams[d.stream], sizeof(StreamState), hipMemcpyDeviceToHost));
    if (mode != MODE_SILK && ctx->last_recs) {
        std::unique_ptr<ParseRec> r(new (std::nothrow) ParseRec);
        if (!r) return OPUSGPU_ALLOC_FAIL;
        HIPCHK(ctx, hipMemcpy(r.get(), (const ParseRec *)ctx->last_recs + slot, sizeof(ParseRec), hipMemcpyDeviceToHost));
        out->celt_valid = 1;
        out->celt_ret = r->ret;
        out->silence = (r->flags & RF_SILENCE) != 0;
        out->transient = (r->flags & RF_TRANSIENT) != 0;
        out->lm = (int)(r->flags >> RF_LM_SHIFT) & 3;
        out->spread = (int)(r->flags >> RF_SPREAD_SHIFT) & 3;
        out->dual_stereo = (r->flags & RF_DUAL) != 0;
        out->anti_collapse_on = (r->flags & RF_ANTI_COLLAPSE) != 0;
        out->intensity = r->intensity;
        out->pf_pitch = r->pf_pitch;
        out->pf_gain = r->pf_gain;
        out->pf_tapset = r->pf_tapset;
        out->n_leaves = r->n_leaves;
        out->celt_rng_final = r->rng_final;
        memcpy(out->bandE, r->bandE, sizeof(out->bandE));
        memcpy(out->pulses, r->pulses, sizeof(out->pulses));
        memcpy(out->tf_res, r->tf_res, sizeof(out->tf_res));
    }
    const CeltState &c = st->celt;
    for (int ch = 0; ch < 2; ch++) {
        for (int i = 0; i < 960; i++) out->syn_post[ch][i] = c.ring[ch][(c.ring_pos - 960 + i) & RING_MASK];
        for (int i = 0; i < 60; i++) out->overlap_tail[ch][i] = c.tail[ch][i];
    }
    memcpy(out->state_bandE, c.bandE, sizeof(out->state_bandE));
    memcpy(out->state_logE1, c.logE1, sizeof(out->state_logE1));
    memcpy(out->state_logE2, c.logE2, sizeof(out->state_logE2));
    out->state_rng = c.rng;
    out->pf_period = c.pf_period;
    out->pf_gain_state = c.pf_gain;
    out->pf_tapset_state = c.pf_tapset;
    if (mode != MODE_CELT && ctx->last_had_silk_recs && ctx->last_srecs) {
        std::unique_ptr<SilkRec> r(new (std::nothrow) SilkRec);
        if (!r) return OPUSGPU_ALLOC_FAIL;
        HIPCHK(ctx, hipMemcpy(r.get(), (const SilkRec *)ctx->last_srecs + slot, sizeof(SilkRec), hipMemcpyDeviceToHost));
        out->silk_valid = 1;
        out->silk_ret = r->ret;
        out->decode_only_middle = r->decode_only_middle;
        out->ms_pred_q13[0] = r->MS_pred_Q13[0];
        out->ms_pred_q13[1] = r->MS_pred_Q13[1];
        for (int ch = 0; ch < 2; ch++) {
            const SilkRecCh &k = r->ch[ch];
            memcpy(out->silk_ch[ch].pitchL, k.pitchL, sizeof(k.pitchL));
            memcpy(out->silk_ch[ch].Gains_Q16, k.Gains_Q16, sizeof(k.Gains_Q16));
            memcpy(out->silk_ch[ch].PredCoef_Q12, k.PredCoef_Q12, sizeof(k.PredCoef_Q12));
            memcpy(out->silk_ch[ch].LTPCoef_Q14, k.LTPCoef_Q14, sizeof(k.LTPCoef_Q14));
            out->silk_ch[ch].LTP_scale_Q14 = k.LTP_scale_Q14;
            out->silk_ch[ch].signalType = k.signalType;
            out->silk_ch[ch].quantOffsetType = k.quantOffsetType;
        }
    }
    for (int ch = 0; ch < 2; ch++) {
        memcpy(out->silk_out[ch], st->silk.ch[ch].outBuf, sizeof(out->silk_out[ch]));
        memcpy(out->silk_sLPC_Q14[ch], st->silk.ch[ch].sLPC_Q14_buf, sizeof(out->silk_sLPC_Q14[ch]));
        out->silk_fs_kHz[ch] = st->silk.ch[ch].fs_kHz;
    }
    return OPUSGPU_OK;
}

int opusgpu_packet_to_frames(const uint8_t *packet, int32_t len, int32_t stream, opusgpu_frame_desc descs[48]) {
    return opusgpu_packet_to_frames_mode(packet, len, stream, OPUSGPU_MODE_REFERENCE, descs);
}

int opusgpu_packet_to_frames_mode(const uint8_t *packet, int32_t len, int32_t stream, int mode, opusgpu_frame_desc descs[48]) {
    if (!packet || !descs) return OPUSGPU_BAD_ARG;
    if (len <= 0) return len == 0 ? OPUSGPU_INVALID_PACKET : OPUSGPU_BAD_ARG;
    return ogh::packet_to_frames_mode(packet, len, stream, mode, descs);
}

int opusgpu_empty_packet_to_frames(int32_t stream, int32_t last_flags, int decoder_channels, int frame_size, opusgpu_frame_desc descs[48]) {
    if (!descs || frame_size <= 0 || frame_size % 120 || (decoder_channels != 1 && decoder_channels != 2)) return OPUSGPU_BAD_ARG;
    const int count = (frame_size + OPUSGPU_FRAME_SAMPLES - 1) / OPUSGPU_FRAME_SAMPLES;
    if (count > 48) return OPUSGPU_BAD_ARG;
    const int32_t flags = ogh::empty_flags(last_flags, decoder_channels);
    for (int i = 0; i < count; i++) descs[i] = opusgpu_frame_desc{stream, 0, 0, flags};
    return count;
}

static int grow(opusgpu_ctx *ctx, void **p, size_t *cap, size_t need) {
    if (*cap >= need) return OPUSGPU_OK;
    if (*p) HIPCHK(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
    size_t want = need + need / 2 + 256;
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) return fail(ctx, OPUSGPU_ALLOC_FAIL, "hipMalloc(staging)", e);
    *cap = want;
    return OPUSGPU_OK;
}

} // extern "C"

// the host-buffer path (opusgpu_decode_packets, opusgpu_decode_packets_fec): queues the steps above
#include "og_host_path.hpp"

// multistream decoding (include/opusgpu.h, MULTISTREAM): drives the contexts above
#include "og_ms.hpp"
#include "og_files_run.hpp"
#include "og_tracks.hpp"
#include "og_tracks_tail.hpp"
#include "og_tracks_loudness.hpp"
#include "og_tracks_resample.hpp"
#include "og_tracks_resample_ratio.hpp"
#include "og_feat.hpp"
#include "og_tracks_mel.hpp"
#include "og_tracks_stft.hpp"    // includes og_tracks_fft.hpp
#include "og_tracks_melspec.hpp" // includes og_tracks_melfft.hpp
#include "og_tracks_fbank.hpp"
#include "og_feat_batch.hpp"
#include "og_wave_batch.hpp"
#include "og_wave_trim.hpp"
#include "og_stft_batch.hpp"
#include "og_ms_tracks.hpp"
