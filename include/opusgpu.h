/*
 * opusgpu.h -- C ABI of the MI355X batched Opus decoder (libopusgpu.so).
 *
 * This is the drop-in boundary for the reference's decode hot path
 *   opus_multistream_decode -> opus_decode_native -> opus_decode_frame -> {ec_*, silk_Decode, celt_decode_with_ec}
 *   (reference: src/opus_decoder.cpp:931, :280, :154; src/silk.cpp:1481; src/celt.cpp:2162).
 * The reference decodes ONE stream per process with its codec state in file-scope globals; this
 * library keeps one state record per stream in HBM and decodes one 20 ms frame of every submitted
 * stream per step, one frame per wavefront.  PCM is bit-exact to the reference's fixed-point decoder.
 *
 * Plain C: opaque handle, plain pointers and sizes, negative OPUS_* error codes (reference values,
 * src/opus_decoder.h:70-77).  No exceptions cross this boundary.  One host thread per context.
 * The reference-compatible C++ entry points (opus_multistream_decode, op_read_stereo, ...) declared in
 * include/opus_decoder.h and include/opusfile.h are implemented on top of this ABI.
 */
#ifndef OPUSGPU_H
#define OPUSGPU_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPUSGPU_OK 0
#define OPUSGPU_BAD_ARG (-1)          /* OPUS_BAD_ARG */
#define OPUSGPU_BUFFER_TOO_SMALL (-2) /* OPUS_BUFFER_TOO_SMALL */
#define OPUSGPU_INTERNAL_ERROR (-3)   /* OPUS_INTERNAL_ERROR */
#define OPUSGPU_INVALID_PACKET (-4)   /* OPUS_INVALID_PACKET */
#define OPUSGPU_UNIMPLEMENTED (-5)    /* OPUS_UNIMPLEMENTED */
#define OPUSGPU_ALLOC_FAIL (-7)       /* OPUS_ALLOC_FAIL */
#define OPUSGPU_CELT_BAD_ARG (-18)    /* ERR_OPUS_CELT_BAD_ARG: a CELT-only / hybrid frame of <= 1 byte (src/celt.cpp:2225) */
#define OPUSGPU_ERR_NO_DEVICE (-100)  /* no usable HIP device / kernel image: there is NO CPU fallback */
#define OPUSGPU_ERR_HIP (-101)        /* a HIP runtime call failed; see opusgpu_last_error() */

#define OPUSGPU_FRAME_SAMPLES 960     /* the reference decodes 20 ms at 48 kHz only (src/opus_decoder.cpp:161) */
#define OPUSGPU_MAX_FRAME_BYTES 1275

typedef struct opusgpu_ctx opusgpu_ctx;

/* One frame of work for one stream in one decode step (16 bytes, device layout).
 * flags: bits 0-1 mode (0 SILK-only, 1 hybrid, 2 CELT-only); bits 2-4 bandwidth (0 NB .. 4 FB); bit 5 stereo;
 * bits 6-10: frame duration, the RFC bit and the FEC bit, zero in reference mode (see OPUSGPU_MODE_RFC);
 * bit 11 OPUSGPU_DESC_NO_MODE: see EMPTY PACKETS below.
 * These are the TOC fields opus_decode_native derives (src/opus_decoder.cpp:312-315).
 *
 * EMPTY PACKETS in reference mode (data == NULL or len == 0; src/opus_decoder.cpp:290-308).  The reference conceals nothing, but
 * its branch for them is live: it calls opus_decode_frame(st, NULL, 0, ...) -- a frame of NO bytes in the decoder's LAST mode,
 * bandwidth and channel count (what the last accepted packet's TOC set, :327-331), always 960 samples (:161) -- again and again
 * until `frame_size` samples exist, and stops at the first pass that fails.  What a pass does follows from opus_decode_frame:
 *   last packet SILK-only  -> the SILK decoder runs off a coder that reads zeros: 960 samples of PCM, the state moves on;
 *   last packet hybrid     -> the SILK half runs (and its state moves on), then celt_decode_with_ec refuses the empty frame:
 *                             ERR_OPUS_CELT_BAD_ARG = -18 (src/celt.cpp:2225); prev_mode is updated all the same (:276);
 *   last packet CELT-only  -> -18, nothing but prev_mode touched;
 *   no packet since the stream was created or reset -> st->mode is 0, which :175 / :249 run like hybrid (SILK at 16 kHz on the
 *                             decoder's channel count, then -18), and prev_mode stays 0.
 * Here: opusgpu_decode_packets takes packets[i] == NULL or lens[i] == 0 as such a packet with frame_size = frame_capacity x 960
 * and returns in result[i] the samples produced or the failing pass's code (the library remembers every stream's last accepted
 * TOC).  On the device path the caller passes, per pass, a descriptor with len 0 and the flags of the stream's last accepted
 * packet -- or, before the stream's first packet, opusgpu_empty_packet_to_frames' flags (hybrid, the decoder's channel count,
 * OPUSGPU_DESC_NO_MODE).  opusgpu_empty_packet_to_frames builds the descriptors either way.  (The library's memory of a stream's
 * last accepted TOC is kept by opusgpu_decode_packets and cleared by opusgpu_streams_alloc / _reset: a caller that decodes a
 * stream through the device path keeps that stream's last flags itself, and should not mix the two paths on one stream around an
 * empty packet.) */
#define OPUSGPU_DESC_NO_MODE (1 << 11)
typedef struct opusgpu_frame_desc {
    int32_t stream;  /* stream index in the context */
    int32_t offset;  /* byte offset of the frame payload inside the packet arena */
    int32_t len;     /* payload bytes, 0..1275 */
    int32_t flags;
} opusgpu_frame_desc;

/* ---- context -------------------------------------------------------------------------------- */
int opusgpu_version(void);
/* Binds to HIP device `device` (>=0).  Fails with OPUSGPU_ERR_NO_DEVICE when no GPU is usable. */
int opusgpu_ctx_create(int device, opusgpu_ctx **out);
void opusgpu_ctx_destroy(opusgpu_ctx *ctx);
const char *opusgpu_last_error(const opusgpu_ctx *ctx);

/* ---- RFC mode (opt-in, off by default) ---------------------------------------------------------
 * The reference decodes every frame as 20 ms whatever its TOC says (src/opus_decoder.cpp:161, :186, :341; Q6).  With
 * OPUSGPU_MODE_RFC set, frames decode at the duration the TOC names -- CELT 2.5 / 5 / 10 / 20 ms, SILK 10 / 20 / 40 / 60 ms
 * (src/silk.cpp:1522-1540 with the real payload duration), hybrid 10 / 20 ms -- multi-frame packets (codes 1 - 3) accordingly;
 * CELT's last band follows the bandwidth (Q1 fixed) and a SILK-only frame after a hybrid one fades the CELT layer out with the
 * two-byte silence frame of RFC 6716 section 4.5.2 instead of Q4's frame off the stale coder; the redundant 5 ms CELT frames of
 * mode transitions (section 4.5.1) are decoded and cross-faded in (Q2 fixed), and a switch between CELT-only and the SILK modes
 * that no redundant frame covers starts with 5 ms of the old mode's concealment, cross-faded into the new frame (section 4.5).
 * Everything else stays as the reference has it (Q3 mixing, Q5 partial reset).  The reference cannot produce these outputs and
 * no libopus exists:
 * this mode is bit-exact to oracle/'s RFC mode (oc_decoder_set_rfc), which is PARITY-UNPINNED.
 * RFC-mode frames run on a kernel of their own (wave-uniform entropy decoding): the mode is for completeness, not speed.
 * LOSS PATH (the reference has none, Q8 -- in reference mode an empty packet does what the reference's
 * empty-packet branch does, see EMPTY PACKETS above: no concealment):
 *   - opusgpu_decode_packets: packets[i] == NULL or lens[i] == 0 is a LOST packet: it is concealed for as long as the stream's
 *     last packet was (frame count x frame duration; 20 ms of zeros before the stream's first packet or after a reset), what
 *     opus_decode(data = NULL, frame_size = last duration) gives; result[i] = the samples concealed;
 *   - a frame of at most one payload byte (DTX) is concealed for its TOC's duration;
 *   - opusgpu_decode_step_device: a descriptor with len <= 1 conceals the duration in its flags; mode and bandwidth come from
 *     the stream's state, the stereo bit should be that of the stream's last packet.
 *   SILK conceals with the reference's own (unreachable) silk_PLC / silk_CNG code restated (src/silk.cpp:2862-3185, :1305-1432),
 *   CELT like RFC 6716's decoder (celt_decode_lost): the first five lost frames of a CELT-only stream are extrapolated from the
 *   pitch period of the last output (pitch search, order-24 LPC, the residual of the last two periods repeated through the
 *   synthesis filter with a decay, an overlap tail for the next frame's transform), later ones and hybrid's CELT layer are
 *   noise at the decaying band energies; hybrid conceals with both coders.
 *   Two things to know (a decoder's concealment is not normative, and the oracle's RFC mode makes the same choices, so GPU and
 *   oracle agree with each other, not sample by sample with libopus): (1) the pitch-based branch follows that decoder's
 *   STRUCTURE with fixed-point detail of this repository's own (64-bit accumulators, the 1,024 samples of history the decoder
 *   keeps, csrc/og_plc.hpp); (2) a concealment is cut into pieces of the stream's LAST frame duration (what opus_decode(NULL)
 *   is asked for), with a remainder of 30 / 50 ms as 20 / 40 + 10 ms.  Use one mode per stream from its (re)set on:
 *   the state the concealment needs is only kept by RFC-mode frames.
 * Applies to opusgpu_packet_to_frames_mode / opusgpu_decode_packets / opusgpu_decode_step_device calls made after it is set:
 *   - descriptors carry the duration and the mode bit (frame_desc.flags bits 6 - 9); one without the bit is OPUSGPU_BAD_ARG;
 *   - opusgpu_decode_packets: result[i] and the PCM block of packet i hold the packet's true sample count (<= 5760);
 *   - opusgpu_decode_step_device: d_pcm is [n][OPUSGPU_RFC_FRAME_SAMPLES * channels] (room for a 60 ms frame), d_result[f]
 *     the frame's sample count. */
#define OPUSGPU_MODE_REFERENCE 0
#define OPUSGPU_MODE_RFC 1
#define OPUSGPU_RFC_FRAME_SAMPLES 2880
int opusgpu_set_mode(opusgpu_ctx *ctx, int mode);
int opusgpu_get_mode(const opusgpu_ctx *ctx);

/* Pipelined decode steps (off by default).  A stream's frames are sequential, but only two things tie step k+1 to step k
 * before its reconstruction: the range decoder of a CELT frame predicts the band energies from the previous frame's, and
 * the SILK half reads the SILK state.  With pipelining on, the library carries the band energies in the parse kernel
 * (k_celt_parse) and runs that kernel for step k+1's CELT-only frames on a stream of its own, NEXT TO step k's
 * reconstruction (k_celt_recon_fb / k_celt_post), into one of three rotating sets of parse records; the reconstruction runs on another
 * stream of the library's own and never touches the caller's buffers, the step's own stream waits for it before the
 * de-emphasis (k_celt_post) writes PCM and result codes.  Results are bit-identical to the in-order flow (tests/test_gpu_pipeline.py); the step's stream
 * still completes everything the step launched, so the caller synchronises exactly as before.
 * What the caller additionally guarantees while it is on, for opusgpu_decode_step_device:
 *   - d_descs and d_arena of a call are COMPLETE in device memory when the call is made (uploaded and synchronised, or
 *     produced by work that has finished) -- not merely queued on `hip_stream` ahead of the call;
 *   - consecutive steps use the same stream (a change of stream is honoured by draining both, i.e. no overlap).
 * Which steps run ahead: a step the caller declares CELT-only (opusgpu_decode_step_device_modes, OPUSGPU_HAS_CELT alone) as
 * described; a step declared free of CELT-only frames (OPUSGPU_HAS_SILK, OPUSGPU_HAS_HYBRID or both) runs its SILK parse -- and a
 * hybrid frame's CELT parse behind it -- for step k+1 next to step k's SILK synthesis: the SILK parse keeps a copy of its own of
 * what the entropy half needs of the frames before (indices' history, gain index, NLSFs, rate, channel count, prev_mode), which is
 * exactly what it can compute itself (tests/test_emul_vs_oracle.py checks the copy against the state frame by frame); only a
 * step that may hold hybrid frames waits for a step that may have held SILK-only ones (the hybrid -> SILK-only transition frame
 * decodes a CELT frame in the step's last kernel).  A step that is undeclared or mixes CELT-only frames with the others runs in
 * order (cut into two halves on two streams when it has SILK frames).  Going from one kind of step to another drains the device.
 * opusgpu_decode_packets (whose uploads are queued by the call itself) runs in order regardless.  Switching synchronises
 * the device.  Reference: the per-packet call sequence this replaces is src/opus_decoder.cpp:931 -> :280 -> :154 ->
 * src/celt.cpp:2162, one packet at a time; there is nothing to pipeline there. */
int opusgpu_set_pipeline(opusgpu_ctx *ctx, int on);
int opusgpu_get_pipeline(const opusgpu_ctx *ctx);

/* ---- streams -------------------------------------------------------------------------------- */
/* Allocates `n_streams` per-stream state records in HBM (replacing any previous set) and gives each
 * the fresh state of opus_multistream_decoder_init(48000, channels, 1, channels-1, {0,1})
 * (src/opus_decoder.cpp:742).  channels is 1 or 2. */
int opusgpu_streams_alloc(opusgpu_ctx *ctx, int n_streams, int channels);
/* full != 0: fresh state again (decoder_init).  full == 0: OPUS_RESET_STATE semantics of
 * opus_multistream_decoder_ctl (src/opus_decoder.cpp:976 -> :382), which is NOT a full reset (CELT keeps
 * its synthesis history, band energies and de-emphasis memory: src/celt.cpp:2479-2498). */
int opusgpu_streams_reset(opusgpu_ctx *ctx, int first, int count, int full);
int opusgpu_stream_count(const opusgpu_ctx *ctx);
int opusgpu_stream_channels(const opusgpu_ctx *ctx);
size_t opusgpu_stream_state_bytes(void);

/* ---- host-buffer path: the batched equivalent of opus_multistream_decode (src/opus_decoder.cpp:931) --- */
/* Decodes packets[i] (lens[i] bytes, TOC first) for stream stream_ids[i], i < n; a stream may appear
 * at most once per call.  pcm receives n blocks of `frame_capacity` * 960 * channels interleaved int16;
 * result[i] = samples per channel decoded for packet i (frames * 960) or a negative OPUS_* code.
 * Packets with several frames (codes 1-3) are decoded frame after frame like opus_decode_native.
 * One deliberate difference from the reference: it checks the room as frames * (frame duration from the TOC) but
 * decodes every frame as 960 samples (src/opus_decoder.cpp:161, :323), so a packet of more short frames than
 * `frame_capacity` passes its check and overruns the caller's buffer.  Here such a packet gets
 * OPUSGPU_BUFFER_TOO_SMALL and nothing is written.
 * Returns OPUSGPU_OK or a context-level error. */
int opusgpu_decode_packets(opusgpu_ctx *ctx, int n, const int32_t *stream_ids, const uint8_t *const *packets,
                           const int32_t *lens, int16_t *pcm, int frame_capacity, int32_t *result);

/* RFC mode only (OPUSGPU_BAD_ARG otherwise): forward error correction, opus_decode(decode_fec = 1) of RFC 6716's decoder -- the
 * reference has neither the flag nor the path.  packets[i] is the packet that FOLLOWS a lost packet of stream stream_ids[i]: the
 * lost packet's duration (that of the stream's last packet) is produced -- the last frame's worth of it from the LBRR frames in
 * packets[i]'s first frame where it is a SILK-only or hybrid packet (SILK conceals the channels / internal frames without an LBRR
 * copy, hybrid's CELT layer conceals), everything before that by concealment; a CELT-only packet or predecessor carries no such
 * data: plain concealment.  result[i] = samples produced.  Call opusgpu_decode_packets with the same packets afterwards: the
 * packet itself is not decoded here.  On the device path: descriptor flags bit 10 on the packet's first frame. */
int opusgpu_decode_packets_fec(opusgpu_ctx *ctx, int n, const int32_t *stream_ids, const uint8_t *const *packets,
                               const int32_t *lens, int16_t *pcm, int frame_capacity, int32_t *result);

/* Splits one packet into frame descriptors exactly as opus_packet_parse_impl + the TOC helpers do
 * (src/opus_decoder.cpp:559, :135, :460, :474).  descs[k].offset is relative to the packet start.
 * Returns the frame count (1..48) or a negative OPUS_* code.  Pure host code. */
int opusgpu_packet_to_frames(const uint8_t *packet, int32_t len, int32_t stream, opusgpu_frame_desc descs[48]);
/* The same for a given mode (OPUSGPU_MODE_*): in RFC mode the descriptors carry the frames' duration (flags bits 6 - 8: 0 20 ms,
 * 1 2.5, 2 5, 3 10, 4 40, 5 60) and the RFC bit (bit 9). */
int opusgpu_packet_to_frames_mode(const uint8_t *packet, int32_t len, int32_t stream, int mode, opusgpu_frame_desc descs[48]);
/* (Both mirror opus_packet_parse_impl, whose answer to len == 0 is OPUS_INVALID_PACKET, src/opus_decoder.cpp:567: an empty
 * packet has no TOC to take descriptors from.)  Reference mode, the frames of an EMPTY packet for the device path (EMPTY
 * PACKETS above): `last_flags` = the flags of the stream's last accepted packet (descs[0].flags of opusgpu_packet_to_frames),
 * or a negative value when the stream has had none since it was created / reset (`decoder_channels` then names the stream's
 * channel count); `frame_size` as opus_decode's.  Writes ceil(frame_size / 960) descriptors of len 0 -- one per pass of the
 * reference's loop, to be run one step each until a pass returns a negative code -- and returns their count; OPUSGPU_BAD_ARG
 * when frame_size <= 0 or no multiple of 120 (:290, :351) or more than 48 passes. */
int opusgpu_empty_packet_to_frames(int32_t stream, int32_t last_flags, int decoder_channels, int frame_size, opusgpu_frame_desc descs[48]);

/* ---- device-resident path (inputs and outputs stay in HBM; used by bench.py and on-device consumers) -- */
int opusgpu_dev_alloc(opusgpu_ctx *ctx, size_t bytes, void **dptr); /* hipMalloc of bytes + 16: aligned and tailed as a packet arena must be */
int opusgpu_dev_free(opusgpu_ctx *ctx, void *dptr);
int opusgpu_memcpy_h2d(opusgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
int opusgpu_memcpy_d2h(opusgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
/* One decode step: n frames described by d_descs (device array of opusgpu_frame_desc), payload bytes in
 * d_arena, PCM to d_pcm[n][960*channels] int16, per-frame result to d_result[n] int32.  Asynchronous on the
 * context's stream (or on `hip_stream` if not NULL: a hipStream_t).
 * The tables are in device memory and are NOT validated beyond what a frame's own kernel can see.  The caller guarantees:
 *   - a stream appears at most once in a step (frames of one stream are sequential: one step each);
 *   - 0 <= offset and offset + len lies inside the arena; d_arena is 16-byte aligned (checked: OPUSGPU_BAD_ARG) and the
 *     ALLOCATION extends at least to the next multiple of 16 past the last frame's end (the kernels fetch packets as aligned
 *     16-byte pieces; allocating 16 bytes more than the packed bytes, as every producer in this repository does, is enough);
 *   - d_descs, d_arena, d_pcm and d_result stay valid and unmodified until the step has completed on its stream.
 * Checked on the device, per frame, and reported in d_result: stream index out of range -> OPUSGPU_BAD_ARG; len outside
 * 0..1275 -> OPUSGPU_BAD_ARG; every decode error the reference would return for the frame.
 * opusgpu_packet_to_frames, opusgpu_decode_packets and opusgpu_pages_demux produce tables that satisfy all of this. */
int opusgpu_decode_step_device(opusgpu_ctx *ctx, int n, const void *d_descs, const void *d_arena, void *d_pcm,
                               void *d_result, void *hip_stream);
/* The same, for a caller that knows which kinds of frame the step contains (whoever framed the packets does: the TOC byte).
 * `modes`: bit 0 SILK-only, bit 1 hybrid, bit 2 CELT-only frames MAY be present (1 .. 7; plus OPUSGPU_STEP_KEEPS_MODE).  The kernels of modes ruled out are
 * not launched -- on a step of 65,536 frames the launches that find nothing to do cost 1 - 2 % -- and a pipelined step
 * (opusgpu_set_pipeline) without SILK-only and hybrid frames also starts its reconstruction while the previous step's
 * de-emphasis still runs.  A frame of a mode that was ruled out is reported as OPUSGPU_BAD_ARG in d_result and not decoded. */
#define OPUSGPU_HAS_SILK 1
#define OPUSGPU_HAS_HYBRID 2
#define OPUSGPU_HAS_CELT 4
/* May be OR-ed into `modes` of a pipelined step (opusgpu_set_pipeline): the caller's word that NO STREAM OF THIS STEP HAS DECODED A
 * FRAME OF ANOTHER MODE (SILK-only, hybrid, CELT-only) SINCE ITS LAST RESET -- SURVEY 8d config 5: a stream's mode is fixed.  What it
 * buys: (1) a step with frames of every mode (modes 7) runs ahead like a declared one -- its entropy kernels next to the arithmetic
 * kernels of the step before -- where without the flag it runs in order: a CELT-only frame changes what the SILK half of the SAME
 * stream's next frame must see, which the library cannot rule out by itself; (2) declared steps of the two pipelined kinds
 * (CELT-only; SILK-only / hybrid) follow each other without the drain that a stream crossing from one to the other would need.
 * Results with a true promise are bit-identical to the in-order flow; with a false one they are undefined for the streams that
 * broke it (never for others). */
#define OPUSGPU_STEP_KEEPS_MODE 8
int opusgpu_decode_step_device_modes(opusgpu_ctx *ctx, int n, const void *d_descs, const void *d_arena, void *d_pcm,
                                     void *d_result, void *hip_stream, int modes);
/* A WINDOW of consecutive decode steps in one call: step j has n[j] frames and the tables d_descs[j] / d_arena[j], and writes
 * d_pcm[j] / d_result[j]; everything opusgpu_decode_step_device_modes says holds per step (`modes`: 0 = not known), the tables of
 * every step are complete in device memory at the call.  Same results as n_steps single calls.  The point is pipelined steps
 * (opusgpu_set_pipeline) of CELT-only frames (SILK-only and hybrid steps pipeline the same way with either entry): knowing the step that follows, the library orders the kernels of neighbouring
 * steps by real dependencies -- the next step's parse is placed before this step's reconstruction, that before the previous
 * step's de-emphasis, each held by a stream memory wait on a count of started workgroups -- where a single call has to leave
 * the order to the hardware queues (round 2 used a spin-wait kernel and an unused LDS request for it; both are gone). */
int opusgpu_decode_steps_device(opusgpu_ctx *ctx, int n_steps, const int32_t *n, const void *const *d_descs, const void *const *d_arena,
                                void *const *d_pcm, void *const *d_result, void *hip_stream, int modes);
int opusgpu_synchronize(opusgpu_ctx *ctx);
/* HIP events on the context's stream, for timing from hosts without HIP headers. */
int opusgpu_event_create(opusgpu_ctx *ctx, void **event);
int opusgpu_event_record(opusgpu_ctx *ctx, void *event);
int opusgpu_event_elapsed_ms(opusgpu_ctx *ctx, void *start, void *stop, float *ms); /* synchronises on stop */
int opusgpu_event_destroy(opusgpu_ctx *ctx, void *event);
int opusgpu_event_synchronize(opusgpu_ctx *ctx, void *event); /* the host waits for it */
/* Uploads NEXT TO the decode (config 5: the ingest of the next batch of Ogg pages under the decode of this one).  The copy runs on
 * a stream of the context's own, not on the decode stream: one host thread demuxes batch b + 1 (opusgpu_pages_demux) and queues
 * its step tables and packet bytes with opusgpu_upload_async, then records a fence; the thread that decodes lets its stream wait
 * for that fence (opusgpu_stream_wait_event; hip_stream NULL = the context's stream -- and with it the streams pipelined steps run
 * ahead on, so that tables behind the fence count as complete in device memory for opusgpu_set_pipeline) before batch b + 1's first step.  `src` must
 * stay valid until the fence has passed (opusgpu_event_synchronize).  These four calls may come from a second host thread. */
int opusgpu_upload_async(opusgpu_ctx *ctx, void *dst, const void *src, size_t bytes);
int opusgpu_upload_fence(opusgpu_ctx *ctx, void *event);
int opusgpu_stream_wait_event(opusgpu_ctx *ctx, void *event, void *hip_stream);
/* Page-lock a caller-owned host buffer in place (and undo it): transfers from / into it need no staging copy. */
int opusgpu_host_register(opusgpu_ctx *ctx, void *ptr, size_t bytes);
int opusgpu_host_unregister(opusgpu_ctx *ctx, void *ptr);
/* Copies stream `index`'s raw state record to the host (tests / checkpointing). */
int opusgpu_stream_state_get(opusgpu_ctx *ctx, int index, void *dst, size_t bytes);
/* What the reference's OPUS_GET_PITCH ctl looks at (src/opus_decoder.cpp:399-407, src/silk.cpp:1764-1769), for stream `index`:
 * out[0] = prev_mode (0 before the first frame, else 1000 / 1001 / 1002), out[1] = the first SILK channel's prevSignalType
 * (2 = voiced), out[2] = its lagPrev, out[3] = its internal rate in kHz (0 before the first SILK frame).  include/opus_decoder.h's
 * ctl is built on it (csrc/og_compat.cpp).  Synchronises the context's stream. */
int opusgpu_stream_pitch_get(opusgpu_ctx *ctx, int index, int32_t out[4]);

/* TEST / DEBUG ENTRY: what the kernels of the last opusgpu_decode_step_device call (reference mode, split path) left BETWEEN
 * the stages, for slot `slot` of that step and the stream it belongs to -- so that a parity test can tell which kernel a
 * difference comes from instead of seeing it only in the PCM (tests/test_gpu_stage_taps.py compares every field with the
 * oracle's taps).  Synchronises the context's stream. */
typedef struct opusgpu_stage_taps {
    /* k_celt_parse's record (CELT-only and hybrid frames; celt_valid = 0 otherwise): the frame's header as parsed */
    int32_t celt_valid, celt_ret, silence, transient, lm, spread, dual_stereo, anti_collapse_on, intensity, pf_pitch, pf_gain,
        pf_tapset, n_leaves;
    uint32_t celt_rng_final;
    int16_t bandE[42];   /* final band energies (coarse + fine + finalise), both channels */
    int16_t pulses[21];
    int8_t tf_res[21];
    int8_t pad0[3];
    /* k_celt_recon / k_celt_recon_fb: the stream's state after the step -- the frame's synthesis output after the comb filter
     * (the newest 960 samples of the history ring), the IMDCT overlap tail carried to the next frame, energies, rng */
    int32_t syn_post[2][960];
    int32_t overlap_tail[2][60];
    int16_t state_bandE[42], state_logE1[42], state_logE2[42], pad1;
    uint32_t state_rng;
    int32_t pf_period, pf_gain_state, pf_tapset_state;
    /* k_silk_parse's record (SILK-only and hybrid frames; silk_valid = 0 otherwise): dequantised parameters per coded channel */
    int32_t silk_valid, silk_ret, decode_only_middle, ms_pred_q13[2];
    struct {
        int32_t pitchL[4], Gains_Q16[4];
        int16_t PredCoef_Q12[2][16];
        int16_t LTPCoef_Q14[20];
        int32_t LTP_scale_Q14, signalType, quantOffsetType;
    } silk_ch[2];
    /* k_silk_synth: the channels' state after the step -- the synthesis core's output at the internal rate (for 20 ms frames
     * the output history IS the frame), the LPC state */
    int16_t silk_out[2][320];
    int32_t silk_sLPC_Q14[2][16];
    int32_t silk_fs_kHz[2];
} opusgpu_stage_taps;
int opusgpu_debug_stage_taps(opusgpu_ctx *ctx, int slot, opusgpu_stage_taps *out);

/* ---- Ogg page ingest at scale (host only, no GPU involved) --------------------------------------
 * The batched equivalent of what the reference does one page at a time: page sync + header checks
 * (ogg_sync_pageseek src/ogg.cpp:839-923), the page CRC (ogg_page_checksum_set :439-480), lacing values -> packets
 * (ogg_stream_pagein / ogg_stream_packetout :969-1097, :1192; op_collect_audio_packets src/opusfile.cpp:424-466) and
 * the TOC split of every packet (opusgpu_packet_to_frames above).  Input: n complete Ogg pages, each tagged by the
 * caller with the decoder stream it belongs to (the caller owns the serial-number -> stream mapping).  Output: decode
 * steps.  Step k holds one descriptor per page that has a k-th 20 ms frame, ready for opusgpu_decode_step_device after
 * the arena and the step's table are copied to the device; frames of one page land in consecutive steps, and a second
 * page of the same stream in the same call starts where the first one ends, so a stream never appears twice in a step.
 * A page must carry whole packets: one that starts with the tail or ends with the head of a spanning packet is
 * reported (OPUSGPU_PAGE_SPANS) and contributes nothing; the file surface (opusfile.h) handles such streams.
 * Every frame becomes its own step entry: if a frame of a multi-frame packet fails on the device (in practice a CELT or
 * hybrid frame of at most one byte, which the reference's CELT decoder rejects), the later frames of that packet are
 * still decoded.  opus_decode_native -- and opusgpu_decode_packets -- stop at a packet's first failing frame. */
#define OPUSGPU_PAGE_BAD_CAPTURE (-200) /* no "OggS", stream structure version != 0, or shorter than its header says */
#define OPUSGPU_PAGE_BAD_CRC (-201)     /* only with OPUSGPU_PAGES_VERIFY_CRC */
#define OPUSGPU_PAGE_SPANS (-202)
#define OPUSGPU_PAGE_BAD_PACKET (-203)  /* a packet with a valid duration fails the frame split (opus_packet_parse_impl): the
                                           reference decodes the page's earlier packets and then reports the error; here
                                           the whole page is dropped.  Packets whose TOC sequence has no valid duration
                                           are skipped like the reference does (src/opusfile.cpp:453-459). */
#define OPUSGPU_PAGE_BAD_STREAM (-204)  /* negative stream id */

#define OPUSGPU_PAGES_VERIFY_CRC 1
#define OPUSGPU_PAGES_GROUP_BY_MODE 2 /* order each step's table SILK-only, hybrid, CELT-only (stable): uniform waves */
#define OPUSGPU_PAGES_ORDER_BY_HEADER 4 /* (implies the grouping) within the SILK-only and the hybrid group: by the frames' LBRR flags -- bits 6 and
                                          4 of a frame's first byte (src/silk.cpp:1568-1573) -- stable otherwise: the 32 frames of a parse wave
                                          then agree on how many frames of forward-error-correction data they read past (:1590-1616) */

typedef struct opusgpu_page_info { /* 32 bytes */
    int32_t status;      /* >= 0: 20 ms frames the page contributes; < 0: OPUSGPU_PAGE_* */
    int32_t packets;     /* packets on the page */
    int32_t first_step;  /* step of the page's first frame */
    int32_t header_type; /* bit 0 continued, bit 1 first page of the stream, bit 2 last page */
    uint32_t serial, seqno;
    int64_t granulepos;
} opusgpu_page_info;

typedef struct opusgpu_page_batch opusgpu_page_batch; /* owns the step tables and the packet arena of one demux call */

/* threads <= 0: one.  info (n_pages entries) may be NULL.  Returns OPUSGPU_OK (bad pages are reported per page, not as
 * a failure of the call), OPUSGPU_BAD_ARG or OPUSGPU_ALLOC_FAIL. */
int opusgpu_pages_demux(int n_pages, const uint8_t *const *pages, const int32_t *page_lens, const int32_t *stream_ids,
                        int flags, int threads, opusgpu_page_info *info, opusgpu_page_batch **out);
/* The same demux with the step tables and the packet arena placed in the CALLER's memory (16-byte aligned; page-locked memory makes
 * the batch uploadable as it lies, in one copy): out_mem = [descriptors of all steps, step after step | padding to a multiple of 256
 * | arena + 16 bytes].  *out_need (may be NULL) receives the bytes needed; OPUSGPU_BUFFER_TOO_SMALL when out_cap is less (nothing is
 * written then; n_pages * 16 * 255 + the pages' bytes + 512 always suffices).  The batch object still owns the per-slot page
 * indices; opusgpu_page_batch_step / _arena point into out_mem, which must outlive the batch.  Descriptor offsets index the arena,
 * which begins opusgpu_page_batch_arena_offset(batch) bytes into out_mem. */
int opusgpu_pages_demux_into(int n_pages, const uint8_t *const *pages, const int32_t *page_lens, const int32_t *stream_ids,
                             int flags, int threads, opusgpu_page_info *info, void *out_mem, size_t out_cap, size_t *out_need,
                             opusgpu_page_batch **out);
size_t opusgpu_page_batch_arena_offset(const opusgpu_page_batch *b);
int opusgpu_page_batch_steps(const opusgpu_page_batch *b);
/* Step `step`: returns its descriptor count and points *descs at the table and *slot_pages (may be NULL) at the index
 * of the input page each descriptor came from (the PCM block of slot s belongs to page (*slot_pages)[s]). */
int opusgpu_page_batch_step(const opusgpu_page_batch *b, int step, const opusgpu_frame_desc **descs,
                            const int32_t **slot_pages);
const uint8_t *opusgpu_page_batch_arena(const opusgpu_page_batch *b, size_t *bytes); /* descriptor offsets index this */
void opusgpu_page_batch_free(opusgpu_page_batch *b);

/* Page checksums on the GPU ("optional GPU CRC"): for pages that are already in HBM -- e.g. raw pages
 * delivered by the work-queue scatter -- the page CRC of ogg_page_checksum_set (src/ogg.cpp:439-480) is recomputed by a
 * kernel, one page per lane, and compared with the stored one.  d_blob: the pages' bytes; d_offsets (int64[n_pages]) and
 * d_lens (int32[n_pages]): where page i lies in d_blob; d_status (int32[n_pages]) receives 1 = checksum matches,
 * 0 = mismatch, OPUSGPU_PAGE_BAD_CAPTURE = not a complete Ogg page (capture pattern, version, lengths: the checks of
 * opusgpu_pages_demux).  The caller guarantees that every [offset, offset + len) lies inside d_blob.  A host demux of
 * pages verified this way can drop OPUSGPU_PAGES_VERIFY_CRC.  Asynchronous on the context's stream (or `hip_stream`). */
int opusgpu_pages_crc_device(opusgpu_ctx *ctx, int n_pages, const void *d_blob, const void *d_offsets, const void *d_lens,
                             void *d_status, void *hip_stream);

/* Output stage of the player: decoded PCM -> the 32-bit words src/main.cpp hands to the I2S peripheral.
 * Replaces playChunk (src/main.cpp:148-224), playSample (:226-256) and Gain (:137-146) for a whole step at once: every
 * block of d_pcm is one m_outBuff.  Per output frame: the two samples are picked by bit depth / channel count /
 * force-mono, 8-bit samples are expanded ((x - 128) << 8), both are halved for headroom (>> 1), scaled
 * ((s * volume) >> 6) and packed as (right << 16) | (left & 0xffff).  The OpusHead output gain is NOT applied -- the
 * reference does not apply it either (op_update_gain is commented out, src/opusfile.cpp:704). */
typedef struct opusgpu_output_cfg {
    uint8_t volume;     /* m_vol (src/main.cpp:39): 64 = unity; above 127 the 16-bit halves wrap as they do there */
    uint8_t force_mono; /* m_f_forceMono: both channels play (left + right) / 2 */
    uint8_t bits;       /* setBitsPerSample: 16, or 8 (every int16 of the block holds two unsigned 8-bit samples) */
    uint8_t channels;   /* setChannels: 2 (interleaved), or 1 */
} opusgpu_output_cfg;

/* Block b: int16 samples at d_pcm + b * pcm_stride (stride in int16 units; a decode step's PCM has stride
 * 2 * 960 * frame_capacity), m_validSamples = d_valid[b] (int32; e.g. the step's result array: a negative entry plays
 * nothing) or valid_all when d_valid is NULL, at most block_samples.  Settings: d_cfgs[b] (device array) or `cfg` when
 * d_cfgs is NULL; `cfg` with other bits / channels than the setters accept is OPUSGPU_BAD_ARG, such a d_cfgs entry makes
 * its block play nothing (as playChunk does).  Output: uint32 words at d_i2s + b * i2s_stride, `valid` of them -- 2 * valid
 * for 8-bit mono, so i2s_stride must hold 2 * block_samples there; words past a block's count are left untouched.
 * 16-byte aligned bases with pcm_stride % 8 == 0 and i2s_stride % 4 == 0 take the fast path; anything else works too.
 * Asynchronous on the context's stream (or `hip_stream`). */
int opusgpu_output_stage_device(opusgpu_ctx *ctx, int n_blocks, int block_samples, const void *d_pcm, long long pcm_stride,
                                const void *d_valid, int valid_all, const void *d_cfgs, opusgpu_output_cfg cfg, void *d_i2s,
                                long long i2s_stride, void *hip_stream);

/* ---- MULTISTREAM: surround, family-255 and other multi-stream Opus ----------------------------------------
 * A multistream packet carries `streams` elementary Opus packets, one per elementary stream, each in self-delimited framing
 * (RFC 6716 Appendix B) except the last one, which is in standard framing (opus_multistream_packet_validate,
 * src/opus_decoder.cpp:803-823).  The first `coupled` streams are stereo and are decoded by 2-channel decoders, the rest are mono
 * and are decoded by 1-channel decoders, with everything that implies: a mono decoder downmixes a stereo packet, a stereo decoder
 * duplicates a mono packet (Q3 mixing of mono SILK-only frames included).  Each elementary stream is exactly what a context of
 * that channel count would make of its packets.  The decoded channels -- 2s and 2s + 1 the left and right of coupled stream s,
 * coupled + s mono stream s (s >= coupled) -- go to output channel c from decoded channel mapping[c] (get_left_channel /
 * get_right_channel / get_mono_channel, :700-727); one decoded channel may feed several outputs, mapping[c] == 255 is silence.
 * The reference defines these semantics but cannot run them for more than one stream (its decoders share one codec state); here
 * every elementary stream has its own state record.
 * The opus_multistream_* entry points of include/opus_decoder.h keep answering OPUS_UNIMPLEMENTED for streams != 1, as the
 * reference build does; this section is the way to decode such streams.
 * An opusgpu_ms holds n_decoders multistream decoders of ONE layout (one object per layout) on two contexts of its own
 * (n_decoders * coupled stereo streams, n_decoders * (streams - coupled) mono streams).  Steps run in order (no pipelining).
 * Layout checks (opus_multistream_decoder_init :742-770 and validate_layout :688-697): 1 <= channels <= 255, streams >= 1,
 * 0 <= coupled <= streams, streams + coupled <= 255, every mapping[c] (c < channels) < streams + coupled or 255; otherwise
 * OPUSGPU_BAD_ARG. */
typedef struct opusgpu_ms_layout {
    int32_t channels;     /* 1..255 output channels */
    int32_t streams;      /* 1..255 elementary streams */
    int32_t coupled;      /* the first `coupled` streams are stereo, the rest mono */
    uint8_t mapping[256]; /* output channel c <- decoded channel mapping[c]; 255 = silent; entries >= channels are ignored */
} opusgpu_ms_layout;
typedef struct opusgpu_ms opusgpu_ms;

int opusgpu_ms_create(int device, const opusgpu_ms_layout *layout, int n_decoders, opusgpu_ms **out);
void opusgpu_ms_destroy(opusgpu_ms *ms);
const char *opusgpu_ms_last_error(const opusgpu_ms *ms);
/* OPUSGPU_MODE_REFERENCE / OPUSGPU_MODE_RFC for both contexts (RFC mode: see opusgpu_set_mode; forward error correction is not
 * offered here). */
int opusgpu_ms_set_mode(opusgpu_ms *ms, int mode);
/* Decoders [first, first + count): every elementary stream as opusgpu_streams_reset does it. */
int opusgpu_ms_reset(opusgpu_ms *ms, int first, int count, int full);
/* Host framing of one multistream packet: descs[s * 48 + k] = frame k of elementary stream s (stream field = `decoder`, offsets
 * relative to the packet start, flags as opusgpu_packet_to_frames_mode makes them for `mode`), counts[s] = its frame count.
 * Returns the packet's duration in samples at 48 kHz (every stream has it) or: OPUSGPU_INVALID_PACKET for len == 0 or
 * len < 2 * streams - 1 (:855), a missing stream, streams of different durations, a stream longer than 120 ms (:803-823); what
 * the frame split returns for a malformed stream; OPUSGPU_BAD_ARG for a bad layout or argument.  Reference mode only: streams
 * with equal durations but different frame counts are OPUSGPU_INVALID_PACKET -- the reference decodes every frame as 960
 * samples (Q6), so such streams would give different sample counts and its loop (:866-909) would overrun its buffer.  Refusing
 * the packet is a deliberate difference. */
int opusgpu_ms_packet_to_frames(const opusgpu_ms_layout *layout, const uint8_t *packet, int32_t len, int32_t decoder, int mode,
                                opusgpu_frame_desc *descs, int32_t *counts);
/* The batched opus_multistream_decode (src/opus_decoder.cpp:826-914): packets[i] (lens[i] bytes) for decoder decoder_ids[i],
 * i < n; a decoder may appear at most once per call.  pcm receives n blocks of frame_capacity * 960 * channels interleaved int16
 * (frame_capacity 1..48); result[i] = samples per channel (the common count of the elementary streams) or a negative code.
 * Checked on the host before anything is decoded: the framing above (OPUSGPU_INVALID_PACKET), the duration against frame_size =
 * min(frame_capacity * 960, 5760) (OPUSGPU_BUFFER_TOO_SMALL, :845-847), and in reference mode, like opusgpu_decode_packets, more
 * frames than frame_capacity (OPUSGPU_BUFFER_TOO_SMALL).  Also reference mode: with more than one stream, frames longer than 20 ms
 * are OPUSGPU_BUFFER_TOO_SMALL -- the reference checks every stream after the first against the first one's result (:880,
 * frame_size = ret), which counts 960 samples per frame, and fails the second stream after decoding the first; here nothing is
 * decoded.  Decode-time refusals (e.g. OPUSGPU_CELT_BAD_ARG for a CELT or hybrid frame of at most one byte) are reported as the
 * first negative elementary result in stream order, AFTER the other elementary streams of the packet have been decoded: the
 * reference stops at the failing stream (:876-878), here every stream goes on (a deliberate difference; an elementary stream
 * itself still stops at its first failing frame, as opus_decode_native does).  Nothing is written to the PCM block of a packet
 * whose result is negative, and a block is written only as far as its result reaches.
 * Empty packets (packets[i] == NULL or lens[i] == 0): reference mode runs the empty-packet branch (EMPTY PACKETS above) on every
 * elementary stream, frame_size / 960 passes each (:851-874 with do_plc); RFC mode conceals a lost packet on every elementary
 * stream, as opusgpu_decode_packets does for one stream.  RFC mode: elementary streams may differ in frame count and frame
 * duration (their durations are equal), result[i] is the packet's duration. */
int opusgpu_ms_decode_packets(opusgpu_ms *ms, int n, const int32_t *decoder_ids, const uint8_t *const *packets,
                              const int32_t *lens, int16_t *pcm, int frame_capacity, int32_t *result);
/* One device step of n multistream frames: d_descs holds n rows of `streams` descriptors (row r = one multistream frame, its
 * elementary frames in stream order; every descriptor's `stream` field names the DECODER, 0 .. n_decoders - 1), payload bytes in
 * d_arena (16-byte aligned, as for opusgpu_decode_step_device); d_pcm (16-byte aligned) receives [n][960 * channels] int16
 * (RFC mode: [n][OPUSGPU_RFC_FRAME_SAMPLES * channels], d_result[r] the row's sample count), d_result[n] int32 the row's common
 * sample count or its first negative elementary result in stream order.  Asynchronous on `hip_stream` (NULL: the object's own
 * stream); consecutive steps on different streams are ordered by a drain.  A row decodes one frame of each elementary stream of
 * its decoder, so a decoder appears at most once per step.  Checked on the device, per row: a row whose descriptors name
 * different decoders, a decoder out of range, a mode value of 3, another mode than the object's (the RFC bit), the FEC bit, or
 * (RFC mode) frames of different durations gets OPUSGPU_BAD_ARG and none of its elementary frames is decoded.  Empty packets
 * take one row per pass (reference mode) or per concealed frame (RFC mode), with the descriptors opusgpu_empty_packet_to_frames
 * makes (decoder channel count 2 for coupled streams, 1 for mono ones).  Rows with a negative result get no PCM. */
int opusgpu_ms_decode_step_device(opusgpu_ms *ms, int n, const void *d_descs, const void *d_arena, void *d_pcm, void *d_result,
                                  void *hip_stream);
/* The host waits for everything the object has queued. */
int opusgpu_ms_synchronize(opusgpu_ms *ms);

/* ---- WHOLE FILES: N Ogg Opus files in, N trimmed PCM tracks in HBM out ------------------------------------------------------
 * The page path above ends at per-step PCM blocks and leaves pre-skip, end trimming, holes and spanning packets to the caller; the
 * file surface (include/opusfile.h) handles all of those, one stream per process.  This section joins the two: a host planner
 * that runs the single-file reader's own bookkeeping (csrc/og_container.hpp: op_find_initial_pcm_offset, op_fetch_and_process_page
 * and the deciding half of op_read_native, src/opusfile.cpp:486-632, :835-1133, :1207-1260) over every file without decoding, and
 * a kernel that copies every decoded frame's kept samples to their place in the file's track.
 * File i is decoder stream i.  The k-th frame of a file goes in step k (a stream at most once per step); step tables and arena
 * are in the device layout of the page batch (16-byte arena tail; OPUSGPU_PAGES_GROUP_BY_MODE / _ORDER_BY_HEADER order a step's
 * table the same way).  In RFC mode the descriptors carry duration and RFC bit as opusgpu_packet_to_frames_mode makes them.
 * On OP_HOLE (-3) the planner does what a caller does who notes it and reads on (holes are counted); any other negative reader
 * code ends the file's plan there and is reported in status -- what was planned before it is decoded.  Chained links are not
 * followed (the reader stops at a new link).  The OpusHead output gain is reported, not applied (the reference does not apply it).
 * Refusals, per file, never a failed call (a refused file contributes no frame and a track of 0 samples):
 *   OpusHead channel count != `channels`  -> OPUSGPU_BAD_ARG (a mono file on a stereo context is not the same decoder, Q3);
 *   mapping family != 0                   -> OPUSGPU_UNIMPLEMENTED (family 1: WHOLE FILES / MULTISTREAM below);
 *   reference mode, an audio packet whose TOC names another frame duration than 20 ms -> OPUSGPU_UNIMPLEMENTED.  What the
 *     single-file reader makes of such a packet: the decoder writes 960 samples per frame whatever the TOC says (Q6) and the reader
 *     hands out the TOC's duration from its scratch buffer -- the head of a frame decoded at the wrong length (2.5 / 5 / 10 ms), or
 *     960 fresh samples followed by whatever an earlier packet left there (40 / 60 ms).  Nobody wants that: such files are RFC mode's.
 *   A packet with a valid duration that fails the frame split ends the plan with OP_EBADPACKET (-136), where the reader's decode
 *   callback would have failed.
 * SEGMENTS.  One per descriptor of a step, in slot order (32 bytes, little-endian, this layout is part of the ABI):
 *   "copy `count` samples per channel of PCM row `slot` of this step, starting at sample `src_first` of the row, to sample
 *   `dst_first` of the packed track buffer" -- dst_first counts samples per channel from the start of the buffer, i.e. the track's
 *   offset (opusgpu_file_info.track_offset) plus the position in the track.  A frame cut by pre-skip or end trimming has a
 *   shortened segment; a frame that is skipped or trimmed entirely keeps a segment of count 0, which copies nothing: its result
 *   code still counts (the reader decodes such packets too and fails on them).
 * FAILED FRAMES.  A segment whose frame's result is negative writes nothing and lowers first_bad of its track's state record to
 * its packet_seq (atomic minimum), recording the code; a segment whose packet_seq is >= its track's first_bad writes nothing.  A
 * track's final length is the planned start of packet first_bad -- where the single-file reader would have returned
 * OP_EBADPACKET.  Samples at or past the final length are unspecified (earlier frames of the failing packet may have landed
 * there).  Later frames of such a stream are still decoded; only their output is dropped. */
typedef struct opusgpu_track_seg { /* 32 bytes */
    int32_t slot;       /* PCM row (and result entry) of the step */
    int32_t src_first;  /* first sample per channel taken from the row */
    int32_t count;      /* samples per channel; 0: nothing to copy */
    int32_t track;      /* file index = state record */
    int64_t dst_first;  /* sample per channel in the packed track buffer */
    int32_t packet_seq; /* index of the audio packet in its file, 0-based, counted over the packets the reader hands to the decoder */
    int32_t reserved;   /* 0 */
} opusgpu_track_seg;
typedef struct opusgpu_track_state { /* 8 bytes, one per track; before the first step: { INT32_MAX, 0 } */
    int32_t first_bad; /* lowest packet_seq with a failed frame */
    int32_t code;      /* that frame's result */
} opusgpu_track_state;
typedef struct opusgpu_file_info { /* 48 bytes */
    int32_t status;         /* 0, a refusal (above), or the reader's code: e.g. -132 OP_ENOTFORMAT, -133 OP_EBADHEADER, -136 OP_EBADPACKET, -139 OP_EBADTIMESTAMP */
    int32_t channels;       /* OpusHead: channel count, pre-skip, output gain (Q7.8 dB), mapping family; 0 when no header was found */
    int32_t pre_skip;
    int32_t output_gain;
    int32_t mapping_family;
    int32_t packets;        /* audio packets planned */
    int32_t frames;         /* frames planned = steps the file takes part in */
    int32_t holes;
    int64_t track_samples;  /* planned track length, samples per channel */
    int64_t track_offset;   /* where the track begins in the packed buffer, samples per channel; a multiple of 64: every track
                               begins on a 128-byte boundary */
} opusgpu_file_info;
typedef struct opusgpu_file_batch opusgpu_file_batch;

/* files[i]: file_lens[i] bytes, a complete Ogg Opus file in memory.  channels 1 or 2; mode OPUSGPU_MODE_REFERENCE or _RFC; flags
 * OPUSGPU_PAGES_GROUP_BY_MODE / OPUSGPU_PAGES_ORDER_BY_HEADER or 0; threads <= 0: one.  info (n_files entries) may be NULL.
 * Returns OPUSGPU_OK, OPUSGPU_BAD_ARG or OPUSGPU_ALLOC_FAIL.  Host only: no GPU involved. */
int opusgpu_files_plan(int n_files, const uint8_t *const *files, const int64_t *file_lens, int channels, int mode, int flags,
                       int threads, opusgpu_file_info *info, opusgpu_file_batch **out);
int opusgpu_file_batch_steps(const opusgpu_file_batch *b);
/* Step `step`: returns its descriptor count; *descs its table, *slot_files (may be NULL) the file of every slot, *modes (may be
 * NULL) what the step may be declared as: OPUSGPU_HAS_* of the modes that occur, plus OPUSGPU_STEP_KEEPS_MODE when no file with
 * a frame in the step has changed its mode up to and including that frame. */
int opusgpu_file_batch_step(const opusgpu_file_batch *b, int step, const opusgpu_frame_desc **descs, const int32_t **slot_files,
                            int *modes);
/* The step's segment list (one per descriptor, slot order); returns the count. */
int opusgpu_file_batch_segments(const opusgpu_file_batch *b, int step, const opusgpu_track_seg **segs);
const uint8_t *opusgpu_file_batch_arena(const opusgpu_file_batch *b, size_t *bytes);
/* Samples per channel of the packed track buffer (the last track's offset + length, rounded up to 64): allocate 2 * channels
 * bytes for each. */
int64_t opusgpu_file_batch_track_samples(const opusgpu_file_batch *b);
/* The planned start (sample per channel, track-relative) of packet `packet_seq` of file `file`; packet_seq == the file's packet
 * count gives the planned track length.  -1 for bad arguments. */
int64_t opusgpu_file_batch_packet_start(const opusgpu_file_batch *b, int file, int packet_seq);
void opusgpu_file_batch_free(opusgpu_file_batch *b);

/* k_tracks_assemble: applies n_segs segments (device array of opusgpu_track_seg) to d_pcm [rows][row_samples * channels] int16
 * (16-byte aligned; row_samples 960, or OPUSGPU_RFC_FRAME_SAMPLES in RFC mode) with the step's results d_result, into the packed
 * track buffer d_tracks (128-byte aligned) with the state records d_track_state.  The caller guarantees that every segment lies
 * inside its row (0 <= src_first, src_first + count <= row_samples) and inside the track buffer, and that segments of one call
 * do not overlap in the buffer.  Asynchronous on the context's stream (or `hip_stream`): queued behind a decode step on the same
 * stream it needs no other ordering. */
int opusgpu_tracks_assemble_device(opusgpu_ctx *ctx, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                   const void *d_result, void *d_tracks, void *d_track_state, void *hip_stream);
/* Everything at once: uploads the batch, gives streams 0 .. n_files - 1 of the context fresh state, runs the steps with the
 * assembly behind each on the context's stream and waits.  The context must have at least n_files streams of the batch's channel
 * count and be in the batch's mode (OPUSGPU_BAD_ARG otherwise).  With opusgpu_set_pipeline on, every step is declared with the
 * modes the planner found (see opusgpu_file_batch_step), so steps run ahead of each other exactly as declared steps do; otherwise
 * they run in order.  The assembly adds no drain: it is queued on the steps' stream, and every kernel of step k + 1 that writes
 * PCM or result codes runs on that stream (or one forked from it) -- ONE step PCM buffer is all the pipeline depth needs, since only
 * parse and reconstruction kernels, which never touch it, run ahead.
 * d_tracks: opusgpu_file_batch_track_samples x channels int16 in HBM, 128-byte aligned.  track_lengths_out[i] (may be NULL): the
 * final length of track i in samples per channel.  status_out (may be NULL) gets two entries per file: [2 * i] = the first
 * failed frame's code (e.g. OPUSGPU_CELT_BAD_ARG), else the plan's status; [2 * i + 1] = the failing packet's packet_seq, or -1. */
int opusgpu_files_decode(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, void *d_tracks, int64_t *track_lengths_out,
                         int32_t *status_out);

/* TRACK FORMATS.  opusgpu_files_decode ends at interleaved int16, what parity with the reference is judged on.  The calls below
 * write the tracks in the form a consumer converts them to anyway, in the same pass:
 *   VALUE.  Every float sample is (float)s * scale[track]: s the int16 sample the S16 path writes at that place (multistream: after
 *   the channel mapping, a muted channel is 0), one IEEE single-precision multiply, nothing fused or contracted -- the float tracks
 *   are a pure function of the S16 tracks, bit for bit.  The default scale is 1.0f / 32768, which is exact.
 *   LAYOUT.  The packed buffer has opusgpu_file_batch_track_samples x channels elements whatever the format, of 4 bytes for the float
 *   formats.  OPUSGPU_TRACKS_F32: the element index is the S16 element index.  OPUSGPU_TRACKS_F32_PLANAR: sample n of channel c of
 *   track t is element  channels * track_offset[t] + c * plane[t] + n,  plane[t] = the track's PLANNED track_samples rounded up to
 *   64.  The planner packs tracks at multiples of 64 samples and begins the next track at the rounded-up end of this one
 *   (opusgpu_file_info.track_offset), so the planes of track t fill exactly the elements its interleaved form would, and every
 *   plane begins on a 256-byte boundary.  A track cut short by a failed frame keeps its planned plane stride; only its reported
 *   length shrinks.
 *   FAILED FRAMES are what they are above: a failed frame writes nothing and lowers first_bad, segments at or behind first_bad
 *   write nothing, the final length is the planned start of the failing packet, elements past it are unspecified.  Padding between
 *   tracks and between planes is never written. */
#define OPUSGPU_TRACKS_S16 0        /* interleaved int16: what opusgpu_files_decode writes */
#define OPUSGPU_TRACKS_F32 1        /* interleaved float32, same sample positions */
#define OPUSGPU_TRACKS_F32_PLANAR 2 /* float32, one contiguous plane per channel and track */
typedef struct opusgpu_track_place { /* 24 bytes, one per track, read by the float kernels through opusgpu_track_seg.track (ABI) */
    int64_t track_offset;  /* where the track begins in the packed buffer, samples per channel; a multiple of 64 */
    int64_t plane_samples; /* planar: distance between the track's planes in samples, a multiple of 64; interleaved: not read */
    float scale;
    int32_t reserved;      /* 0 */
} opusgpu_track_place;
/* The OpusHead output gain (Q7.8 dB, RFC 7845 section 5.1; opusgpu_file_info.output_gain) as a linear factor, folded with the
 * 1 / 32768 of the float formats: (float)(pow(10, q8 / 5120.0) / 32768).  Host only. */
float opusgpu_head_gain_scale(int32_t output_gain_q8);
/* opusgpu_tracks_assemble_device for any format.  OPUSGPU_TRACKS_S16 with d_place NULL is that call; S16 with a d_place, or an
 * unknown format, is OPUSGPU_BAD_ARG.  For the float formats d_tracks holds floats (128-byte aligned, as above) and d_place is a
 * device array of opusgpu_track_place, 8-byte aligned, with a record for every `track` the segments name.  Planar: the caller
 * guarantees track_offset <= dst_first of the track's segments, both multiples as the record says, and that the planes lie inside
 * the buffer.  The other alignment rules and guarantees are those of opusgpu_tracks_assemble_device. */
int opusgpu_tracks_assemble_device_as(opusgpu_ctx *ctx, int n_segs, const void *d_segs, const void *d_pcm, int row_samples,
                                      const void *d_result, int format, const void *d_place, void *d_tracks, void *d_track_state,
                                      void *hip_stream);
/* opusgpu_files_decode into tracks of `format`.  scale: host array of n_files floats, or NULL for 1 / 32768 each.  With
 * OPUSGPU_TRACKS_S16 and scale NULL this is opusgpu_files_decode; S16 with a scale is OPUSGPU_BAD_ARG (integer gain has rounding
 * rules of its own and is not offered), as are an unknown format and a scale entry that is not finite.  d_tracks:
 * opusgpu_file_batch_track_samples x channels elements of the format, 128-byte aligned.  The place table is built from the batch,
 * uploaded before the first step and freed before the call returns, also when it fails; steps, buffers and ordering are those of
 * opusgpu_files_decode -- none of them depends on the format. */
int opusgpu_files_decode_as(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int format, const float *scale, void *d_tracks,
                            int64_t *track_lengths_out, int32_t *status_out);

/* TRACK RATES.  Tracks at 48000 / D Hz, D in {2, 3, 4, 6} (rates 24000, 16000, 12000, 8000), and a mono downmix of mono or stereo
 * tracks; rate 48000 is allowed only together with `mono`.  Like the float formats the new tracks are a pure function of the S16
 * track, bit for bit:
 *   VALUE.  For track t let x[n] be the int16 sample of the S16 track, and x[n] = 0 for n < 0 and for n >= the track's FINAL length
 *   (samples at or past the final length are unspecified in the buffer and are never read as signal).  With `mono` (1 or 2
 *   channels only) x is first replaced by (l + r + 1) >> 1 for stereo and is unchanged for mono, and there is one output channel.
 *   Output sample m of each channel, for m in [0, ceil(len / D)), len the final length, is
 *       y[m] = sat16((sum_k h_D[k] * x[m * D + k - (L - 1) / 2] + 16384) >> 15),     k in [0, L), L = 24 D + 1,
 *   >> arithmetic, the accumulation exact in int32 (sum |h_D| <= 65535, asserted where the taps are made), sat16 a clamp to
 *   [-32768, 32767].  With rate 48000 the downmix is the whole operation (h = {32768}: y = x).  The float formats follow TRACK
 *   FORMATS: (float)y * scale[track], one IEEE multiply.
 *   TAPS.  h_D is one symmetric Q15 table of int16: scipy.signal.firwin(L, 0.92 / D, window=("kaiser", 8.0)) rounded to Q15, the
 *   centre tap corrected so that the sum is exactly 32768 (tools/gen_resample_taps.py writes them to csrc/og_resample_taps.hpp).
 *   LAYOUT.  Resampled tracks are packed on a grid of their own: out_offset[t] is the running sum of roundup64(ceil(planned[u] / D))
 *   over the earlier tracks u, planned the PLANNED track_samples -- always a multiple of 64.  Interleaved formats: sample m of
 *   channel c of track t is element out_channels * (out_offset[t] + m) + c.  OPUSGPU_TRACKS_F32_PLANAR: element out_channels *
 *   out_offset[t] + c * plane[t] + m, plane[t] = roundup64(ceil(planned[t] / D)).  out_channels is 1 with `mono`, else the channel
 *   count.  Padding is never written. */
/* The taps of `rate`: returns L and sets *taps (may be NULL) to the table, or OPUSGPU_BAD_ARG for a rate without a table -- 48000
 * included, whose single tap 32768 is no int16.  Host only. */
int opusgpu_resample_taps(int rate, const int16_t **taps);
/* The grid above for n tracks of planned_samples[i] samples: writes out_offsets[i] (may be NULL) and returns the total in samples
 * per channel -- allocate out_channels elements of the format for each.  Serves both kinds of batch.  OPUSGPU_BAD_ARG for an unknown
 * rate (48000 is known: D = 1) or a negative length.  Host only. */
int64_t opusgpu_resample_layout(int n, const int64_t *planned_samples, int rate, int64_t *out_offsets);
typedef struct opusgpu_resample_span { /* 40 bytes, one per track (ABI) */
    int64_t in_offset;  /* where the S16 track begins in d_in, samples per channel; a multiple of 8 */
    int64_t in_samples; /* its FINAL length */
    int64_t out_offset; /* where the resampled track begins in d_out, samples per channel; a multiple of 64 */
    int64_t out_plane;  /* planar: distance between the track's planes, a multiple of 64 and >= ceil(in_samples / D); else not read */
    float scale;        /* float formats; not read for OPUSGPU_TRACKS_S16 */
    int32_t reserved;   /* 0 */
} opusgpu_resample_span;
/* k_tracks_resample alone: d_in holds packed interleaved int16 tracks of `channels` (1 - 8) channels, 16-byte aligned; `spans` is a
 * HOST array of n_tracks records.  Writes the tracks of TRACK RATES into d_out (128-byte aligned) in `format`.  The kernel reads
 * d_in in aligned 16-byte pieces: the buffer must reach to the end of the piece that holds a track's last sample (a buffer of
 * opusgpu_file_batch_track_samples does).  The caller guarantees that the spans lie inside both buffers and do not overlap in
 * d_out.  Uploads the records and its tile table, launches on the context's stream (or `hip_stream`), waits, and frees both on
 * every way out.  OPUSGPU_BAD_ARG before any device work: an unknown rate or format, 48000 without `mono`, `mono` with more than 2
 * channels, a span that breaks the rules above, a scale that is not finite with a float format. */
int opusgpu_tracks_resample_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_resample_span *spans, const void *d_in, int channels,
                                   int rate, int mono, int format, void *d_out, void *hip_stream);
/* opusgpu_files_decode into resampled tracks: allocates a scratch S16 track buffer (opusgpu_file_batch_track_samples x channels x 2
 * bytes), runs opusgpu_files_decode into it -- steps, assembly and ordering unchanged --, takes the final lengths from its
 * outcome, runs k_tracks_resample into d_out and frees the scratch on every way out.  d_out: opusgpu_resample_layout's total x
 * out_channels elements of `format`, 128-byte aligned.  scale as for opusgpu_files_decode_as.  out_offsets[i] and out_lengths[i]
 * (either may be NULL): where resampled track i begins and its length ceil(final / D); track_lengths_out and status_out as for
 * opusgpu_files_decode (the lengths at 48 kHz).  OPUSGPU_BAD_ARG before any device work: an unknown rate or format, 48000 without
 * `mono`, `mono` with more than 2 channels, a scale with OPUSGPU_TRACKS_S16, a scale entry that is not finite.  On a failure the
 * caller's arrays are left as they were. */
int opusgpu_files_decode_resampled(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int mono, int format, const float *scale,
                                   void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                                   int32_t *status_out);

/* CHANNEL MIX.  A matrix in front of TRACK RATES: surround to stereo or mono, one channel of a pair, a swap, mid / side, any
 * weighting.  A mix is out_channels (1 - 8) rows of in_channels (1 - 8) int16 coefficients in Q14, M[o][c].
 *   VALUE.  For a track with int16 samples s_c[n], zero in front of the track and at or behind its FINAL length as in TRACK RATES,
 *       x_o[n] = sat16((sum_c M[o][c] * s_c[n] + 8192) >> 14),
 *   >> arithmetic, the sum exact in int32.  Then TRACK RATES applies to x as if it were the S16 track of out_channels channels: the
 *   FIR and its sat16((sum + 16384) >> 15), the float formats, the LAYOUT with out_channels as its channel count.  Rate 48000 is
 *   allowed with a mix and is the mix alone.  There is no `mono` next to a matrix.
 *   REFUSED before any device work (OPUSGPU_BAD_ARG): out_channels or in_channels outside 1 - 8; in_channels other than the tracks'
 *   channel count; a row with sum_c |M[o][c]| > 65535 (up to there 65535 * 32768 + 8192 < 2^31: the argument the taps use).
 *   Entries of m[][] outside the matrix are not read.
 *   The row {8192, 8192} is exactly `mono`'s (l + r + 1) >> 1; 16384 on the diagonal is exactly x = s.
 *   DEFAULT TABLES.  opusgpu_downmix_matrix fills the matrix that takes `channels` (1 - 8) channels in the Vorbis order of channel
 *   mapping family 1 to stereo or mono.  The tables are defined here, not taken from a codec.  Speaker order: 1: M; 2: FL FR; 3: FL C FR;
 *   4: FL FR RL RR; 5: FL C FR RL RR; 6: FL C FR RL RR LFE; 7: FL C FR SL SR RC LFE; 8: FL C FR SL SR RL RR LFE.  Stereo weights
 *   (left, right) before normalisation: FL (1, 0), FR (0, 1), C and M (1/sqrt 2, 1/sqrt 2), SL and RL (1/sqrt 2, 0), SR and RR
 *   (0, 1/sqrt 2), RC (1/2, 1/2), LFE (0, 0); the mono row's weights are left + right.  Each row is rint(16384 w / sum(w)), and its
 *   largest entry (the first of them when tied) is then corrected so that the row sums to exactly 16384: entries are >= 0, so a
 *   default mix never clamps (tools/gen_downmix_tables.py writes them to csrc/og_downmix_tables.hpp). */
typedef struct opusgpu_mix_matrix { /* 136 bytes (ABI) */
    int32_t out_channels, in_channels;
    int16_t m[8][8]; /* m[o][c], Q14; unused entries 0 */
} opusgpu_mix_matrix;
/* The default table for `channels` (1 - 8) and out_channels 1 or 2 into *m, unused entries 0; anything else, or m NULL, is
 * OPUSGPU_BAD_ARG.  Host only. */
int opusgpu_downmix_matrix(int channels, int out_channels, opusgpu_mix_matrix *m);
/* k_tracks_resample_mix alone: opusgpu_tracks_resample_device's contract and refusals with *mix in place of `mono`, plus REFUSED
 * above and a NULL mix; every rate of TRACK RATES, 48000 included.  d_out holds mix->out_channels channels. */
int opusgpu_tracks_resample_mixed_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_resample_span *spans, const void *d_in, int channels,
                                         int rate, const opusgpu_mix_matrix *mix, int format, void *d_out, void *hip_stream);
/* opusgpu_files_decode_resampled with *mix in place of `mono`: the same scratch S16 buffer, the same decode, the same grid with
 * mix->out_channels as out_channels.  OPUSGPU_BAD_ARG before any device work: an unknown rate or format, a matrix that REFUSED
 * names (or NULL), a scale with OPUSGPU_TRACKS_S16, a scale entry that is not finite.  On a failure the caller's arrays are left as
 * they were. */
int opusgpu_files_decode_mixed(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, const opusgpu_mix_matrix *mix, int format,
                               const float *scale, void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                               int32_t *status_out);

/* TRACK RATIOS.  Tracks at 48000 * up / down Hz by a rational polyphase FIR, for the rates that do not divide 48000: 44100 is
 * 147 / 160, 32000 is 2 / 3, 22050 is 147 / 320.  The arguments are those of scipy.signal.resample_poly(x, up, down).  Like TRACK
 * RATES the result is a pure function of the S16 track, bit for bit, in exact integer arithmetic.  TRACK RATES, its taps and its
 * refusals (rate 44100, rate 32000) are unchanged: this is a section of its own with calls of its own.
 *   RATIO.  up and down are divided by their gcd first.  The reduced pair must keep 1 <= up <= 160 and up < down <=
 *   min(8 * up, 640); everything else is OPUSGPU_BAD_ARG before any device work.  147/160, 2/3, 147/320 and 147/640 are inside, and so
 *   are the plain 1 / D, which go through THIS filter with THIS section's taps -- 1 / 2 is not promised to equal rate 24000.
 *   VALUE.  Let x[n] be the int16 track after `mono` or the mix, exactly as TRACK RATES and CHANNEL MIX define it (`mono`: (l + r +
 *   1) >> 1 of a stereo track; a mix: sat16((sum_c M[o][c] * s_c[n] + 8192) >> 14)), x[n] = 0 for n < 0 and for n >= the track's
 *   FINAL length len.  With Lp = 24 * down + 1 and c = 12 * down, output sample m of each channel, for m in [0, ceil(len * up /
 *   down)), is
 *       y[m] = sat16((sum_n h[m * down + c - n * up] * x[n] + 16384) >> 15),
 *   the sum over those n whose tap index m * down + c - n * up lies in [0, Lp), >> arithmetic, the sum exact in int32, sat16 a
 *   clamp to [-32768, 32767]: a filter on the 48000 * up grid of which every output takes one phase, the taps h[p], h[p + up], ...
 *   with p = (m * down + c) mod up.  The float formats follow TRACK FORMATS: (float)y * scale[track], one IEEE multiply.
 *   TAPS.  h is an int16 table of Lp entries in Q15, built in double at first use, kept per reduced (up, down) for the life of the
 *   process, safe to ask for from any number of threads.  The prototype is TRACK RATES' design moved to the fine grid,
 *       g[i] = fc * sinc(fc * (i - c)) * I0(8 * sqrt(1 - ((i - c) / c)^2)) / I0(8),   fc = 0.92 / down,  sinc(t) = sin(pi t) / (pi t):
 *   a Kaiser window of beta 8 over a low-pass at 0.92 of the OUTPUT's Nyquist.  Each of the up phases g[p], g[p + up], ... is
 *   scaled to sum 32768 and rounded to nearest; the phase's largest rounded tap (the first of them when tied) is then corrected so
 *   that the phase sums to exactly 32768: every phase has a DC gain of exactly 1, a constant track comes back as it is.  The
 *   builder holds sum |h_phase| <= 65535 for every phase (65535 * 32768 + 16384 < 2^31: the argument that makes TRACK RATES' sum
 *   exact), and a ratio whose table broke that would be refused like one outside RATIO.  The table is NOT promised to be
 *   symmetric -- the correction breaks the symmetry for 2 / 3 -- and sin, sqrt and the rounding are the host's: the table that
 *   opusgpu_resample_ratio_taps hands out is the definition, and tests compute against it.
 *   LAYOUT.  TRACK RATES' grid with ceil(planned * up / down) in place of ceil(planned / D): out_offset[t] is the running sum of
 *   roundup64(ceil(planned[u] * up / down)); tracks begin at multiples of 64 samples, the planes of OPUSGPU_TRACKS_F32_PLANAR are
 *   roundup64(ceil(planned[t] * up / down)) long; padding is never written.  opusgpu_resample_span is reused, its out_plane a
 *   multiple of 64 and >= ceil(in_samples * up / down).
 *   ARITHMETIC.  Everything that multiplies a sample index by up or down is 64-bit. */
/* The taps of up / down: returns Lp = 24 * down' + 1 for the reduced down' and sets *taps (may be NULL) to the table, which stays
 * valid for the life of the process; OPUSGPU_BAD_ARG for a ratio outside RATIO.  Host only. */
int opusgpu_resample_ratio_taps(int up, int down, const int16_t **taps);
/* LAYOUT above for n tracks of planned_samples[i] samples: writes out_offsets[i] (may be NULL) and returns the total in samples per
 * channel.  Serves both kinds of batch.  OPUSGPU_BAD_ARG for a ratio outside RATIO or a negative length.  Host only. */
int64_t opusgpu_resample_ratio_layout(int n, const int64_t *planned_samples, int up, int down, int64_t *out_offsets);
/* k_tracks_resample_ratio alone: opusgpu_tracks_resample_mixed_device's contract and refusals with the ratio in place of the rate
 * -- d_in packed interleaved int16 tracks of `channels` (1 - 8) channels, 16-byte aligned, read in aligned 16-byte pieces up to the
 * one that holds a track's last sample; `spans` a HOST array; d_out 128-byte aligned; uploads the spans, the tile table and the tap
 * rows, launches on the context's stream (or `hip_stream`), waits, frees them on every way out.  mix NULL: no matrix, and `mono` as
 * in opusgpu_tracks_resample_device (1 or 2 channels) or all channels.  OPUSGPU_BAD_ARG before any device work: a ratio outside
 * RATIO, an unknown format, `mono` with more than 2 channels, `mono` together with a mix, a matrix that CHANNEL MIX refuses, a span
 * that breaks the rules, a scale that is not finite with a float format. */
int opusgpu_tracks_resample_ratio_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_resample_span *spans, const void *d_in, int channels,
                                         int up, int down, int mono, const opusgpu_mix_matrix *mix /* NULL: none */, int format, void *d_out,
                                         void *hip_stream);
/* opusgpu_files_decode_mixed with the ratio in place of the rate, and `mono` where there is no matrix (mix NULL): the same scratch
 * S16 buffer, the same decode, LAYOUT above with the output channels as its channel count; out_lengths[i] = ceil(final * up /
 * down).  OPUSGPU_BAD_ARG before any device work: what opusgpu_tracks_resample_ratio_device refuses of its ratio, format, `mono`
 * and mix, a scale with OPUSGPU_TRACKS_S16, a scale entry that is not finite.  On a failure the caller's arrays are left as they
 * were. */
int opusgpu_files_decode_ratio(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int up, int down, int mono,
                               const opusgpu_mix_matrix *mix /* NULL: none */, int format, const float *scale, void *d_out,
                               int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out, int32_t *status_out);

/* TRACK FEATURES.  Log-mel features of the mono track at 16 kHz, the front end of Whisper-style speech models, in the same call
 * that decodes the files.  Like the float formats, the rates and the mix, the features are a function of an array that is pinned
 * bit for bit; they are themselves float sums, pinned to a tolerance and to two exact properties (below).
 *   INPUT.  The int16 mono track at 16 kHz exactly as TRACK RATES / CHANNEL MIX define it -- `mono` on a 1- or 2-channel context, or
 *   a mix with out_channels == 1 on either kind of context --: y[m], m in [0, n), n = ceil(final_48k / 3).
 *   CONSTANTS of this version (not fields): n_fft 400, hop 160, sr 16000, fmin 0, fmax 8000, 201 power bins.
 *   FRAMES.  F = n / 160 (floor): torch.stft(center=True) without its last frame, as Whisper does.
 *   WINDOW INDEX.  Frame f, tap i in [0, 400) reads index q = 160 f - 200 + i, reflected ONCE: q < 0 becomes -q, q >= n becomes
 *   2 (n - 1) - q; if q is still outside [0, n) the sample is 0 (that happens only for n < 201).
 *   SAMPLE.  x_i = (float)y[q] * scale[track], one IEEE multiply; the default scale is 1 / 32768 (the scale rule of TRACK FORMATS).
 *   POWER.  P[k] = (sum_i Wc[i][k] x_i)^2 + (sum_i Ws[i][k] x_i)^2, k in [0, 201).
 *   MEL.  mel[j] = sum_k B[j][k] P[k], j in [0, n_mels).
 *   OUTPUT.  log10f(max(mel[j], 1e-10f)), float32.  Whisper's clip-wide max - 8 clamp and (x + 4) / 4 are two element-wise
 *   operations on the result and are left to the caller -- or to FEATURE BATCHES (below), which applies them per track while it
 *   pads the features into one tensor.
 *   TABLES.  float32, each entry computed in double and rounded once, at first use (once per process):
 *       w[i] = 0.5 - 0.5 cos(2 pi i / 400)                       the periodic Hann window
 *       Wc[i][k] = w[i] cos(a), Ws[i][k] = w[i] sin(a),           a = 2 pi ((i k) mod 400) / 400: 2 pi i k / 400 reduced in integers
 *       B: Slaney's scale, Slaney's normalisation, the formula librosa.filters.mel(sr=16000, n_fft=400, n_mels=n_mels) implements:
 *         hz(m) = 200 / 3 * m for m < 15, else 1000 exp((ln 6.4 / 27) (m - 15));   mmax = 15 + ln(8) / (ln 6.4 / 27)   (8000 Hz)
 *         p[j] = hz(j * (mmax / (n_mels + 1))) for j in [0, n_mels], p[n_mels + 1] = hz(mmax)      n_mels + 2 points over [0, 8000] Hz
 *         B[j][k] = max(0, min((40 k - p[j]) / (p[j + 1] - p[j]), (p[j + 2] - 40 k) / (p[j + 2] - p[j + 1]))) * (2 / (p[j + 2] - p[j]))
 *     opusgpu_mel_basis and opusgpu_mel_filterbank hand them out: a test or a user computes against exactly the numbers the kernel
 *     multiplies.
 *   SUMMATION ORDER is not part of the contract (the kernel folds the window's symmetry: x_i +- x_{400 - i} against half the basis).
 *   What is: the same call on the same input returns the same bits -- no float atomics, no sum that depends on the launch order --,
 *   and an all-zero track gives one bit-identical value in every cell.  tests/test_gpu_tracks_mel.py holds the kernel to a
 *   float64 reference within 8 x the error of a float32 restatement.
 *   LAYOUT.  Feature tracks lie on a grid of their own, in floats: plane[t] = roundup64(ceil(planned[t] / 3) / 160), planned the
 *   PLANNED track_samples at 48 kHz; feat_offset[t] is the running sum of n_mels * plane[u] over the earlier tracks u, a multiple
 *   of 64 floats, in BOTH layouts.  OPUSGPU_MEL_BANDS_MAJOR: band j of frame f is element feat_offset[t] + j * plane[t] + f ([n_mels]
 *   [frames], what Whisper takes).  OPUSGPU_MEL_FRAMES_MAJOR: element feat_offset[t] + f * n_mels + j.  Padding is never written.  A
 *   track cut short by a failed frame keeps its planned plane and reports its shorter F. */
#define OPUSGPU_MEL_NFFT 400
#define OPUSGPU_MEL_HOP 160
#define OPUSGPU_MEL_SR 16000
#define OPUSGPU_MEL_FMIN 0
#define OPUSGPU_MEL_FMAX 8000
#define OPUSGPU_MEL_BINS 201
#define OPUSGPU_MEL_BANDS_MAJOR 0  /* [n_mels][frames], the band's row plane[t] floats long */
#define OPUSGPU_MEL_FRAMES_MAJOR 1 /* [frames][n_mels] */
typedef struct opusgpu_mel_params { /* 32 bytes (ABI) */
    int32_t n_mels;      /* 80 or 128 */
    int32_t layout;      /* OPUSGPU_MEL_BANDS_MAJOR or OPUSGPU_MEL_FRAMES_MAJOR */
    int32_t reserved[6]; /* 0 */
} opusgpu_mel_params;
/* The DFT basis: sets *wc and *ws (either may be NULL) to Wc and Ws, [400][201] floats each, and returns 400 * 201.  Host only. */
int opusgpu_mel_basis(const float **wc, const float **ws);
/* The filterbank of n_mels (80 or 128) bands: sets *b (may be NULL) to B, [n_mels][201] floats, and returns n_mels * 201;
 * OPUSGPU_BAD_ARG for any other n_mels.  Host only. */
int opusgpu_mel_filterbank(int n_mels, const float **b);
/* The grid above for n tracks of planned_48k_samples[i] samples at 48 kHz: writes feat_offsets[i] (may be NULL) and returns the total
 * in floats.  Serves both kinds of batch.  OPUSGPU_BAD_ARG: params NULL, n_mels not 80 or 128, an unknown layout, a reserved word
 * that is not 0, a negative length.  Host only. */
int64_t opusgpu_mel_layout(int n, const int64_t *planned_48k_samples, const opusgpu_mel_params *params, int64_t *feat_offsets);
typedef struct opusgpu_mel_span { /* 40 bytes, one per track (ABI) */
    int64_t in_offset;  /* where the int16 mono track begins in d_in16k_mono, in samples; a multiple of 8 */
    int64_t in_samples; /* n, its length at 16 kHz */
    int64_t out_offset; /* where the feature track begins in d_out, in floats; a multiple of 64 */
    int64_t plane;      /* a multiple of 64 and >= n / 160; bands-major: the distance between two bands' rows; frames-major: not read */
    float scale;
    int32_t reserved;   /* 0 */
} opusgpu_mel_span;
/* k_tracks_mel alone: d_in16k_mono holds packed int16 mono tracks at 16 kHz, 16-byte aligned; `spans` is a HOST array of n_tracks
 * records.  Writes the features of TRACK FEATURES into d_out (floats, 128-byte aligned).  The kernel reads d_in16k_mono in aligned
 * 16-byte pieces: the buffer must reach to the end of the piece that holds a track's last sample.  The caller guarantees that the
 * spans lie inside both buffers and do not overlap in d_out.  A track with n < 160 has no frame and writes nothing.  Uploads the
 * records, its tile table and the tables, launches on the context's stream (or `hip_stream`), waits, and frees all of them on every
 * way out.  OPUSGPU_BAD_ARG before any device work: what opusgpu_mel_layout refuses of params, a span that breaks the rules above,
 * a scale that is not finite. */
int opusgpu_tracks_mel_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in16k_mono,
                              const opusgpu_mel_params *params, void *d_out, void *hip_stream);
/* opusgpu_files_decode into features: runs opusgpu_files_decode_resampled (mix NULL, `mono` 1) or opusgpu_files_decode_mixed (`mono`
 * 0, *mix with out_channels == 1) at rate 16000 into a scratch buffer of int16 mono tracks, then k_tracks_mel from there into
 * d_out; both scratch buffers are freed on every way out.  d_out: opusgpu_mel_layout's total in floats, 128-byte aligned.  scale:
 * host array of n_files floats, or NULL for 1 / 32768 each.  feat_offsets[i] and frames_out[i] (either may be NULL): where feature
 * track i begins and its F = ceil(final / 3) / 160; track_lengths_out and status_out as for opusgpu_files_decode (the lengths at 48
 * kHz).  OPUSGPU_BAD_ARG before any device work: what opusgpu_mel_layout refuses of params, neither `mono` nor a mix or both, a mix
 * with out_channels != 1 or one that CHANNEL MIX refuses, `mono` on more than 2 channels, a scale entry that is not finite, a
 * d_out that is not 128-byte aligned.  On a failure the caller's arrays are left as they were. */
int opusgpu_files_decode_mel(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int mono, const opusgpu_mix_matrix *mix,
                             const opusgpu_mel_params *params, const float *scale, void *d_out, int64_t *feat_offsets, int64_t *frames_out,
                             int64_t *track_lengths_out, int32_t *status_out);

/* TRACK SPECTROGRAMS.  Mel spectrograms of the mono track at any rate of TRACK RATES and TRACK RATIOS, with the numbers that
 * torchaudio.transforms.MelSpectrogram and librosa.feature.melspectrogram take as FIELDS: the front ends of vocoders (22050 Hz,
 * 1024 / 256, 80 Slaney bands, ln of the magnitude), Kaldi-style filterbanks (16000 Hz, 512 / 400 / 160, HTK), audio taggers (48000 or
 * 32000 Hz, 64 HTK bands) and music models (44100 Hz, 2048 / 441), in the same call that decodes the files.  TRACK FEATURES, its
 * record, its refusals and its kernel are unchanged: this is a section of its own with a record, calls and a kernel of its own.
 * The definition is this comment.
 *   INPUT.  An int16 mono track y[m], m in [0, n), exactly as TRACK RATES, TRACK RATIOS and CHANNEL MIX define it.
 *   FRAMES.  OPUSGPU_SPEC_FRAMES_TORCH: F = n / hop + 1 (floor; F = 0 for n == 0), torch.stft(center=True).  _WHISPER: F = n / hop.
 *   WINDOW.  L = win_length (n_fft if 0), left = (n_fft - L) / 2; w[i] = 0.5 - 0.5 cos(2 pi (i - left) / L) for i in [left, left + L),
 *   else 0: the periodic Hann window that torch.stft centres in the frame.  n_fft and L are even, so w[i] = w[n_fft - i].
 *   WINDOW INDEX.  TRACK FEATURES' rule with the constants as fields: frame f, tap i in [0, n_fft) reads q = hop * f - n_fft / 2 + i,
 *   reflected ONCE: q < 0 becomes -q, q >= n becomes 2 (n - 1) - q; if q is still outside [0, n) the sample is 0.  Unlike
 *   torch.stft, which refuses n <= n_fft / 2, the value is defined for every n.
 *   SAMPLE.  x_i = (float)y[q] * scale[track], one IEEE multiply; the default scale is 1 / 32768.
 *   DFT.  Re[k] = sum_i Wc[i][k] x_i, Im[k] = sum_i Ws[i][k] x_i, k in [0, n_fft / 2]; Wc[i][k] = w[i] cos(a), Ws[i][k] = w[i] sin(a),
 *   a = 2 pi ((i k) mod n_fft) / n_fft.  S[k] = Re^2 + Im^2 (power 2) or sqrtf of it (power 1).
 *   MEL.  mel[j] = sum_k B[j][k] S[k], j in [0, n_mels).
 *   OUTPUT.  v = max(mel[j], floor); v, log10f(v) or logf(v) as `log` says, float32.
 *   FILTERBANK.  Bin k lies at k * (sample_rate / n_fft) Hz, in double.  OPUSGPU_SPEC_SLANEY: mel(f) = 3 f / 200 below 1000 Hz, else
 *   15 + ln(f / 1000) / (ln 6.4 / 27); hz(m) as TRACK FEATURES writes it.  OPUSGPU_SPEC_HTK: mel(f) = 2595 log10(1 + f / 700), hz(m) =
 *   700 (10^(m / 2595) - 1).  m0 = mel(fmin), m1 = mel(fmax); p[j] = hz(m0 + j * ((m1 - m0) / (n_mels + 1))) for j in [0, n_mels],
 *   p[n_mels + 1] = hz(m1); B[j][k] = max(0, min((fk - p[j]) / (p[j + 1] - p[j]), (p[j + 2] - fk) / (p[j + 2] - p[j + 1]))), times
 *   2 / (p[j + 2] - p[j]) for OPUSGPU_SPEC_NORM_SLANEY only.
 *   TABLES.  float32, each entry computed in double and rounded once, at first use, kept per distinct (sample_rate, n_fft, win_length,
 *   n_mels, mel_scale, norm, fmin, fmax) for the life of the process and safe to ask for from any number of threads.  A cached set
 *   holds Wc and Ws -- 2 x n_fft x (n_fft / 2 + 1) floats, 2 x 2048 x 1025 floats = 16.8 MB at the top end --, B, and the kernel's
 *   copy of the half of the basis and of B that it multiplies (half of that again at most).  With Whisper's numbers (16000, 400,
 *   0 or 400, 160, 80 or 128, Slaney, Slaney, 0, 8000) Wc, Ws and B are opusgpu_mel_basis' and opusgpu_mel_filterbank's bit for bit:
 *   one builder makes both.
 *   SUMMATION ORDER is not part of the contract, as in TRACK FEATURES (the kernel folds x_i +- x_{n_fft - i} against half the
 *   basis).  What is: the tolerance of tests/test_gpu_tracks_melspec.py (8 x the error of a float32 restatement against float64,
 *   DESIGN.md section 13f), the same bits from the same call on the same input, and one bit pattern in every cell of an all-zero
 *   track.
 *   LAYOUT.  TRACK FEATURES' grid with the new F: plane[t] = roundup64(F(ceil(planned_48k[t] * up / down))), up / down the track's
 *   rate over 48000 (1 / D for a rate of TRACK RATES); feat_offset[t] the running sum of n_mels * plane[u]; both layouts of TRACK
 *   FEATURES; padding is never written; a track cut short by a failed frame keeps its planned plane and reports its shorter F.
 *   ALGORITHM.  reserved[1] of the record selects it.  OPUSGPU_SPEC_ALGO_DENSE (0, what every record without the word is): the dense
 *   DFT above on the matrix cores (k_tracks_melspec), n_fft up to 2048 -- its table grows with n_fft^2.  OPUSGPU_SPEC_ALGO_FFT (1):
 *   S[k] comes from a fast Fourier transform of the windowed frame (k_tracks_melfft: TRACK STFT's transform, its window and twiddle
 *   tables, then S and a sparse band product in the same kernel), n_fft a power of two in [64, 8192]: 4096- and 8192-point mel
 *   spectrograms for source separation and music models, and the sizes from 64 to 2048 without the dense table.  Rules with
 *   OPUSGPU_SPEC_ALGO_FFT: n_fft a power of two in [64, 8192]; win_length even, in [16, n_fft], 0 means n_fft; hop in [1, n_fft] and
 *   nothing else (the kernel keeps no window of the tile in LDS, so 31 * hop + n_fft <= 32768 has no counterpart); every other field
 *   as above.  INPUT, FRAMES, WINDOW, WINDOW INDEX, SAMPLE, MEL, OUTPUT, FILTERBANK and LAYOUT hold word for word; DFT is the same
 *   mathematical sum with w in double; SUMMATION ORDER is still not part of the contract.  What is: the tolerance of
 *   tests/test_gpu_tracks_melfft.py (8 x the error of a float32 restatement -- a radix-2 FFT in numpy, a float32 S and band product
 *   -- against float64, per parameter set); the same bits from the same call on the same input; one bit
 *   pattern, the floor's value (its log with a log), in every cell of an all-zero track, +0.0f if the floor is 0, under a negative
 *   scale too; a frame's cells depend only on the record, the scale and the n_fft samples the frame reads, not on where the frame
 *   sits in its tile, track or batch; padding is never written, and a track without a frame writes nothing.  TABLES of an FFT
 *   record: B, [n_mels][n_fft / 2 + 1], by the builder of the dense records -- for n_fft <= 2048 the dense record's B bit for bit --,
 *   the runs of B that the kernel multiplies (per band from its first to its last non-zero float32 entry; a band without one gives
 *   max(0, floor)), and TRACK STFT's FFT TABLES for the same n_fft and win_length, from the one cache (opusgpu_spec_fft_tables hands
 *   out what opusgpu_stft_fft_tables does).  No Wc and no Ws are ever built for an FFT record.  Any other value of reserved[1] is
 *   refused, as is n_fft 4096 without the word. */
#define OPUSGPU_SPEC_ALGO_DENSE 0
#define OPUSGPU_SPEC_ALGO_FFT 1
#define OPUSGPU_SPEC_SLANEY 0
#define OPUSGPU_SPEC_HTK 1
#define OPUSGPU_SPEC_NORM_SLANEY 0
#define OPUSGPU_SPEC_NORM_NONE 1
#define OPUSGPU_SPEC_LOG_NONE 0
#define OPUSGPU_SPEC_LOG10 1
#define OPUSGPU_SPEC_LN 2
#define OPUSGPU_SPEC_FRAMES_TORCH 0
#define OPUSGPU_SPEC_FRAMES_WHISPER 1
typedef struct opusgpu_spec_params { /* 64 bytes (ABI) */
    int32_t sample_rate; /* Hz of the mono track the frames are cut from, 1 .. 1048576; places the filterbank, and the whole-file calls check it */
    int32_t n_fft;       /* a multiple of 16 in [64, 2048] */
    int32_t win_length;  /* even, in [16, n_fft]; 0 means n_fft */
    int32_t hop;         /* in [1, n_fft], and 31 * hop + n_fft <= 32768 */
    int32_t n_mels;      /* 1 .. 128 */
    int32_t mel_scale;   /* OPUSGPU_SPEC_SLANEY 0 | OPUSGPU_SPEC_HTK 1 */
    int32_t norm;        /* OPUSGPU_SPEC_NORM_SLANEY 0 | OPUSGPU_SPEC_NORM_NONE 1 */
    int32_t power;       /* 1: sqrt(Re^2 + Im^2); 2: Re^2 + Im^2 */
    int32_t log;         /* OPUSGPU_SPEC_LOG_NONE 0 | OPUSGPU_SPEC_LOG10 1 | OPUSGPU_SPEC_LN 2 */
    int32_t frames;      /* OPUSGPU_SPEC_FRAMES_TORCH 0: F = n / hop + 1 (0 for n == 0); OPUSGPU_SPEC_FRAMES_WHISPER 1: F = n / hop */
    int32_t layout;      /* OPUSGPU_MEL_BANDS_MAJOR | OPUSGPU_MEL_FRAMES_MAJOR */
    float fmin, fmax;    /* Hz, 0 <= fmin < fmax <= sample_rate / 2 */
    float floor;         /* finite, >= 0; > 0 with a log */
    int32_t reserved[2]; /* 0, but reserved[1]: the ALGORITHM, OPUSGPU_SPEC_ALGO_DENSE 0 | OPUSGPU_SPEC_ALGO_FFT 1, under which n_fft
                            is a power of two in [64, 8192] and hop is in [1, n_fft] */
} opusgpu_spec_params;
/* The DFT basis of *p: sets *wc and *ws (either may be NULL) to Wc and Ws, [n_fft][n_fft / 2 + 1] floats each, valid for the life
 * of the process, and returns n_fft * (n_fft / 2 + 1); OPUSGPU_BAD_ARG for a record that breaks a rule above, and for every
 * OPUSGPU_SPEC_ALGO_FFT record: there is no dense basis behind one.  Host only. */
int opusgpu_spec_basis(const opusgpu_spec_params *p, const float **wc, const float **ws);
/* The filterbank of *p, either algorithm, every size: sets *b (may be NULL) to B, [n_mels][n_fft / 2 + 1] floats, and returns their
 * count; OPUSGPU_BAD_ARG as above.  Host only. */
int opusgpu_spec_filterbank(const opusgpu_spec_params *p, const float **b);
/* FFT TABLES of an OPUSGPU_SPEC_ALGO_FFT record: opusgpu_stft_fft_tables' for the same n_fft and win_length, the very tables -- sets
 * *window (n_fft floats) and *twiddle (n_fft / 2 pairs of cos, sin), either may be NULL, valid for the life of the process, and
 * returns n_fft; OPUSGPU_BAD_ARG for an OPUSGPU_SPEC_ALGO_DENSE record and for a record that breaks a rule.  Host only. */
int opusgpu_spec_fft_tables(const opusgpu_spec_params *p, const float **window, const float **twiddle);
/* The frames of a tile for *p: of k_tracks_melspec the largest of 128, 64 and 32 whose window of (T - 1) hop + n_fft samples is at
 * most 32768 samples; of k_tracks_melfft (an OPUSGPU_SPEC_ALGO_FFT record) the larger of 32 and 8192 / n_fft, whatever the hop.
 * OPUSGPU_BAD_ARG for a record that breaks a rule.  Host only. */
int opusgpu_spec_tile(const opusgpu_spec_params *p);
/* LAYOUT above for n tracks of planned_48k_samples[i] samples at 48 kHz whose spectrograms are cut at up / down of that rate (1 <=
 * up <= down <= 48000; not reduced, not held against sample_rate): writes feat_offsets[i] (may be NULL) and returns the total in
 * floats.  OPUSGPU_BAD_ARG: a record that breaks a rule, such an up / down, a negative length.  Host only. */
int64_t opusgpu_spec_layout(int n, const int64_t *planned_48k_samples, int up, int down, const opusgpu_spec_params *p, int64_t *feat_offsets);
/* k_tracks_melspec alone (k_tracks_melfft for an OPUSGPU_SPEC_ALGO_FFT record): opusgpu_tracks_mel_device's contract and alignment rules -- d_in_mono packed int16 mono tracks, 16-byte
 * aligned, read in aligned 16-byte pieces up to the one that holds a track's last sample; `spans` a HOST array of opusgpu_mel_span,
 * whose plane must be a multiple of 64 and >= F; d_out floats, 128-byte aligned -- with *p in place of the constants.  sample_rate
 * places the filterbank and is held against nothing.  A track without a frame writes nothing.  Uploads the records, its tile table
 * and the kernel's tables, launches on the context's stream (or `hip_stream`), waits, and frees all of them on every way out.
 * OPUSGPU_BAD_ARG before any device work: a record that breaks a rule, a span that does, a scale that is not finite. */
int opusgpu_tracks_melspec_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in_mono,
                                  const opusgpu_spec_params *p, void *d_out, void *hip_stream);
/* opusgpu_files_decode into spectrograms.  rate != 0 (and up == down == 0): the track of TRACK RATES at that rate, 48000 included,
 * through opusgpu_files_decode_resampled (`mono` 1, mix NULL) or opusgpu_files_decode_mixed (`mono` 0, *mix of one row).  rate == 0:
 * the track of TRACK RATIOS at up / down through opusgpu_files_decode_ratio.  Either runs into a scratch buffer of int16 mono
 * tracks (its own 48 kHz scratch is freed before the kernel starts), then k_tracks_melspec from there into d_out: opusgpu_spec_layout's
 * total in floats, 128-byte aligned.  scale, feat_offsets, frames_out (F of the final length), track_lengths_out and status_out as
 * for opusgpu_files_decode_mel; they are written last.  OPUSGPU_BAD_ARG before any device work, the buffer and the caller's arrays
 * left as they were: a record that breaks a rule; a sample_rate that is not the track's rate, a ratio whose rate is no integer
 * included; neither `mono` nor a mix, or both, or a mix of more than one row; what the rate and ratio calls refuse; a scale entry
 * that is not finite; a d_out that is not 128-byte aligned. */
int opusgpu_files_decode_melspec(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int up, int down, int mono,
                                 const opusgpu_mix_matrix *mix, const opusgpu_spec_params *p, const float *scale, void *d_out,
                                 int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out);

/* TRACK KALDI FEATURES.  Kaldi's compute-fbank-feats / compute-mfcc-feats (torchaudio.compliance.kaldi.fbank and .mfcc) of the mono
 * track at any rate of TRACK RATES and TRACK RATIOS, in the same call that decodes the files: the front end of WeNet, k2 / icefall,
 * ESPnet recipes and most speaker-verification stacks.  No setting of opusgpu_spec_params is this computation -- frames that are not
 * centred, a mean and a pre-emphasis per frame, a symmetric window at the start of a zero-padded FFT, triangles that are linear in
 * mel -- so it is a section of its own with a record, calls and a kernel of its own; TRACK FEATURES and TRACK SPECTROGRAMS are
 * unchanged.  The definition is this comment.
 *   INPUT.  An int16 mono track y[m], m in [0, n), exactly as TRACK RATES, TRACK RATIOS and CHANNEL MIX define it.
 *   NOT OFFERED.  Dither (the features are a function of the track); use_energy, raw_energy and energy_floor; htk_compat; VTLN
 *   warping; subtract_mean (one torch operation on the result, or OPUSGPU_FEAT_NORM_CMN of FEATURE BATCHES below).
 *   FRAMES.  L = frame_length, H = frame_shift.  snip_edges 1: F = 0 for n < L, else 1 + (n - L) / H (floor); frame f starts at s =
 *   f H: only whole windows inside the track.  snip_edges 0: F = (n + H / 2) / H; frame f starts at s = f H + H / 2 - L / 2 (integer
 *   halves), and an index q outside [0, n) is mapped by q < 0 -> -q - 1 and q >= n -> 2 n - 1 - q, REPEATED until it lies inside:
 *   Kaldi's rule, not torch.stft's; the repeats matter for n < L.
 *   PER FRAME, with x_i = y[q(s + i)], i in [0, L), written over the reals:
 *     1. remove_dc 1: m = (sum_i x_i) / L and d_i = x_i - m.  The sum is an exact integer and the kernel takes it as one: a constant
 *        track gives d_i = 0 exactly.  remove_dc 0: d_i = x_i.
 *     2. e_0 = d_0 - c d_0 and e_i = d_i - c d_{i-1} for i >= 1, c = preemphasis: the frame's first sample is its own predecessor.
 *     3. t_i = e_i * scale[track] * w[i]; the scale rule of TRACK FORMATS, default 1 / 32768.  A scale of 1 is Kaldi's convention of
 *        samples in the int16 range.
 *     4. X[k] = sum_{i < L} t_i e^{-2 pi i k / N}, k in [0, N / 2), N = n_fft: the frame at the START of a zero-padded FFT of N
 *        points.  The Nyquist bin takes no part.
 *     5. S[k] = |X[k]|^2 (power 2) or |X[k]| (power 1).
 *   WINDOW.  Symmetric, a = 2 pi i / (L - 1):  OPUSGPU_FBANK_HANNING 0.5 - 0.5 cos a;  _POVEY that to the power 0.85;  _HAMMING
 *   0.54 - 0.46 cos a;  _BLACKMAN 0.42 - 0.5 cos a + 0.08 cos 2a;  _RECTANGULAR 1.  w[i] = w[L - 1 - i].
 *   FILTERBANK.  bw = sample_rate / N, in double.  mel(f) = 1127 ln(1 + f / 700).  high = high_freq if > 0, else sample_rate / 2 +
 *   high_freq.  m_lo = mel(low_freq), m_hi = mel(high), delta = (m_hi - m_lo) / (n_mels + 1).  Band j: left = m_lo + j delta, centre
 *   = left + delta, right = centre + delta;  B[j][k] = max(0, min((mel(k bw) - left) / (centre - left), (right - mel(k bw)) / (right
 *   - centre))) for k in [0, N / 2): triangles that are linear in MEL (torchaudio's and librosa's HTK banks are linear in Hz).  No
 *   normalisation.  A band that no bin reaches is a row of zeros, as in Kaldi.
 *   OUTPUT, fbank (n_ceps 0).  v = max(sum_k B[j][k] S[k], floor); v (OPUSGPU_FBANK_LOG_NONE) or logf(v) (OPUSGPU_FBANK_LOG_LN),
 *   float32.  Kaldi's floor is FLT_EPSILON = 1.1920929e-07.
 *   OUTPUT, MFCC (n_ceps in [1, n_mels]; log must be LN).  g_j = logf(v_j), then c_q = lift[q] * sum_j D[q][j] g_j for q in [0,
 *   n_ceps):  D[0][j] = sqrt(1 / n_mels), D[q][j] = sqrt(2 / n_mels) cos(pi q (j + 0.5) / n_mels);  lift[q] = 1 + 0.5 Q sin(pi q /
 *   Q), Q = cepstral_lifter (Kaldi's is 22), lift = 1 for Q = 0.  The feature width is n_ceps when it is > 0, else n_mels.
 *   TABLES.  float32, each entry computed in double and rounded once, at first use, kept per distinct (sample_rate, frame_length,
 *   n_fft, n_mels, n_ceps, window, low_freq, high_freq, cepstral_lifter) for the life of the process and safe to ask for from any
 *   number of threads: w[L] (opusgpu_fbank_window), B[n_mels][N / 2] (opusgpu_fbank_filterbank), lift[q] D[q][j] as [n_ceps][n_mels]
 *   (opusgpu_fbank_dct).  The basis that the kernel multiplies is its own business.
 *   PRECISION and SUMMATION ORDER are not part of the contract, as in TRACK SPECTROGRAMS (the kernel turns the spectrum by e^{i pi k
 *   (L - 1) / N}, which changes no magnitude, and folds t_i +- t_{L - 1 - i} against half a basis that carries w).  What is: the
 *   tolerance of tests/test_gpu_tracks_fbank.py (8 x the error of a float32 restatement against float64), the
 *   same bits from the same call on the same input -- no float atomics --, one bit pattern in every cell of an all-zero track, and
 *   with remove_dc one bit pattern in every cell of any constant track: the floor's value (for MFCC one pattern per coefficient q,
 *   the DCT of a row of logf(floor)).
 *   LAYOUT.  TRACK FEATURES' grid with this F and the feature width: plane[t] = roundup64(F(ceil(planned_48k[t] * up / down)));
 *   feat_offset[t] the running sum of width * plane[u]; both layouts of TRACK FEATURES; padding is never written; a track cut short
 *   by a failed frame keeps its planned plane and reports its shorter F. */
#define OPUSGPU_FBANK_POVEY 0
#define OPUSGPU_FBANK_HANNING 1
#define OPUSGPU_FBANK_HAMMING 2
#define OPUSGPU_FBANK_RECTANGULAR 3
#define OPUSGPU_FBANK_BLACKMAN 4
#define OPUSGPU_FBANK_LOG_NONE 0
#define OPUSGPU_FBANK_LOG_LN 1
typedef struct opusgpu_fbank_params { /* 64 bytes (ABI) */
    int32_t sample_rate;  /* Hz of the mono track, 1 .. 1048576; places the filterbank, and the whole-file calls check it */
    int32_t frame_length; /* L, samples, 2 .. 2048 (odd allowed) */
    int32_t frame_shift;  /* H, samples, >= 1, and 31 * frame_shift + frame_length <= 32768 (32 frames' window in the kernel's LDS) */
    int32_t n_fft;        /* N: a multiple of 16 in [64, 2048], >= L; 0 means the smallest power of two >= max(L, 64) */
    int32_t n_mels;       /* 3 .. 128 */
    int32_t n_ceps;       /* 0: fbank; 1 .. n_mels: MFCC with that many coefficients */
    int32_t window;       /* OPUSGPU_FBANK_POVEY 0 | _HANNING 1 | _HAMMING 2 | _RECTANGULAR 3 | _BLACKMAN 4 */
    uint8_t snip_edges;   /* 0 or 1 */
    uint8_t remove_dc;    /* 0 or 1 */
    uint8_t power;        /* 1: |X|; 2: |X|^2 */
    uint8_t log;          /* OPUSGPU_FBANK_LOG_NONE 0 | OPUSGPU_FBANK_LOG_LN 1; MFCC requires LN */
    int32_t layout;       /* OPUSGPU_MEL_BANDS_MAJOR | OPUSGPU_MEL_FRAMES_MAJOR */
    float preemphasis;    /* c, in [0, 1] */
    float low_freq;       /* Hz */
    float high_freq;      /* Hz; <= 0 means sample_rate / 2 + high_freq; 0 <= low_freq < high <= sample_rate / 2 after that */
    float floor;          /* finite, >= 0; > 0 with a log */
    float cepstral_lifter; /* Q, finite, >= 0; read for MFCC only */
    int32_t reserved[2];  /* 0 */
} opusgpu_fbank_params;
/* The window of *p: sets *w (may be NULL) to w, L floats, valid for the life of the process, and returns L; OPUSGPU_BAD_ARG for a
 * record that breaks a rule above.  Host only. */
int opusgpu_fbank_window(const opusgpu_fbank_params *p, const float **w);
/* The filterbank of *p: sets *b (may be NULL) to B, [n_mels][N / 2] floats, and returns their count; OPUSGPU_BAD_ARG as above.
 * Host only. */
int opusgpu_fbank_filterbank(const opusgpu_fbank_params *p, const float **b);
/* The lifted DCT of *p: sets *d (may be NULL) to lift[q] D[q][j], [n_ceps][n_mels] floats, and returns their count (0, and *d NULL,
 * for n_ceps 0); OPUSGPU_BAD_ARG as above.  Host only. */
int opusgpu_fbank_dct(const opusgpu_fbank_params *p, const float **d);
/* LAYOUT above for n tracks of planned_48k_samples[i] samples at 48 kHz whose features are cut at up / down of that rate (1 <= up
 * <= down <= 48000; not reduced, not held against sample_rate): writes feat_offsets[i] (may be NULL) and returns the total in
 * floats.  OPUSGPU_BAD_ARG: a record that breaks a rule, such an up / down, a negative length.  Host only. */
int64_t opusgpu_fbank_layout(int n, const int64_t *planned_48k_samples, int up, int down, const opusgpu_fbank_params *p, int64_t *feat_offsets);
/* k_tracks_fbank alone: opusgpu_tracks_melspec_device's contract and alignment rules -- d_in_mono packed int16 mono tracks, 16-byte
 * aligned, read in aligned 16-byte pieces up to the one that holds a track's last sample; `spans` a HOST array of opusgpu_mel_span,
 * whose plane must be a multiple of 64 and >= F; d_out floats, 128-byte aligned -- with this section's record, F and feature width.
 * sample_rate places the filterbank and is held against nothing.  A track without a frame writes nothing.  OPUSGPU_BAD_ARG before
 * any device work: a record that breaks a rule, a span that does, a scale that is not finite. */
int opusgpu_tracks_fbank_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in_mono,
                                const opusgpu_fbank_params *p, void *d_out, void *hip_stream);
/* opusgpu_files_decode into Kaldi features: opusgpu_files_decode_melspec's flow, arguments, "written last" and refusals with this
 * section's record, kernel and layout: rate != 0 names a rate of TRACK RATES, rate == 0 the ratio up / down of TRACK RATIOS;
 * `mono` 1 or a *mix of one row; d_out opusgpu_fbank_layout's total in floats, 128-byte aligned; frames_out is F of the final
 * length.  OPUSGPU_BAD_ARG before any device work, the buffer and the caller's arrays left as they were: a record that breaks a
 * rule; a sample_rate that is not the track's rate; whatever opusgpu_files_decode_melspec refuses of the other arguments. */
int opusgpu_files_decode_fbank(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int up, int down, int mono,
                               const opusgpu_mix_matrix *mix, const opusgpu_fbank_params *p, const float *scale, void *d_out,
                               int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out);

/* TRACK STFT.  The spectrogram itself: all n_fft / 2 + 1 linear bins of the short-time Fourier transform of the mono track at any
 * rate of TRACK RATES and TRACK RATIOS, as magnitude, power or complex numbers -- what torchaudio.transforms.Spectrogram and
 * torch.stft(center=True, pad_mode="reflect", window=hann_window(win_length), return_complex=True) give -- in the same call that
 * decodes the files: the input of VITS-style TTS (22050 Hz, 1024 / 256, magnitude), of speech enhancement and separation (16000 Hz,
 * 512 / 400 / 128, complex), of music models (44100 Hz, 2048 points) and of any filterbank of the caller's own.  No setting of
 * opusgpu_spec_params is this computation (n_mels is 1 .. 128 there and the band product always runs), so it is a section of its
 * own with a record, calls and a kernel of its own; TRACK FEATURES, TRACK SPECTROGRAMS and TRACK KALDI FEATURES, their records,
 * grids, refusals and kernels are unchanged.  The definition is this comment.
 *   INPUT.  An int16 mono track y[m], m in [0, n), exactly as TRACK RATES, TRACK RATIOS and CHANNEL MIX define it.
 *   FRAMES.  OPUSGPU_SPEC_FRAMES_TORCH: F = n / hop + 1 (floor; F = 0 for n == 0), torch.stft(center=True).  _WHISPER: F = n / hop.
 *   WINDOW.  L = win_length (n_fft if 0), left = (n_fft - L) / 2; w[i] = 0.5 - 0.5 cos(2 pi (i - left) / L) for i in [left, left + L),
 *   else 0: the periodic Hann window that torch.stft centres in the frame.  n_fft and L are even, so w[i] = w[n_fft - i].
 *   WINDOW INDEX.  Frame f, tap i in [0, n_fft) reads q = hop * f - n_fft / 2 + i, reflected ONCE: q < 0 becomes -q, q >= n becomes
 *   2 (n - 1) - q; if q is still outside [0, n) the sample is 0.  Unlike torch.stft, which refuses n <= n_fft / 2, the value is
 *   defined for every n.
 *   SAMPLE.  x_i = (float)y[q] * scale[track], one IEEE multiply; the default scale is 1 / 32768.
 *   DFT.  Re[k] = sum_i Wc[i][k] x_i, Im[k] = -sum_i Ws[i][k] x_i, k in [0, n_fft / 2]; Wc[i][k] = w[i] cos(a), Ws[i][k] = w[i] sin(a),
 *   a = 2 pi ((i k) mod n_fft) / n_fft.  Wc and Ws are TRACK SPECTROGRAMS' tables, made by the one builder: what opusgpu_stft_basis
 *   hands out is what opusgpu_spec_basis hands out for the same n_fft and win_length, bit for bit.  SIGN: Ws as both accessors hand
 *   it out is +w sin(a), the OPPOSITE of torch.stft's imaginary part (e^{-ia} = cos a - i sin a), which the mel path never sees
 *   because it squares; Im here carries torch.stft's sign, hence the minus above.
 *   OUTPUT, for every k in [0, n_fft / 2].  OPUSGPU_STFT_COMPLEX (power 0): the pair (Re[k], Im[k]) as two adjacent floats, torch's
 *   view_as_real order; floor is not applied.  power 2: S = Re^2 + Im^2; power 1: S = sqrtf(Re^2 + Im^2); v = max(S, floor); then v,
 *   log10f(v) or logf(v) as `log` says, float32.  A log is refused with OPUSGPU_STFT_COMPLEX.
 *   TABLES.  float32, each entry computed in double and rounded once, at first use, kept per distinct (n_fft, win_length) for the
 *   life of the process and safe to ask for from any number of threads: Wc, Ws (2 x n_fft x (n_fft / 2 + 1) floats) and the kernel's
 *   copy of the half it multiplies.
 *   SUMMATION ORDER is not part of the contract (the kernel folds x_i +- x_{n_fft - i} against half the basis).  What is: the
 *   tolerance of tests/test_gpu_tracks_stft.py (8 x the error of a float32 restatement against float64), the
 *   same bits from the same call on the same input, and one bit pattern in every cell of an all-zero track: the floor's value (its
 *   log with a log), and +0.0f in both halves of every pair for OPUSGPU_STFT_COMPLEX -- never -0.0f, whatever the scale's sign.
 *   LAYOUT.  TRACK FEATURES' grid at width bins * c, bins = n_fft / 2 + 1, c = 2 for OPUSGPU_STFT_COMPLEX, else 1: plane[t] =
 *   roundup64(F(ceil(planned_48k[t] * up / down))) frames; feat_offset[t] the running sum of bins * c * plane[u], a multiple of 64
 *   floats.  OPUSGPU_MEL_BANDS_MAJOR (bins-major): cell (k, f) at feat_offset + (k * plane + f) * c.  OPUSGPU_MEL_FRAMES_MAJOR: at
 *   feat_offset + (f * bins + k) * c.  Padding is never written; a track cut short by a failed frame keeps its planned plane and
 *   reports its shorter F.
 *   ALGORITHM.  reserved[1] of the record selects it.  OPUSGPU_STFT_ALGO_DENSE (0, what every record without the word is): the dense
 *   DFT above on the matrix cores (k_tracks_stft), n_fft up to 2048 -- its table grows with n_fft^2.  OPUSGPU_STFT_ALGO_FFT (1): a
 *   fast Fourier transform (k_tracks_fft), n_fft a power of two in [64, 8192]: 4096- and 8192-point spectrograms for source
 *   separation and music models, and the sizes from 64 to 2048 for comparison.  Rules with OPUSGPU_STFT_ALGO_FFT: n_fft a power of
 *   two in [64, 8192]; win_length even, in [16, n_fft], 0 means n_fft; hop in [1, n_fft] and nothing else (the kernel keeps no window
 *   of the tile in LDS and forms hop * frame in 64 bits, so the dense kernel's 31 * hop + n_fft <= 32768 has no counterpart); power,
 *   log, frames, layout, floor and sample_rate as above.  INPUT, FRAMES, WINDOW, WINDOW INDEX, SAMPLE, OUTPUT and LAYOUT hold word
 *   for word (bins up to 4097); DFT is the same mathematical sum with w in double, Im with torch.stft's sign; SUMMATION ORDER is
 *   outside the contract here too; the same call on the same input gives the same bits; an all-zero track is one bit pattern, the
 *   floor's value or +0.0f in both halves of a pair.  FFT TABLES: the kernel multiplies a window, window[i] = (float)w[i], n_fft
 *   floats, and one twiddle table, twiddle[2j], twiddle[2j + 1] = (float)cos(2 pi j / n_fft), (float)sin(2 pi j / n_fft) for j in
 *   [0, n_fft / 2) -- no sine or cosine is computed on the device --, each entry computed in double and rounded once, at first use,
 *   kept per (n_fft, win_length) for the life of the process, safe from any number of threads (opusgpu_stft_fft_tables).  The
 *   tolerance is that of tests/test_gpu_tracks_fft.py: 8 x the error of a float32 radix-2 FFT in numpy against float64 (DESIGN.md
 *   section 13p).  Any other value of reserved[1] is refused, as is n_fft 4096 without the word. */
#define OPUSGPU_STFT_COMPLEX 0
#define OPUSGPU_STFT_ALGO_DENSE 0
#define OPUSGPU_STFT_ALGO_FFT 1
typedef struct opusgpu_stft_params { /* 64 bytes (ABI) */
    int32_t sample_rate; /* Hz of the mono track the frames are cut from, 1 .. 1048576; the whole-file calls check it */
    int32_t n_fft;       /* a multiple of 16 in [64, 2048] */
    int32_t win_length;  /* even, in [16, n_fft]; 0 means n_fft */
    int32_t hop;         /* in [1, n_fft], and 31 * hop + n_fft <= 32768 */
    int32_t power;       /* OPUSGPU_STFT_COMPLEX 0: (Re, Im) pairs; 1: sqrt(Re^2 + Im^2); 2: Re^2 + Im^2 */
    int32_t log;         /* OPUSGPU_SPEC_LOG_NONE 0 | OPUSGPU_SPEC_LOG10 1 | OPUSGPU_SPEC_LN 2; OPUSGPU_SPEC_LOG_NONE with power 0 */
    int32_t frames;      /* OPUSGPU_SPEC_FRAMES_TORCH 0: F = n / hop + 1 (0 for n == 0); OPUSGPU_SPEC_FRAMES_WHISPER 1: F = n / hop */
    int32_t layout;      /* OPUSGPU_MEL_BANDS_MAJOR (bins-major) | OPUSGPU_MEL_FRAMES_MAJOR */
    float floor;         /* finite, >= 0; > 0 with a log; not applied to pairs */
    int32_t reserved[7]; /* 0, but reserved[1]: the ALGORITHM, OPUSGPU_STFT_ALGO_DENSE 0 | OPUSGPU_STFT_ALGO_FFT 1, under which n_fft
                            is a power of two in [64, 8192] and hop is in [1, n_fft] */
} opusgpu_stft_params;
/* The DFT basis of *p: sets *wc and *ws (either may be NULL) to Wc and Ws, [n_fft][n_fft / 2 + 1] floats each, valid for the life
 * of the process, and returns n_fft * (n_fft / 2 + 1); OPUSGPU_BAD_ARG for a record that breaks a rule above.  The same tables for
 * either algorithm; OPUSGPU_BAD_ARG for n_fft above 2048, where the two tables would hold 2 x n_fft x (n_fft / 2 + 1) floats (268 MB
 * at 8192) that no kernel multiplies: FFT records have opusgpu_stft_fft_tables.  Host only. */
int opusgpu_stft_basis(const opusgpu_stft_params *p, const float **wc, const float **ws);
/* FFT TABLES of an OPUSGPU_STFT_ALGO_FFT record: sets *window (n_fft floats) and *twiddle (n_fft / 2 pairs of cos, sin), either may
 * be NULL, valid for the life of the process, and returns n_fft; OPUSGPU_BAD_ARG for an OPUSGPU_STFT_ALGO_DENSE record and for a
 * record that breaks a rule.  Host only. */
int opusgpu_stft_fft_tables(const opusgpu_stft_params *p, const float **window, const float **twiddle);
/* The frames of a tile of k_tracks_stft for *p: the largest of 128, 64 and 32 whose window of (T - 1) hop + n_fft samples is at most
 * 32768 samples (65,536 bytes of LDS), TRACK SPECTROGRAMS' rule: the kernel stores from its accumulators and needs no store area.
 * For an OPUSGPU_STFT_ALGO_FFT record, the frames of a tile of k_tracks_fft: the larger of 16 and 8192 / n_fft, whatever the hop --
 * 256 / min(256, n_fft / 8) frames are in flight in a workgroup, and a tile is four rounds of them up to n_fft 256, 16 frames from
 * 512 up.  OPUSGPU_BAD_ARG for a record that breaks a rule.  Host only. */
int opusgpu_stft_tile(const opusgpu_stft_params *p);
/* LAYOUT above for n tracks of planned_48k_samples[i] samples at 48 kHz whose frames are cut at up / down of that rate (1 <= up <=
 * down <= 48000; not reduced, not held against sample_rate): writes feat_offsets[i] (may be NULL) and returns the total in floats.
 * OPUSGPU_BAD_ARG: a record that breaks a rule, such an up / down, a negative length.  Host only. */
int64_t opusgpu_stft_layout(int n, const int64_t *planned_48k_samples, int up, int down, const opusgpu_stft_params *p, int64_t *feat_offsets);
/* k_tracks_stft alone (k_tracks_fft for an OPUSGPU_STFT_ALGO_FFT record): opusgpu_tracks_melspec_device's contract and alignment rules -- d_in_mono packed int16 mono tracks, 16-byte
 * aligned, read in aligned 16-byte pieces up to the one that holds a track's last sample; `spans` a HOST array of opusgpu_mel_span,
 * whose plane must be a multiple of 64 and >= F; d_out floats, 128-byte aligned -- with this section's record and width.
 * sample_rate is held against nothing.  A track without a frame writes nothing.  Uploads the records, its tile table and the
 * kernel's table, launches on the context's stream (or `hip_stream`), waits, and frees all of them on every way out.
 * OPUSGPU_BAD_ARG before any device work: a record that breaks a rule, a span that does, a scale that is not finite. */
int opusgpu_tracks_stft_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_mel_span *spans, const void *d_in_mono,
                               const opusgpu_stft_params *p, void *d_out, void *hip_stream);
/* opusgpu_files_decode into linear or complex spectrograms: opusgpu_files_decode_melspec's flow, arguments, "written last" and
 * refusals with this section's record, kernel and layout: rate != 0 names a rate of TRACK RATES, rate == 0 the ratio up / down of
 * TRACK RATIOS; `mono` 1 or a *mix of one row; d_out opusgpu_stft_layout's total in floats, 128-byte aligned; frames_out is F of
 * the final length.  OPUSGPU_BAD_ARG before any device work, the buffer and the caller's arrays left as they were: a record that
 * breaks a rule; a sample_rate that is not the track's rate; whatever opusgpu_files_decode_melspec refuses of the other arguments;
 * a feature-batch request on the context (FEATURE BATCHES hold widths of 1 - 128).  With a request of STFT BATCHES (below) on the
 * context, d_out is that section's dense tensor and feat_offsets reports its offsets. */
int opusgpu_files_decode_stft(opusgpu_ctx *ctx, const opusgpu_file_batch *batch, int rate, int up, int down, int mono,
                              const opusgpu_mix_matrix *mix, const opusgpu_stft_params *p, const float *scale, void *d_out,
                              int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out);

/* TRACK LOUDNESS. Integrated loudness per ITU-R BS.1770-4 and the sample peak of every track, measured on the GPU, and optionally
 * a gain to a target loudness folded into the float scale of the same call.  All of it is a function of the S16 track at 48 kHz:
 * the int16 samples s_c[n] the default path writes, at the track's FINAL length len.  Samples at or past len are never read as
 * signal.
 *   K-WEIGHTING.  The two 48 kHz biquads of BS.1770-4 with the standard's own numbers, y[n] = b0 x[n] + b1 x[n-1] + b2 x[n-2]
 *   - a1 y[n-1] - a2 y[n-2]:  stage 1  b = {1.53512485958697, -2.69169618940638, 1.19839281085285}, a = {1, -1.69065929318241,
 *   0.73248077421585};  stage 2  b = {1, -2, 1}, a = {1, -1.99004745483398, 0.99007225036621}.  The input is x_c[n] = s_c[n] / 32768,
 *   the state is zero at the track's first sample, the output is z_c.
 *   SEGMENTS AND BLOCKS.  Segment j of channel c has the energy e_c[j] = sum z_c[n]^2 over n in [4800 j, 4800 j + 4800); only whole
 *   segments count, floor(len / 4800) of them.  Block j covers segments j .. j + 3 (400 ms, 75 % overlap):
 *       p[j] = sum_c G_c (e_c[j] + e_c[j+1] + e_c[j+2] + e_c[j+3]) / 19200,         blocks = max(0, floor(len / 4800) - 3).
 *   GATING.  The blocks with -0.691 + 10 log10 p[j] > -70 pass the absolute gate; those among them with p[j] > 0.1 x the mean of
 *   the blocks that passed the absolute gate pass the relative gate (10 LU below that mean);  lufs = -0.691 + 10 log10(mean of
 *   the blocks that passed the relative gate), `gated` their count.  If no block passes, lufs = -inf and gated = 0.
 *   CHANNEL WEIGHTS.  G_c defaults by channel count in the Vorbis order of CHANNEL MIX, by BS.1770-4's azimuth rule at the nominal
 *   positions (between 60 and 120 degrees: 1.41; the LFE: 0; else 1):  1: {1};  2: {1, 1};  3: {1, 1, 1};  4: {1, 1, 1.41, 1.41};
 *   5: {1, 1, 1, 1.41, 1.41};  6: {1, 1, 1, 1.41, 1.41, 0};  7: {1, 1, 1, 1.41, 1.41, 1, 0};  8: {1, 1, 1, 1.41, 1.41, 1, 1, 0}.  A
 *   caller may pass weights of their own: finite and >= 0.
 *   PEAK.  max |s_c[n]| / 32768 over all channels, the LFE included, and over all len samples.  It is exact.
 *   GAIN.  A pure function of the record, on the host in double:  g = 10^((target - lufs) / 20);  if peak_limit > 0 and peak * g >
 *   peak_limit, g = peak_limit / peak;  if lufs is -inf, g = 1.  The scale a normalising call applies to track t is
 *   (float)((double)scale[t] * g), and every float sample is then (float)s * that, as TRACK FORMATS says: normalised tracks stay a
 *   bit-for-bit function of the int16 tracks and the record.
 *   PRECISION.  The kernels filter and sum the segment energies in float32 (every operation rounded on its own, nothing fused; a
 *   segment's starting state comes from one segment of warm-up, which leaves out 0.99502^4800 = 4e-11 of it) and gate in double;
 *   the result is the same bits from run to run, and a track's record does not depend on which other tracks are in the call.
 *   Against the definition in double lufs differs by rounding alone (DESIGN 13h has the measured bound); peak, blocks and gated
 *   do not differ unless a block lies within that rounding of a gate. */
typedef struct opusgpu_loudness_span { /* 16 bytes, one per track (ABI) */
    int64_t in_offset;  /* where the S16 track begins in d_in, samples per channel; a multiple of 8 */
    int64_t in_samples; /* its FINAL length */
} opusgpu_loudness_span;
typedef struct opusgpu_loudness { /* 16 bytes, one per track (ABI) */
    float lufs;     /* integrated loudness, -inf when no block passes */
    float peak;     /* sample peak, 0 .. 1 */
    int32_t blocks; /* 400 ms blocks of the track */
    int32_t gated;  /* of which passed both gates */
} opusgpu_loudness;
/* The default weights of `channels` (1 - 8) channels into weights[0 .. channels); anything else is OPUSGPU_BAD_ARG.  Host only. */
int opusgpu_loudness_weights(int channels, float *weights);
/* GAIN above for the record *r (NULL: 1).  Host only. */
double opusgpu_loudness_gain(const opusgpu_loudness *r, double target_lufs, double peak_limit);
/* k_tracks_loudness_seg and k_tracks_loudness_gate alone: d_in holds packed interleaved int16 tracks of `channels` (1 - 8) channels,
 * 16-byte aligned, read in aligned 16-byte pieces up to the one that holds a track's last sample; `spans` is a HOST array of
 * n_tracks records, `weights` a host array of `channels` floats or NULL for the defaults, `out` a HOST array of n_tracks records.
 * Uploads the spans and its tile table, launches on the context's stream (or `hip_stream`), waits, brings 16 bytes per track back
 * and frees everything on every way out; `out` is written only on success.  OPUSGPU_BAD_ARG before any device work: channels
 * outside 1 - 8, a span that breaks the rules above, a weight that is negative or not finite. */
int opusgpu_tracks_loudness_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_loudness_span *spans, const void *d_in, int channels,
                                   const float *weights /* NULL: defaults */, opusgpu_loudness *out, void *hip_stream);
#define OPUSGPU_LOUDNESS_OFF 0
#define OPUSGPU_LOUDNESS_MEASURE 1   /* records only: every result is what it is without the request */
#define OPUSGPU_LOUDNESS_NORMALIZE 2 /* and GAIN folded into the float scale */
typedef struct opusgpu_loudness_req { /* 48 bytes (ABI) */
    int32_t mode;
    float target_lufs; /* OPUSGPU_LOUDNESS_NORMALIZE: the target, e.g. -23 (EBU R 128) */
    float peak_limit;  /* OPUSGPU_LOUDNESS_NORMALIZE: see GAIN; <= 0: none */
    int32_t n_weights; /* 0: the defaults of the tracks' channel count; else it must be that count */
    float weights[8];
} opusgpu_loudness_req;
/* The request that holds for the whole-file calls that follow, as opusgpu_set_mode does; NULL or mode 0 is off, the default, and
 * every call is then exactly what it is above.  OPUSGPU_BAD_ARG: an unknown mode, n_weights outside 0 - 8, a weight that is negative
 * or not finite, a target or limit that is not finite.  With a request on:
 *   every whole-file call that holds scratch S16 tracks -- _resampled, _mixed, _ratio, _mel and _melspec, of both kinds of context --
 *   measures them between its decode and its own kernel, at their final lengths (a failed track too), on all decoded channels, in
 *   front of the mix and the rate; with OPUSGPU_LOUDNESS_NORMALIZE the gain goes into the scale its kernel applies;
 *   opusgpu_files_decode and opusgpu_ms_files_decode (and the _as calls with OPUSGPU_TRACKS_S16) measure the int16 tracks in the
 *   caller's buffer after the last step;
 *   OPUSGPU_LOUDNESS_NORMALIZE with an int16 result is OPUSGPU_BAD_ARG before any device work, as a scale with S16 is, and so is a
 *   request whose n_weights is neither 0 nor the batch's channel count;
 *   opusgpu_files_decode_as and opusgpu_ms_files_decode_as with a float format fuse the float store into the assembly and never
 *   have an S16 track: they return OPUSGPU_BAD_ARG, and the message names the way round -- the _mixed call at rate 48000 with
 *   the identity matrix (16384 on the diagonal), which is exact (sat16((16384 s + 8192) >> 14) = s) and writes the same elements. */
int opusgpu_set_loudness(opusgpu_ctx *ctx, const opusgpu_loudness_req *req);
/* What the last whole-file call with a request on measured and applied: returns the number of its tracks (0: none yet) and writes
 * the first min(n, that) records and gains (either may be NULL; a gain is 1 when the request only measured). */
int opusgpu_last_loudness(const opusgpu_ctx *ctx, int n, opusgpu_loudness *records, double *gains);
int opusgpu_ms_set_loudness(opusgpu_ms *ms, const opusgpu_loudness_req *req);
int opusgpu_ms_last_loudness(const opusgpu_ms *ms, int n, opusgpu_loudness *records, double *gains);

/* FEATURE BATCHES.  The features of a call as ONE dense tensor, padded to a common length and normalised per track, behind the
 * feature kernels of TRACK FEATURES, TRACK SPECTROGRAMS and TRACK KALDI FEATURES: what a model takes -- a [B, 80, 3000] Whisper
 * input, a [B, T, 80] fbank batch with per-utterance CMVN -- without a loop over tracks in the caller's code.  Those three sections
 * and their kernels are unchanged; this stage reads their packed grid and writes a second buffer.  The definition is this comment.
 *   INPUT.  A packed feature grid exactly as those sections lay it out: feat_offset[t] and plane[t] multiples of 64 floats, width
 *   W in [1, 128] (n_mels, or n_ceps for MFCC), OPUSGPU_MEL_BANDS_MAJOR (cell (j, f) at feat_offset[t] + j * plane[t] + f) or
 *   OPUSGPU_MEL_FRAMES_MAJOR (feat_offset[t] + f * W + j).  F[t] is the frame count of the track's FINAL length: cells f >= F[t] of
 *   the grid are never interpreted.  The real cells are finite; the caller of the stand-alone call guarantees it (a feature kernel
 *   with a log and a floor > 0 writes nothing else).
 *   OUTPUT.  A dense float32 tensor of n_tracks * S * W floats, S = stride_frames, in the grid's own layout.  Bands-major: cell
 *   (t, j, f) at (t * W + j) * S + f -- [n, W, S].  Frames-major: cell (t, f, j) at (t * S + f) * W + j -- [n, S, W].  EVERY element
 *   is written exactly once, the pad cells f >= F[t] included; nothing outside the tensor is touched.  S is any integer >= 1 that
 *   holds every track's frames, with S * W <= 0x7fffffff: 3000 is not a multiple of 64, and nothing is asked of S's alignment.
 *   STATISTICS are per track, over its F[t] real cells only: they never depend on pad cells, on the grid's padding or on which
 *   other tracks are in the call.
 *   NORMALISATIONS (norm), x a real cell of bin j:
 *     OPUSGPU_FEAT_NORM_NONE     y = x.
 *     OPUSGPU_FEAT_NORM_WHISPER  m = the max over ALL real cells of the track (every bin); y = (fmaxf(x, m - range) + add) * mul:
 *       one float32 subtraction for m - range, then three float32 operations, each rounded on its own, nothing fused.  Whisper's
 *       numbers are range 8, add 4, mul 0.25.  F = 0 gives m = -inf.
 *     OPUSGPU_FEAT_NORM_CMN      mean_j = (sum_f (double)x[f][j]) / F;  y = (float)((double)x - mean_j).  Kaldi's subtract_mean, and
 *       apply-cmvn --norm-vars=false per utterance.
 *     OPUSGPU_FEAT_NORM_CMVN     and var_j = (sum_f (double)x[f][j]^2) / F - mean_j^2, the population variance in double in one
 *       pass;  y = (float)(((double)x - mean_j) / sqrt(max(var_j, var_floor))), var_floor finite and > 0.
 *       F = 0 gives mean 0 and var 0 under both.
 *     OPUSGPU_FEAT_NORM_AFFINE   y = (x - sub[j]) * mul[j] in float32, two rounded operations; sub and mul are host arrays of W
 *       finite floats given with the request and copied: global CMVN, the dataset's statistics per bin.
 *   PAD CELLS (pad_mode).  OPUSGPU_FEAT_PAD_VALUE: pad_value verbatim.  OPUSGPU_FEAT_PAD_NORMALIZED: the track's normalisation
 *   applied to pad_value as if it were a cell of that track and bin; it takes no part in the statistics.  Whisper pads with zero
 *   audio, whose cells are log10(1e-10) = -10 before the clamp: that is pad_value -10 with OPUSGPU_FEAT_PAD_NORMALIZED.  What this
 *   does NOT reproduce of Whisper's pad_or_trim: there the last real frames' windows reach into the zeros, here they see the
 *   track's own reflection, as TRACK FEATURES defines them.
 *   CONTRACT.  The same bits from the same call on the same input: no float atomics, and a summation order that depends only on the
 *   track's own F, W and layout -- segments of 1024 frames, each summed in a fixed order, folded in ascending order.  NONE, WHISPER
 *   and AFFINE are bit-for-bit functions of the grid.  The sums are kept in double, so a track whose real cells all hold one value
 *   c gives exactly 0.0f in every real cell under CMN and CMVN (F * c and its division by F are exact in double for F < 2^29, which
 *   is also the most frames a track may have here).  Against the definition in exact arithmetic a CMN / CMVN cell differs by at most
 *   2^-23 |y| + 2^-30 max_f |x[f][j]| / d, d = 1 or sqrt(max(var_j, var_floor)) (tests/test_gpu_feat_batch.py). */
#define OPUSGPU_FEAT_NORM_NONE 0
#define OPUSGPU_FEAT_NORM_WHISPER 1
#define OPUSGPU_FEAT_NORM_CMN 2
#define OPUSGPU_FEAT_NORM_CMVN 3
#define OPUSGPU_FEAT_NORM_AFFINE 4
#define OPUSGPU_FEAT_PAD_VALUE 0
#define OPUSGPU_FEAT_PAD_NORMALIZED 1
#define OPUSGPU_FEAT_SEG 1024 /* frames per segment of the statistics: part of the summation order */
typedef struct opusgpu_feat_batch_req { /* 64 bytes (ABI) */
    int64_t stride_frames; /* S, >= 1 */
    double var_floor;      /* CMVN: finite and > 0 (Kaldi floors at 1e-20) */
    int32_t enabled;       /* opusgpu_set_feature_batch: 0 is off; the stand-alone call does not read it */
    int32_t norm;          /* OPUSGPU_FEAT_NORM_* */
    int32_t pad_mode;      /* OPUSGPU_FEAT_PAD_* */
    float pad_value;
    float range, add, mul; /* WHISPER: 8, 4, 0.25 */
    int32_t reserved[5];   /* 0 */
} opusgpu_feat_batch_req;
typedef struct opusgpu_feat_span { /* 24 bytes, one per track (ABI) */
    int64_t grid_offset; /* feat_offset[t], in floats; a multiple of 64 */
    int64_t plane;       /* plane[t]: a multiple of 64 and >= frames */
    int64_t frames;      /* F[t], 0 <= F <= S and F < 2^29 */
} opusgpu_feat_span;
/* The request that holds for the whole-file FEATURE calls that follow, as opusgpu_set_loudness does for its own; NULL or `enabled`
 * 0 is off, the default, and every call is then byte for byte what it is above.  sub and mul_vec: host arrays of `width` floats for
 * OPUSGPU_FEAT_NORM_AFFINE, copied; not read otherwise.  OPUSGPU_BAD_ARG, the request in force left as it was: an unknown norm or
 * pad mode; a field that is not finite (pad_value, range, add, mul, var_floor); var_floor <= 0; stride_frames < 1; AFFINE without
 * both arrays, with a width outside 1 - 128 or with an entry that is not finite; a reserved word that is not 0.  With a request on,
 * opusgpu_files_decode_mel, _melspec and _fbank and their opusgpu_ms_ twins run as above into a scratch grid of their own layout
 * call, then this stage writes d_out, which is now opusgpu_feat_batch_layout's total in floats, 128-byte aligned; feat_offsets[t]
 * reports t * S * W; frames_out, track_lengths_out and status_out are what they were; the scratch is freed on every way out and
 * the caller's arrays are written last.  OPUSGPU_BAD_ARG before any device work, the buffer and the arrays left as they were, with
 * the reason in opusgpu_last_error: S below the frames of a track's PLANNED length; S * W above 0x7fffffff; AFFINE whose width is
 * not the features' W.  A loudness request composes untouched: its gain is in the feature kernel's scale.  Whole-file calls
 * without features ignore the request. */
int opusgpu_set_feature_batch(opusgpu_ctx *ctx, const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, int width);
int opusgpu_ms_set_feature_batch(opusgpu_ms *ms, const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, int width);
/* OUTPUT above for n tracks: writes feat_offsets[t] = t * S * W (may be NULL) and returns the total n * S * W in floats.
 * OPUSGPU_BAD_ARG: n < 0, width outside 1 - 128, stride_frames < 1, S * W above 0x7fffffff.  Host only. */
int64_t opusgpu_feat_batch_layout(int n, int width, int64_t stride_frames, int64_t *feat_offsets);
/* The stage alone over a packed grid in device memory (k_feat_stats, k_feat_fold, k_feat_batch): `spans` is a HOST array of n_tracks
 * records, tracks come out in span order; d_grid floats, 128-byte aligned, read in aligned 16-byte pieces inside a track's plane;
 * d_out n_tracks * S * W floats, 128-byte aligned, not overlapping the grid.  sub, mul_vec: as for opusgpu_set_feature_batch, `width`
 * of them.  Uploads the spans, its segment table and the vectors, launches on the context's stream (or `hip_stream`), waits, and
 * frees everything on every way out.  OPUSGPU_BAD_ARG before any device work: what opusgpu_set_feature_batch and
 * opusgpu_feat_batch_layout refuse, an unknown layout, a span that breaks a rule above. */
int opusgpu_tracks_feature_batch_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_feat_span *spans, int width, int layout,
                                        const opusgpu_feat_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid,
                                        void *d_out, void *hip_stream);

/* WAVE BATCHES.  The waveforms of a call as ONE dense float32 tensor at the model's rate, every track normalised by statistics of its
 * own and padded to a common length, with an attention mask: what wav2vec 2.0, HuBERT, WavLM and every pad_sequence collate function
 * take -- [B, T] at 16 kHz, zero mean and unit variance per utterance -- without a loop over tracks in the caller's code.  A stage
 * behind the kernels of TRACK RATES, CHANNEL MIX and TRACK RATIOS, which are unchanged: they write their int16 result into a
 * scratch grid of their own layout, 2 bytes a sample, and this stage writes the caller's buffer from there.  The result stays a
 * pure function of the int16 track, bit for bit.  The definition is this comment.
 *   INPUT.  For track t: y_c[m], the int16 result of those sections, interleaved, C = out_channels in [1, 8]; L[t] its output
 *   length, derived from the FINAL length; scale[t], the float scale the call would have used for a float format (a loudness gain is
 *   folded into it as TRACK LOUDNESS says).
 *   OUTPUT.  A dense float32 tensor of n * S * C elements, S = stride_samples.  OPUSGPU_TRACKS_F32: element (t * S + m) * C + c --
 *   [n, S, C], [n, S] for one channel.  OPUSGPU_TRACKS_F32_PLANAR: element (t * C + c) * S + m -- [n, C, S].  EVERY element is
 *   written exactly once, the pad cells m >= L[t] included; nothing outside the tensor is touched.  S is any integer >= 1 that holds
 *   every track's PLANNED output length, with S * C <= 0x7fffffff; nothing is asked of its alignment.
 *   MASK (optional).  uint8 [n, S]: 1 for m < L[t], else 0; every byte written once.  It lies behind the tensor in the same buffer,
 *   on the next 128-byte boundary (opusgpu_wave_batch_layout).
 *   STATISTICS are per track, over its N = L[t] * C real samples of all channels jointly: sum = sum y (int64), sumsq = sum y^2
 *   (uint64; N < 2^31 keeps it below 2^61), peak = max |y| (0 .. 32768).  All three are exact integers: they do not depend on the
 *   order of summation, on the padding or on which other tracks are in the call, so integer atomics keep the contract of identical
 *   bits from call to call.
 *   NORMALISATIONS (norm), y a real sample, k = (double)scale[t]:
 *     OPUSGPU_WAVE_NORM_NONE  out = (float)y * scale[t], one float32 multiplication: the very bits TRACK FORMATS writes.  Nothing is
 *       measured: the record's integers are 0, sub 0, mul 1.
 *     OPUSGPU_WAVE_NORM_ZMUV  (eps finite and > 0; Wav2Vec2FeatureExtractor's is 1e-7)  V = N * sumsq - sum^2 as an exact integer (up
 *       to 93 bits); sub = k * sum / N; mul = 1 / sqrt(k^2 * V / N^2 + eps).  N = 0: sub = 0, mul = 1 / sqrt(eps).
 *     OPUSGPU_WAVE_NORM_PEAK  (target finite and > 0)  sub = 0; mul = target / (peak * k), or 1 where peak * k is 0.
 *     Under ZMUV and PEAK a real cell is out = (float)(((double)y * k - sub) * mul): y * k is exact in double (16 x 24 bits), so the
 *     subtraction, the multiplication and the conversion are each rounded once, fused with the product or not.
 *   PAD CELLS hold pad_value verbatim (0: HF pads after normalising).
 *   RECORD.  opusgpu_wave_stat per track: count = N, the three integers, and sub and mul AS COMPUTED AND USED, within relative 2^-48
 *   of the definition above (eight double roundings of 2^-53, and as many for whoever checks it, doubled).  The output is a
 *   bit-for-bit function of the int16 track and the record, as normalised tracks are of the opusgpu_loudness gain.  A constant track
 *   has V = 0 and y * k - sub = 0 exactly (sub is formed as k * (sum / N), and sum / N is exact there): 0.0f in every real cell. */
#define OPUSGPU_WAVE_NORM_NONE 0
#define OPUSGPU_WAVE_NORM_ZMUV 1
#define OPUSGPU_WAVE_NORM_PEAK 2
typedef struct opusgpu_wave_batch_req { /* 64 bytes (ABI) */
    int64_t stride_samples; /* S, >= 1 */
    double eps;             /* ZMUV: finite and > 0 */
    double target;          /* PEAK: finite and > 0, the peak of the result */
    int32_t enabled;        /* opusgpu_set_wave_batch: 0 is off; the stand-alone call does not read it */
    int32_t norm;           /* OPUSGPU_WAVE_NORM_* */
    float pad_value;
    int32_t mask;           /* 1: the mask is written behind the tensor */
    int32_t reserved[6];    /* 0 */
} opusgpu_wave_batch_req;
typedef struct opusgpu_wave_span { /* 24 bytes, one per track (ABI) */
    int64_t in_offset; /* the track's first sample in the int16 grid, per channel; a multiple of 8 */
    int64_t samples;   /* L[t], 0 <= L <= S */
    float scale;       /* finite */
    int32_t reserved;  /* 0 */
} opusgpu_wave_span;
typedef struct opusgpu_wave_stat { /* 48 bytes, one per track (ABI) */
    int64_t count;  /* N = L * C */
    int64_t sum;
    uint64_t sumsq;
    double sub, mul;
    int32_t peak;
    int32_t reserved;
} opusgpu_wave_stat;
/* The request that holds for the whole-file calls that follow, as opusgpu_set_feature_batch does for its own; NULL or `enabled` 0
 * is off, the default, and every call is then byte for byte what it is above.  OPUSGPU_BAD_ARG, the request in force left as it
 * was: an unknown norm; a field that is not finite (eps, target, pad_value); eps <= 0 under ZMUV; target <= 0 under PEAK;
 * stride_samples < 1; a mask that is neither 0 nor 1; a reserved word that is not 0.  With a request on, the float-format calls
 * that end in a resampling kernel -- opusgpu_files_decode_resampled, _mixed and _ratio and their opusgpu_ms_ twins -- run their kernel
 * into an int16 scratch grid, then this stage writes d_out, which is now opusgpu_wave_batch_layout's total in floats, 128-byte
 * aligned; out_offsets[t] reports t * S; out_lengths, track_lengths_out and status_out are what they were, and a track that a failed
 * frame cut short pads from its final length; opusgpu_last_wave_stats has the records.  OPUSGPU_BAD_ARG before any device work, the
 * buffer and the arrays left as they were, with the reason in opusgpu_last_error: OPUSGPU_TRACKS_S16 with a request on; S below a
 * track's PLANNED output length; S * C above 0x7fffffff.  A loudness request composes untouched: its gain is in the scale.
 * opusgpu_files_decode, opusgpu_files_decode_as and the feature calls ignore the request. */
int opusgpu_set_wave_batch(opusgpu_ctx *ctx, const opusgpu_wave_batch_req *req);
int opusgpu_ms_set_wave_batch(opusgpu_ms *ms, const opusgpu_wave_batch_req *req);
/* The records of the last whole-file call that ran the stage, as opusgpu_last_loudness: copies min(n, have) of them and returns
 * `have`. */
int opusgpu_last_wave_stats(const opusgpu_ctx *ctx, int n, opusgpu_wave_stat *records);
int opusgpu_ms_last_wave_stats(const opusgpu_ms *ms, int n, opusgpu_wave_stat *records);
/* OUTPUT above for n tracks: returns the buffer's total in floats.  Without a mask that is n * S * C.  With one, the mask begins
 * *mask_byte_offset bytes (may be NULL) into the buffer, the first multiple of 128 at or behind the tensor's end, and the total
 * covers its n * S bytes.  OPUSGPU_BAD_ARG: n < 0, channels outside 1 - 8, stride_samples < 1, S * C above 0x7fffffff, a mask that
 * is neither 0 nor 1.  Host only. */
int64_t opusgpu_wave_batch_layout(int n, int channels, int64_t stride_samples, int mask, int64_t *mask_byte_offset);
/* The stage alone over int16 tracks in device memory (k_wave_stats, k_wave_fold, k_wave_batch): `spans` is a HOST array of n_tracks
 * records, tracks come out in span order; d_s16 interleaved int16 tracks of `channels` channels, 16-byte aligned, read in aligned
 * 16-byte pieces up to the one that holds a track's last sample; d_out opusgpu_wave_batch_layout's floats, 128-byte aligned, not
 * overlapping the tracks; format OPUSGPU_TRACKS_F32 or OPUSGPU_TRACKS_F32_PLANAR; stats_out n_tracks records on the HOST, or NULL.
 * Uploads the spans and its chunk table, launches on the context's stream (or `hip_stream`), waits, and frees everything on every
 * way out.  OPUSGPU_BAD_ARG before any device work: what opusgpu_set_wave_batch and opusgpu_wave_batch_layout refuse, another
 * format, a span that breaks a rule above. */
int opusgpu_tracks_wave_batch_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_wave_span *spans, int channels, int format,
                                     const opusgpu_wave_batch_req *req, const void *d_s16, void *d_out, opusgpu_wave_stat *stats_out,
                                     void *hip_stream);

/* WAVE TRIM.  The silence in front of and behind an utterance cut off before the tracks of a WAVE BATCHES call are collated:
 * librosa.effects.trim (top_db = 60 in most TTS recipes) and the absolute dBFS gate of ASR data preparation, as a stage between the
 * resampling kernel and the wave batch.  Trimming changes a row's length, the statistics ZMUV and PEAK are taken over and the mask,
 * so it cannot follow the dense tensor; here the wave batch simply sees shorter tracks.  A frame's energy of an int16 track is an
 * exact integer, so the trimmed batch stays a bit-for-bit function of the int16 track and a small record.  WAVE BATCHES, its records,
 * calls and kernels are unchanged.  The definition is this comment.
 *   INPUT.  For track t: y_c[m], the interleaved int16 result of the resampling kernel, C = out_channels in [1, 8]; L its output
 *   length, derived from the FINAL length, exactly as WAVE BATCHES takes it.
 *   PARAMETERS.  frame_length fl: a multiple of 16, 16 <= fl <= 8192.  hop: a multiple of 8, 8 <= hop <= fl.  margin: a multiple of
 *   8, >= 0, the samples kept on either side.  mode: OPUSGPU_WAVE_TRIM_REL or _ABS.  ratio: a double in (0, 1], read in REL mode --
 *   the caller passes 10^(-top_db / 10), no kernel calls pow; ABS only asks that it is finite.  threshold: a uint64, read in ABS
 *   mode, the frame-energy threshold in int16^2 units summed over the frame.  flags: 0 or 1.
 *   FRAMES.  F = 1 + L / hop (integer division).  Frame f covers the samples m in [f * hop - fl / 2, f * hop + fl / 2) that lie in
 *   [0, L): librosa.feature.rms(center=True, pad_mode="constant")'s framing.  Nothing at or behind L is read, interpreted or allowed
 *   to influence a bit -- the grid holds other tracks there.
 *   ENERGY.  E[c][f] = sum of y_c[m]^2 over the frame, an exact integer of at most 2^43.  M[f] = max over c of E[c][f] (librosa's
 *   aggregate=np.max).  Emax = max over f of M[f].
 *   THRESHOLD.  ABS: thr = threshold.  REL: thr = (uint64)floor((double)Emax * ratio) -- (double)Emax is exact, the product is
 *   rounded once, the floor is exact: numpy float64 reproduces thr bit for bit.
 *   ACTIVITY.  Frame f is active iff M[f] > thr, as integers.
 *   RESULT.  first and last are the first and the last active frame, active their count.  No active frame: start = 0, count = 0.
 *   Otherwise start = max(0, first * hop - margin), end = min(L, (last + 1) * hop + margin), count = end - start.  With margin 0
 *   these are librosa.effects.trim's indices.
 *   ONE DIVERGENCE.  A digitally silent track (Emax = 0) in REL mode trims to nothing: no M[f] is above 0.  librosa keeps it whole,
 *   because power_to_db clamps both sides of its comparison to amin.
 *   SCALE.  The energies are of the int16 samples IN FRONT OF scale[t]: a loudness gain, which is folded into the scale, does not
 *   move an ABS threshold and changes no trim index.
 *   RECORD.  opusgpu_wave_trim_stat per track: start, count, full = L, Emax, thr, frames = F, first, last (both -1 when nothing is
 *   active), active.
 *   FLAGS.  With flags = 1, one uint8 per frame (1 = active), the tracks packed back to back in track order, F[t] bytes each: what
 *   librosa.effects.split makes its intervals from. */
#define OPUSGPU_WAVE_TRIM_REL 0
#define OPUSGPU_WAVE_TRIM_ABS 1
typedef struct opusgpu_wave_trim_req { /* 64 bytes (ABI) */
    double ratio;         /* REL: in (0, 1]; ABS: finite */
    uint64_t threshold;   /* ABS */
    int32_t enabled;      /* opusgpu_set_wave_trim: 0 is off; the stand-alone call does not read it */
    int32_t mode;         /* OPUSGPU_WAVE_TRIM_* */
    int32_t frame_length; /* a multiple of 16 in [16, 8192] */
    int32_t hop;          /* a multiple of 8 in [8, frame_length] */
    int32_t margin;       /* a multiple of 8, >= 0 */
    int32_t flags;        /* 1: the activity flags are kept */
    int32_t reserved[6];  /* 0 */
} opusgpu_wave_trim_req;
typedef struct opusgpu_wave_trim_stat { /* 64 bytes, one per track (ABI) */
    int64_t start, count; /* the samples kept: [start, start + count) */
    int64_t full;         /* L, the untrimmed length */
    uint64_t emax, thr;
    int32_t frames;       /* F */
    int32_t first, last;  /* -1: no frame is active */
    int32_t active;
    int32_t reserved[2];  /* 0 */
} opusgpu_wave_trim_stat;
/* The request that holds for the whole-file calls that follow, as opusgpu_set_wave_batch does for its own; NULL or `enabled` 0 is
 * off, the default, and every call is then byte for byte what it is above.  OPUSGPU_BAD_ARG, the request in force left as it was
 * and the reason in opusgpu_last_error: a frame_length that is no multiple of 16 in [16, 8192]; a hop that is no multiple of 8 in
 * [8, frame_length]; a margin that is negative or no multiple of 8; an unknown mode; a ratio that is not finite, or outside (0, 1]
 * in REL mode; flags neither 0 nor 1; a reserved word that is not 0; a request turned on while the context holds no wave-batch
 * request -- the packed grids are planned on the host and cannot shrink, only the dense tensor's rows can.  With both requests on,
 * the calls that WAVE BATCHES names run this stage over their int16 scratch grid and hand the wave batch the trimmed tracks:
 * statistics, cells, padding and mask follow the trimmed track; out_lengths[t] reports the trimmed count, the row's real length;
 * track_lengths_out and status_out are what they were, and S is still held against the PLANNED, untrimmed length.  A call that
 * finds this request on and the wave-batch request off is refused before any device work, with the reason.  The calls that ignore
 * a wave-batch request ignore this one. */
int opusgpu_set_wave_trim(opusgpu_ctx *ctx, const opusgpu_wave_trim_req *req);
int opusgpu_ms_set_wave_trim(opusgpu_ms *ms, const opusgpu_wave_trim_req *req);
/* The records of the last whole-file call that ran the stage: copies min(n, have) of them and returns `have`. */
int opusgpu_last_wave_trim(const opusgpu_ctx *ctx, int n, opusgpu_wave_trim_stat *records);
int opusgpu_ms_last_wave_trim(const opusgpu_ms *ms, int n, opusgpu_wave_trim_stat *records);
/* FLAGS of that call, where its request asked for them: copies min(n_bytes, have) bytes and returns `have`, the sum of the records'
 * `frames` (0 without flags). */
int64_t opusgpu_last_wave_trim_flags(const opusgpu_ctx *ctx, int64_t n_bytes, uint8_t *flags);
int64_t opusgpu_ms_last_wave_trim_flags(const opusgpu_ms *ms, int64_t n_bytes, uint8_t *flags);
/* The stage alone over int16 tracks in device memory (k_wave_trim_energy, k_wave_trim_fold): `spans` is a HOST array of n_tracks
 * opusgpu_wave_span records (their scale is not read); d_s16 interleaved int16 tracks of `channels` channels, 16-byte aligned, read
 * in aligned 16-byte pieces up to the one that holds a track's last sample; stats_out n_tracks records on the HOST; flags_out the
 * HOST bytes of FLAGS, the sum over the tracks of 1 + samples / hop, or NULL -- it is written only where req->flags is 1.  Uploads
 * the spans and its tile table, launches on the context's stream (or `hip_stream`), copies the result back once, waits, and frees
 * everything on every way out.  OPUSGPU_BAD_ARG before any device work, with the reason: what opusgpu_set_wave_trim refuses of the
 * record, channels outside 1 - 8, a span that breaks a rule of WAVE BATCHES, samples * channels above 0x7fffffff, no stats_out. */
int opusgpu_tracks_wave_trim_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_wave_span *spans, int channels,
                                    const opusgpu_wave_trim_req *req, const void *d_s16, opusgpu_wave_trim_stat *stats_out,
                                    uint8_t *flags_out, void *hip_stream);

/* STFT BATCHES. The spectrograms of a TRACK STFT call as ONE dense tensor, padded to a common length and normalised per track: the
 * [B, 513, T] that VITS pads in its collate function, the complex [B, 257, T] of enhancement and separation models, the [B, 1025, T]
 * of music models, a spectrogram image in dB under its own maximum -- without a loop over tracks in the caller's code.  FEATURE
 * BATCHES, its record, its calls, its kernels and everything it refuses (widths above 128, an STFT call with a feature-batch
 * request on the context) are unchanged; this is a section of its own with a record, calls, kernels and a request of its own.  The
 * definition is this comment.
 *   INPUT.  A packed TRACK STFT grid: bins in [1, 1025]; c = 1 for real cells, 2 for (Re, Im) pairs; feat_offset[t] and plane[t]
 *   multiples of 64.  OPUSGPU_MEL_BANDS_MAJOR (bins-major): cell (k, f) at feat_offset[t] + (k * plane[t] + f) * c.
 *   OPUSGPU_MEL_FRAMES_MAJOR: cell (f, k) at feat_offset[t] + (f * bins + k) * c.  F[t] is the frame count of the track's FINAL
 *   length: cells f >= F[t] of the grid are never interpreted.  The real cells are finite; the caller of the stand-alone call
 *   guarantees it.
 *   OUTPUT.  One dense float32 tensor of n_tracks * S * bins * c floats, S = stride_frames, in the grid's own layout.  Bins-major:
 *   [n, bins, S], or [n, bins, S, 2] for pairs.  Frames-major: [n, S, bins], or [n, S, bins, 2] for pairs.  Track t begins at
 *   t * S * bins * c.  EVERY element is written exactly once, the pad cells f >= F[t] included; nothing outside the tensor is
 *   touched.  S is any integer >= 1 that holds every track's planned frames, with S * bins * c <= 0x7fffffff; nothing is asked of
 *   its alignment.
 *   STATISTICS are per track, over its F[t] real cells only: they never depend on pad cells, on the grid's padding or on which
 *   other tracks are in the call.
 *   NORMALISATIONS (norm), x a real cell of bin k.  OPUSGPU_FEAT_NORM_NONE, _WHISPER, _CMN, _CMVN and _AFFINE (0 - 4) are defined
 *   word for word as in FEATURE BATCHES, with `bins` in the place of W: sub and mul_vec have `bins` entries.  One more:
 *     OPUSGPU_STFT_NORM_REFMAX  m = the max over ALL real cells of the track (every bin); lo = m - range, one float32 subtraction;
 *       y = (fmaxf(x, lo) - m) * mul: two float32 operations, each rounded on its own, nothing fused.  With a log10 power
 *       spectrogram, range 8 and mul 10 this is dB under the track's own maximum with top_db = 80, librosa.power_to_db(ref=np.max).
 *       F = 0 has no maximum: every cell of such a track takes pad_value verbatim, whatever the pad mode.
 *   PAIRS (c = 2) take OPUSGPU_FEAT_NORM_NONE and _AFFINE only; AFFINE applies (x - sub[k]) * mul[k] to both members of bin k.
 *   Every other norm with pairs is refused before any device work, with the reason.
 *   PAD CELLS (pad_mode) are those of FEATURE BATCHES: OPUSGPU_FEAT_PAD_VALUE, pad_value verbatim; OPUSGPU_FEAT_PAD_NORMALIZED, the
 *   track's normalisation applied to pad_value as if it were a cell of that track and bin.  For pairs the pad value fills both
 *   members.
 *   CONTRACT.  The same bits from the same call on the same input; no float atomics.  NONE, WHISPER, REFMAX and AFFINE are
 *   bit-for-bit functions of the grid.  CMN and CMVN keep the per-bin summation order that FEATURE BATCHES fixes: segments of
 *   OPUSGPU_FEAT_SEG frames; bins-major a lane's cells (frames 4 l .. 4 l + 3 of every 256, l the lane) in ascending frame order,
 *   then the butterfly over the 64 lanes; frames-major every fourth frame per wave, then the four waves in ascending order; the
 *   segments folded in ascending order.  A bin's statistics therefore do not depend on `bins`: a grid of width <= 128 gives the same
 *   bits through this stage as through opusgpu_tracks_feature_batch_device, and so do the first 128 bins of a wider one.  The bound
 *   of FEATURE BATCHES holds unchanged, 2^-23 |y| + 2^-30 max_f |x[f][k]| / d, and a track whose real cells all hold one value gives
 *   exactly 0.0f in every real cell under CMN and CMVN (tests/test_gpu_stft_batch.py). */
#define OPUSGPU_STFT_NORM_REFMAX 5
typedef struct opusgpu_stft_batch_req { /* 64 bytes (ABI): the fields of opusgpu_feat_batch_req */
    int64_t stride_frames; /* S, >= 1 */
    double var_floor;      /* CMVN: finite and > 0 */
    int32_t enabled;       /* opusgpu_set_stft_batch: 0 is off; the stand-alone call does not read it */
    int32_t norm;          /* OPUSGPU_FEAT_NORM_* 0 - 4 | OPUSGPU_STFT_NORM_REFMAX */
    int32_t pad_mode;      /* OPUSGPU_FEAT_PAD_* */
    float pad_value;
    float range, add, mul; /* WHISPER: 8, 4, 0.25; REFMAX reads range and mul (dB: 8, 10) */
    int32_t reserved[5];   /* 0 */
} opusgpu_stft_batch_req;
typedef struct opusgpu_stft_batch_span { /* 24 bytes, one per track (ABI) */
    int64_t grid_offset; /* feat_offset[t], in floats; a multiple of 64 */
    int64_t plane;       /* plane[t], in frames: a multiple of 64 and >= frames */
    int64_t frames;      /* F[t], 0 <= F <= S and F < 2^29 */
} opusgpu_stft_batch_span;
/* The request that holds for the opusgpu_files_decode_stft / opusgpu_ms_files_decode_stft calls that follow, as
 * opusgpu_set_feature_batch does for its calls; NULL or `enabled` 0 is off, the default, and every call is then byte for byte what
 * it is above.  The other feature calls ignore the request.  sub and mul_vec: host arrays of `bins` floats for
 * OPUSGPU_FEAT_NORM_AFFINE, copied; not read otherwise.  OPUSGPU_BAD_ARG, the request in force left as it was: what
 * opusgpu_set_feature_batch refuses, with norms 0 - 5 and AFFINE vectors of 1 - 1025 entries.  With a request on, the two calls
 * write d_out as this section's tensor: d_out is opusgpu_stft_batch_layout's total in floats, 128-byte aligned; feat_offsets[t]
 * reports t * S * bins * c; frames_out, track_lengths_out and status_out are what they were; the caller's arrays are written last.
 * DIRECT PATH: with OPUSGPU_FEAT_NORM_NONE and S a multiple of 64 the tensor is itself a valid grid for k_tracks_stft (feat_offset
 * t * S * bins * c, plane S), which then writes the real cells straight into d_out, and k_stft_pad the pad cells behind them: no
 * scratch grid and no second pass over the cells.  Every other request runs the kernel into a scratch grid of opusgpu_stft_layout's
 * size, freed on every way out, and this stage from there.  Both paths give the same tensor bit for bit.  OPUSGPU_BAD_ARG before
 * any device work, the buffer and the arrays left as they were, with the reason in opusgpu_last_error: S below the frames of a
 * track's PLANNED length; S * bins * c above 0x7fffffff; AFFINE vectors that do not have `bins` entries; a norm that pairs do not
 * take.  A loudness request composes untouched: its gain is in the kernel's scale. */
int opusgpu_set_stft_batch(opusgpu_ctx *ctx, const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, int bins);
int opusgpu_ms_set_stft_batch(opusgpu_ms *ms, const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, int bins);
/* OUTPUT above for n tracks: writes feat_offsets[t] = t * S * bins * c (may be NULL) and returns the total n * S * bins * c in
 * floats.  OPUSGPU_BAD_ARG: n < 0, bins outside 1 - 1025, c neither 1 nor 2, stride_frames < 1, S * bins * c above 0x7fffffff.
 * Host only. */
int64_t opusgpu_stft_batch_layout(int n, int bins, int c, int64_t stride_frames, int64_t *feat_offsets);
/* The stage alone over a packed grid in device memory (k_stft_stats, k_stft_fold, k_stft_batch): opusgpu_tracks_feature_batch_device's
 * contract, alignment and "frees everything on every way out" rules with this section's record and widths -- `spans` a HOST array of
 * n_tracks records, tracks come out in span order; d_grid floats, 128-byte aligned, read in aligned 16-byte pieces inside a track's
 * planes; d_out n_tracks * S * bins * c floats, 128-byte aligned, not overlapping the grid; sub, mul_vec `bins` floats each for
 * AFFINE.  OPUSGPU_BAD_ARG before any device work, with the reason in opusgpu_last_error: what opusgpu_set_stft_batch and
 * opusgpu_stft_batch_layout refuse, an unknown layout, a span that breaks a rule above, a norm that pairs do not take. */
int opusgpu_tracks_stft_batch_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_stft_batch_span *spans, int bins, int c, int layout,
                                     const opusgpu_stft_batch_req *req, const float *sub, const float *mul_vec, const void *d_grid,
                                     void *d_out, void *hip_stream);

/* ---- WHOLE FILES / MULTISTREAM: N surround Ogg Opus files in, N trimmed interleaved tracks in HBM out -----------------------------
 * The two sections above joined: files whose OpusHead carries channel mapping family 1 (1 - 8 channels, `streams` elementary
 * streams) are planned by the same reader-driven loop as stereo files and decoded by an opusgpu_ms of their layout.  The reader's
 * bookkeeping looks only at a packet's first TOC byte -- elementary stream 0's, and every elementary stream of a packet has the
 * same duration -- and at the granule positions, so pre-skip, end trimming, holes, the 80 ms discard after a hole, spanning packets
 * and CRC resync are exactly what they are for a stereo file with the same pages (tests/test_ms_files_plan.py pins that).
 * File i is DECODER i.  Step k holds one row of `streams` descriptors (the layout opusgpu_ms_decode_step_device documents: row r =
 * descriptors [r * streams, (r + 1) * streams), stream field = the decoder, offsets into the batch's arena) for every file that
 * has a k-th frame, rows in file order, and one opusgpu_track_seg per row: `slot` is the row.  A segment counts samples per
 * channel, as above; a track holds `channels` interleaved int16 per sample and begins at a multiple of 64 samples.
 * Refusals, per file, never a failed call (a refused file contributes no row and a track of 0 samples):
 *   the OpusHead's layout differs from `layout` in channel, stream or coupled count or in a mapping entry -> OPUSGPU_BAD_ARG
 *     (family 0 heads are the layouts {1, 1, 0, {0}} and {2, 1, 1, {0, 1}});
 *   mapping family 255 -> OPUSGPU_UNIMPLEMENTED (the reader's OP_EIMPL);
 *   reference mode, an audio packet whose TOC names another frame duration than 20 ms -> OPUSGPU_UNIMPLEMENTED, as above;
 *   RFC mode, a packet whose elementary streams differ in frame count or in frame duration -> OPUSGPU_UNIMPLEMENTED: the device
 *     step takes rows of one duration (opusgpu_ms_decode_packets takes such packets one call at a time).
 *   A packet with a valid duration that opusgpu_ms_packet_to_frames rejects -- too short for its streams, a malformed elementary
 *   packet, streams of different durations, reference mode: of different frame counts -- ends the plan with OP_EBADPACKET (-136);
 *   what was planned before it is decoded.
 * A failed elementary frame fails its row (the first negative elementary result in stream order), and a failed row ends its track
 * as a failed frame does above (FAILED FRAMES). */
typedef struct opusgpu_ms_file_batch opusgpu_ms_file_batch;

/* The layout of one file, read from its OpusHead by the single-file reader's open (headers and the first audio page): family 0 gives
 * streams 1, coupled channels - 1 and the identity mapping, family 1 what the header says; mapping entries >= channels are 255.
 * A caller with a mixed corpus groups its files by this, one opusgpu_ms per layout.  info (may be NULL) receives status and the
 * OpusHead fields.  Returns OPUSGPU_OK, OPUSGPU_BAD_ARG, or what the reader says, e.g. -132 OP_ENOTFORMAT, -133 OP_EBADHEADER;
 * family 255 is OPUSGPU_UNIMPLEMENTED.  *layout is written only on success.  Host only. */
int opusgpu_file_layout(const uint8_t *file, int64_t len, opusgpu_ms_layout *layout, opusgpu_file_info *info);
/* opusgpu_files_plan for files of ONE layout.  There is no `flags`: the grouping flags order single frames by mode, and a row
 * mixes the modes of its elementary streams.  Returns OPUSGPU_OK, OPUSGPU_BAD_ARG (a layout opusgpu_ms_create would refuse
 * included) or OPUSGPU_ALLOC_FAIL.  Host only. */
int opusgpu_ms_files_plan(int n_files, const uint8_t *const *files, const int64_t *file_lens, const opusgpu_ms_layout *layout,
                          int mode, int threads, opusgpu_file_info *info, opusgpu_ms_file_batch **out);
int opusgpu_ms_file_batch_steps(const opusgpu_ms_file_batch *b);
/* Step `step`: returns its ROW count; *descs its table (rows x streams descriptors), *slot_files (may be NULL) the file of every row. */
int opusgpu_ms_file_batch_step(const opusgpu_ms_file_batch *b, int step, const opusgpu_frame_desc **descs, const int32_t **slot_files);
int opusgpu_ms_file_batch_segments(const opusgpu_ms_file_batch *b, int step, const opusgpu_track_seg **segs); /* one per row */
const uint8_t *opusgpu_ms_file_batch_arena(const opusgpu_ms_file_batch *b, size_t *bytes);
/* Samples per channel of the packed track buffer: allocate 2 * channels bytes for each. */
int64_t opusgpu_ms_file_batch_track_samples(const opusgpu_ms_file_batch *b);
int64_t opusgpu_ms_file_batch_packet_start(const opusgpu_ms_file_batch *b, int file, int packet_seq);
void opusgpu_ms_file_batch_free(opusgpu_ms_file_batch *b);

/* k_ms_tracks_assemble: the channel mapping and the track assembly in one pass.  Applies n_segs segments to the ELEMENTARY PCM of
 * one ms step -- d_pcm_coupled [rows * coupled][row_samples * 2] and d_pcm_mono [rows * (streams - coupled)][row_samples] int16,
 * with the elementary results d_res_coupled [rows * coupled] and d_res_mono [rows * (streams - coupled)], the layout in which the
 * object's two contexts leave a step -- and writes output channel c of every kept sample from decoded channel mapping[c] (255:
 * zero) into the packed track buffer d_tracks (`channels` interleaved int16 per sample, 128-byte aligned).  A row's result is its
 * first negative elementary result in stream order, else the common sample count (streams that disagree: OPUSGPU_INTERNAL_ERROR);
 * a negative one is a failed frame (FAILED FRAMES above).  Layouts of 1 - 8 channels (OPUSGPU_BAD_ARG otherwise); row_samples a
 * multiple of 8; PCM pointers 16-byte aligned; a pointer of a kind of stream the layout does not have may be NULL.  The caller
 * guarantees what opusgpu_tracks_assemble_device asks for.  Asynchronous on `hip_stream` (NULL: the object's own stream). */
int opusgpu_ms_tracks_assemble_device(opusgpu_ms *ms, int n_segs, const void *d_segs, const void *d_pcm_coupled,
                                      const void *d_pcm_mono, int row_samples, const void *d_res_coupled, const void *d_res_mono,
                                      void *d_tracks, void *d_track_state, void *hip_stream);
/* opusgpu_files_decode for a multistream batch: uploads it, gives decoders 0 .. n_files - 1 fresh state, and per step runs the row
 * split, the stereo step, the mono step and k_ms_tracks_assemble on the object's stream; the interleaved [rows][960 * channels]
 * PCM of opusgpu_ms_decode_step_device is never made.  Steps run in order.  The object must hold at least n_files decoders of the
 * batch's layout and be in the batch's mode (OPUSGPU_BAD_ARG otherwise).  d_tracks: opusgpu_ms_file_batch_track_samples x
 * channels int16 in HBM, 128-byte aligned; track_lengths_out and status_out as for opusgpu_files_decode. */
int opusgpu_ms_files_decode(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, void *d_tracks, int64_t *track_lengths_out,
                            int32_t *status_out);
/* Measurement aid (tools/ms_files_rate.py): the device time in ms of the step loop of this process's last successful
 * opusgpu_ms_files_decode -- split, both halves and the assembly of every step, without the upload and the reset in front of them
 * (events on the object's stream around the loop); -1 before the first call. */
float opusgpu_ms_files_last_steps_ms(void);
/* The two calls above for any track format (TRACK FORMATS in WHOLE FILES: value, layout, scale and the place record are the same,
 * `channels` the layout's; planar: output channel c's plane is decoded channel mapping[c] scaled, or zeros for 255).  Arguments,
 * refusals and alignment as opusgpu_tracks_assemble_device_as / opusgpu_files_decode_as say. */
int opusgpu_ms_tracks_assemble_device_as(opusgpu_ms *ms, int n_segs, const void *d_segs, const void *d_pcm_coupled,
                                         const void *d_pcm_mono, int row_samples, const void *d_res_coupled, const void *d_res_mono,
                                         int format, const void *d_place, void *d_tracks, void *d_track_state, void *hip_stream);
int opusgpu_ms_files_decode_as(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int format, const float *scale, void *d_tracks,
                               int64_t *track_lengths_out, int32_t *status_out);
/* opusgpu_files_decode_resampled behind opusgpu_ms_files_decode (TRACK RATES in WHOLE FILES): all of the layout's channels; there is no
 * `mono` -- a surround downmix needs a matrix and is not offered -- so rate 48000 is OPUSGPU_BAD_ARG here. */
int opusgpu_ms_files_decode_resampled(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int format, const float *scale,
                                      void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                                      int32_t *status_out);
/* opusgpu_files_decode_mixed behind opusgpu_ms_files_decode (CHANNEL MIX): the layout's channels through *mix, at any rate of TRACK
 * RATES -- the surround downmix that opusgpu_ms_files_decode_resampled does not have. */
int opusgpu_ms_files_decode_mixed(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, const opusgpu_mix_matrix *mix, int format,
                                  const float *scale, void *d_out, int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out,
                                  int32_t *status_out);
/* opusgpu_files_decode_ratio behind opusgpu_ms_files_decode (TRACK RATIOS): the layout's channels through *mix, or all of them
 * with mix NULL, at up / down of 48 kHz.  There is no `mono` here: the row of a mono mix is what it would be. */
int opusgpu_ms_files_decode_ratio(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int up, int down,
                                  const opusgpu_mix_matrix *mix /* NULL: none */, int format, const float *scale, void *d_out,
                                  int64_t *out_offsets, int64_t *out_lengths, int64_t *track_lengths_out, int32_t *status_out);
/* opusgpu_files_decode_mel behind opusgpu_ms_files_decode (TRACK FEATURES): the layout's channels through *mix, which must have
 * out_channels == 1; there is no `mono` here.  Refusals as there, plus a NULL mix. */
int opusgpu_ms_files_decode_mel(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, const opusgpu_mix_matrix *mix,
                                const opusgpu_mel_params *params, const float *scale, void *d_out, int64_t *feat_offsets, int64_t *frames_out,
                                int64_t *track_lengths_out, int32_t *status_out);

/* opusgpu_files_decode_melspec behind opusgpu_ms_files_decode (TRACK SPECTROGRAMS): the layout's channels through *mix, which must
 * have out_channels == 1; there is no `mono` here.  Refusals as there, plus a NULL mix. */
int opusgpu_ms_files_decode_melspec(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int up, int down,
                                    const opusgpu_mix_matrix *mix, const opusgpu_spec_params *p, const float *scale, void *d_out,
                                    int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out);

/* opusgpu_files_decode_fbank behind opusgpu_ms_files_decode (TRACK KALDI FEATURES): the layout's channels through *mix, which must
 * have out_channels == 1; there is no `mono` here.  Refusals as there, plus a NULL mix. */
int opusgpu_ms_files_decode_fbank(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int up, int down,
                                  const opusgpu_mix_matrix *mix, const opusgpu_fbank_params *p, const float *scale, void *d_out,
                                  int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out);

/* opusgpu_files_decode_stft behind opusgpu_ms_files_decode (TRACK STFT): the layout's channels through *mix, which must have
 * out_channels == 1; there is no `mono` here.  Refusals as there, plus a NULL mix. */
int opusgpu_ms_files_decode_stft(opusgpu_ms *ms, const opusgpu_ms_file_batch *batch, int rate, int up, int down,
                                 const opusgpu_mix_matrix *mix, const opusgpu_stft_params *p, const float *scale, void *d_out,
                                 int64_t *feat_offsets, int64_t *frames_out, int64_t *track_lengths_out, int32_t *status_out);

/* ---- WHOLE FILES / CUTS: pieces of files as tracks, with pre-roll, packed or at a fixed stride -------------------------------
 * A cut is samples [start, start + count) of a file's whole-file track (the axis opusgpu_files_plan makes: pre-skip, hole discards
 * and end trimming applied), decoded as a stream of its own the way RFC 7845 section 4.6 says: from a RESET decoder, starting at a
 * packet at least `preroll` decoded samples in front of `start`, the pre-roll thrown away.  The planner runs the reader ONCE per
 * file, however many cuts point into it, and makes an ordinary batch: track t and decoder stream t are cut t, its k-th decoded frame
 * goes in step k, and every accessor, opusgpu_files_decode* call, loudness request and kernel takes the batch as it takes any other.
 * WHICH PACKETS.  pa: the packet with packet_start[pa] <= start < packet_start[pa + 1].  D[p]: the decoded samples (TOC durations)
 * of the packets in front of p.  The lead a start at packet p gives is  D[pa] - D[p] + skip[pa] + (start - packet_start[pa])
 * (skip: what pre-skip or a hole's 80 ms discard takes off the front of pa).  first_packet is the largest p <= pa whose lead is at
 * least `preroll`; if there is none it is 0.  The last packet is the one that holds sample start + count - 1.  Packets outside
 * [first_packet, last] get no descriptor.
 * EXACT.  first_packet == 0: the cut's decoder sees what the whole file's decoder saw, and the cut is the whole-file track's slice
 * bit for bit.  Any other cut starts from reset state and is NOT bit-identical to that slice; it converges to it over the pre-roll
 * (DESIGN 13j has figures per mode).
 * CLAMPING.  start is clamped to [0, track length], count (< 0: to the end) to what is left.  A cut of 0 samples is legal: it has
 * no packets and no frames, lead 0, exact 1.
 * SEGMENTS of a cut keep, of the reader's kept range of every frame, what also lies in the cut; dst_first is relative to the cut's
 * start (plus the track's offset).  Frames wholly in the pre-roll keep a segment of count 0, whose result still counts.  packet_seq
 * counts from first_packet, and opusgpu_file_batch_packet_start(b, t, seq) is the cut's own table: 0 for the pre-roll packets, so a
 * failed frame in the pre-roll ends the cut at 0 samples and one inside it at its packet's start, by the FAILED FRAMES rule as it is.
 * BYTES.  The arena holds, per file, the bytes from the earliest first_packet to the latest last packet of its cuts, once;
 * descriptors of different cuts may name the same bytes.
 * INFO.  info[t]: the file's header fields, status and holes, with the cut's track_samples, track_offset, packets and frames.  A
 * file the whole-file planner refuses gives each of its cuts that status and no frames; a plan that ends in an error gives each
 * cut the status, and the cuts are clamped to the track planned up to there.  OPUSGPU_STEP_KEEPS_MODE is formed over the cuts'
 * own frames.
 * STRIDE.  track_stride 0: tracks are packed at multiples of 64 samples, as always.  Otherwise (a multiple of 64, at least every
 * clamped count, else OPUSGPU_BAD_ARG) track t begins at t * track_stride, opusgpu_file_batch_track_samples is n_cuts *
 * track_stride, the planes of OPUSGPU_TRACKS_F32_PLANAR lie track_stride apart, and opusgpu_files_decode / _as (and their
 * multistream twins) set every sample between a track's FINAL length and the stride to zero behind the last step
 * (opusgpu_tracks_fill_tail_device): the buffer is a [n_cuts, track_stride, channels] tensor ([n_cuts, channels, track_stride]
 * planar).  The resampled and feature outputs have grids of their own: every call that ends in another kernel refuses a strided
 * batch with OPUSGPU_BAD_ARG and says so in opusgpu_last_error.  Packed cut batches work with all of them.
 * Returns OPUSGPU_OK, OPUSGPU_ALLOC_FAIL, or OPUSGPU_BAD_ARG: what opusgpu_files_plan refuses, n_cuts < 0, cuts NULL with n_cuts > 0,
 * a `file` outside [0, n_files), a bad stride.  info (n_cuts entries) and cut_info (n_cuts entries) may be NULL.  Host only. */
typedef struct opusgpu_cut { /* 24 bytes (ABI) */
    int32_t file;    /* index into files[] */
    int32_t preroll; /* decoded samples per channel at 48 kHz wanted in front of `start`; < 0: 3840 (80 ms) */
    int64_t start;   /* first sample, on the axis of the file's whole-file track */
    int64_t count;   /* samples per channel; < 0: to the end of the track */
} opusgpu_cut;
typedef struct opusgpu_cut_info { /* 24 bytes (ABI) */
    int32_t first_packet; /* packet_seq, in the file, of the first packet decoded for the cut */
    int32_t packets;      /* packets decoded for it */
    int32_t lead;         /* decoded samples in front of `start` that the cut really gets (>= preroll unless exact) */
    int32_t exact;        /* 1: decoding starts at the file's first packet */
    int64_t start;        /* the cut's start after clamping to [0, track length] */
} opusgpu_cut_info;
#define OPUSGPU_CUT_PREROLL 3840
int opusgpu_files_plan_cuts(int n_files, const uint8_t *const *files, const int64_t *file_lens, int n_cuts, const opusgpu_cut *cuts,
                            int64_t track_stride, int channels, int mode, int flags, int threads, opusgpu_file_info *info,
                            opusgpu_cut_info *cut_info, opusgpu_file_batch **out);
int opusgpu_ms_files_plan_cuts(int n_files, const uint8_t *const *files, const int64_t *file_lens, int n_cuts, const opusgpu_cut *cuts,
                               int64_t track_stride, const opusgpu_ms_layout *layout, int mode, int threads, opusgpu_file_info *info,
                               opusgpu_cut_info *cut_info, opusgpu_ms_file_batch **out);
/* The batch's stride in samples per channel; 0 for a packed batch (every batch of opusgpu_files_plan); -1 for NULL. */
int64_t opusgpu_file_batch_track_stride(const opusgpu_file_batch *b);
int64_t opusgpu_ms_file_batch_track_stride(const opusgpu_ms_file_batch *b);

/* k_tracks_fill_tail: sets samples [first, end) per channel of every named track to zero, in the element size and placement of
 * `format` (OPUSGPU_TRACKS_*; placement as opusgpu_track_place says: interleaved, sample n of a track is elements channels *
 * (track_offset + n) ..; planar, channel c's are  channels * track_offset + c * plane_samples + n).  spans: HOST array, one per
 * track; 0 <= first <= end, track_offset >= 0, and for the planar format end <= plane_samples; an empty range writes nothing.
 * channels 1 .. 8.  One launch for all tracks: a lane owns an aligned 16-byte piece of the buffer and stores it whole; the first
 * and last piece of a range, where covered in part, go out as element stores, so nothing outside a range is touched.  d_tracks is
 * 128-byte aligned; the caller guarantees that the ranges lie inside it.  Queued on the context's stream (or `hip_stream`); the
 * call returns when the kernel has finished.  OPUSGPU_BAD_ARG for a span that breaks a rule. */
typedef struct opusgpu_tail_span { /* 32 bytes, one per track (ABI) */
    int64_t track_offset;  /* where the track begins in the buffer, samples per channel */
    int64_t plane_samples; /* planar: distance between the track's planes; interleaved: not read */
    int64_t first, end;    /* samples per channel of the track to zero: [first, end) */
} opusgpu_tail_span;
int opusgpu_tracks_fill_tail_device(opusgpu_ctx *ctx, int n_tracks, const opusgpu_tail_span *spans, int format, int channels,
                                    void *d_tracks, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
