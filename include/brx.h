/*
 * brx.h -- C ABI of the MI355X-native batched Brotli decompressor (libbrx.so).
 *
 * This is the drop-in boundary for the ONE hot path of ende76/brotli-rs: everything behind
 *     pub struct Decompressor<R: Read>            (reference src/lib.rs:377-394)
 *     pub fn new(r: R) -> Decompressor<R>          (reference src/lib.rs:398-410)
 *     impl<R: Read> Read for Decompressor<R>::read (reference src/lib.rs:2173-2193)
 * i.e. the private decompress() state machine (src/lib.rs:1545-2170) and the primitives under it
 * (src/bitreader, src/huffman, src/ringbuffer, src/lookuptable, src/dictionary, src/transformation).
 * The reference has no FFI of its own (pure safe Rust, `#![deny(unsafe_code)]`, src/lib.rs:1); the entry
 * points below are what a Rust `extern "C"` block for this path binds -- INTEGRATION.md shows the shim.
 *
 * Plain pointers and sizes only; no torch / HIP types in the signatures (a hipStream_t travels as void*).
 * Results are bit-exact with the reference: identical output bytes for valid streams and the identical
 * error kind (status 1..24 = DecompressorError in declaration order, src/lib.rs:294-319) for invalid ones.
 */
#ifndef BRX_H
#define BRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-stream status codes ------------------------------------------------------------------------
 * 0 = stream decoded; 1..24 = reference DecompressorError (src/lib.rs:294-319, same order);
 * 25/26 are additions of this build. */
enum {
    BRX_OK = 0,
    BRX_CODE_LENGTHS_CHECKSUM = 1,
    BRX_EXPECTED_END_OF_STREAM = 2,
    BRX_EXCEEDED_EXPECTED_BYTES = 3,
    BRX_INVALID_BLOCK_COUNT_CODE = 4,
    BRX_INVALID_BLOCK_SWITCH_COMMAND_CODE = 5,
    BRX_INVALID_LENGTH_IN_STATIC_DICTIONARY = 6,
    BRX_INVALID_MSKIP_LEN = 7, /* never observable, exactly like the reference (src/lib.rs:1661-1664) */
    BRX_INVALID_SYMBOL = 8,
    BRX_INVALID_TRANSFORM_ID = 9,
    BRX_INVALID_NON_POSITIVE_DISTANCE = 10,
    BRX_LESS_THAN_TWO_NON_ZERO_CODE_LENGTHS = 11,
    BRX_NO_CODE_LENGTH = 12,
    BRX_NON_ZERO_FILL_BIT = 13,
    BRX_NON_ZERO_RESERVED_BIT = 14,
    BRX_NON_ZERO_TRAILER_BIT = 15,
    BRX_NON_ZERO_TRAILER_NIBBLE = 16,
    BRX_PARSE_ERROR_CONTEXT_MAP = 17,
    BRX_PARSE_ERROR_COMPLEX_PREFIX_CODE_LENGTHS = 18,
    BRX_PARSE_ERROR_DISTANCE_CODE = 19,
    BRX_PARSE_ERROR_INSERT_AND_COPY_LENGTH = 20,
    BRX_PARSE_ERROR_INSERT_LITERALS = 21,
    BRX_RING_BUFFER_ERROR = 22,
    BRX_RUN_LENGTH_EXCEEDED_SIZE_OF_CONTEXT_MAP = 23,
    BRX_UNEXPECTED_EOF = 24,
    BRX_OUTPUT_TOO_SMALL = 25, /* capacity out_off[i+1]-out_off[i] exhausted; out_len[i] = bytes needed so far: the position in front of
                                  the item that did not fit plus that item's size (an insert's literals, a copy, a dictionary word, an
                                  uncompressed meta-block); no byte outside the slot is written for any status, the slot's own bytes are
                                  unspecified under this one */
    BRX_REF_PANIC = 26,        /* the reference would panic here: UppercaseFirst on a dictionary word that
                                  starts with 0x00 (src/transformation/mod.rs:52-82) */
    BRX_INTERNAL_WATCHDOG = 27 /* bug guard inside the kernel.  Unreachable from any stream the reference terminates on, by construction:
                                  (1) the loop guard counts commands and meta-blocks against  8 * input bytes + capacity + 65536 --
                                  every command consumes a bit or emits a byte (one that does neither -- one-symbol codes throughout and a
                                  transform that leaves nothing of its word -- repeats for ever in the reference too, src/lib.rs:2003-2141);
                                  (2) the wait for a spill slab: since round 6 the pool holds one slab per wave of ALL launches in flight
                                  on the context (at most the 16 waves per CU the chip can hold at a time), so no wave ever waits --
                                  until then a second overlapping launch could starve a wave for 4 s and end a VALID stream with 27 */
};

/* ---- library-level return codes (not per-stream) ---------------------------------------------------- */
enum {
    BRX_SUCCESS = 0,
    BRX_ERR_INVALID_ARGUMENT = -1,
    BRX_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at init: there is NO CPU fallback */
    BRX_ERR_HIP = -3,         /* a HIP call failed; brx_last_error() has the text */
    BRX_ERR_OUT_OF_MEMORY = -4
};

/* ---- options -------------------------------------------------------------------------------------- */
#define BRX_MEM_HOST 0u   /* every pointer argument is host memory; the library stages through HBM */
#define BRX_MEM_DEVICE 1u /* every pointer argument (data, offset tables, out_len, status) is device memory */
#define BRX_OPT_TIMING 2u /* record HIP-event timings of the kernels of this call (brx_last_timing) */
#define BRX_GEN_SWITCHES 8u /* brx_generate_batch only: two literal block types taking turns every 100 literals */
#define BRX_GEN_ADAPTIVE 16u /* brx_generate_batch only: the adaptive generator -- one wavefront per stream, prefix codes built
                                from each meta-block's own statistics (<= 15 bits, complex form with zero runs), two literal
                                trees behind a context map (mode UTF8), two literal block types switching every 1200 / 700
                                literals, last-distance codes; a slot of  len + len / 8 + 2048 * (len / metablock_bytes + 2)
                                bytes always suffices */
#define BRX_OPT_ORDER 4u  /* BRX_MEM_DEVICE only: queue the longest compressed streams first (a ragged batch finishes when
                             its longest stream does).  Costs one synchronous read of the offset table; the host-pointer
                             path always orders.  The work queue itself is dynamic: a wave that finishes a stream takes the
                             next one, so short streams never wait behind a fixed assignment. */

typedef struct brx_opts {
    uint32_t flags;   /* BRX_MEM_* | BRX_OPT_* */
    uint32_t reserved;
    void *hip_stream; /* hipStream_t to launch on, NULL = the context's own stream */
} brx_opts;

typedef struct brx_ctx brx_ctx; /* one per (process, GPU): device tables, spill-slab pool, HIP streams */

/* Threading and ordering contract.
 *  - Every entry point may be called from any thread.  Calls on ONE context are serialised on the host by a mutex
 *    (a batch call holds it until its work is enqueued -- and, for host pointers, finished); use one context per
 *    thread for host-side parallelism.  The reference Decompressor owns all of its state (src/lib.rs:377-394); a
 *    brx_stream does too once decoded.
 *  - Launches never share device state that matters: each gets its own work counter, and spill slabs are claimed by
 *    the waves themselves from a pool, so BRX_MEM_DEVICE calls enqueued on different HIP streams may overlap on the
 *    device.
 *  - BRX_MEM_DEVICE with hip_stream == NULL runs on the context's own NON-BLOCKING stream: it is not ordered after
 *    work on the caller's streams (not even the NULL stream).  Either pass the stream that produced the buffers in
 *    opts->hip_stream, or synchronise before the call.
 *  - A context that met streams whose prefix-code tables exceed the regular kernel's LDS also launches the wider kernel for
 *    them on a second HIP stream of its own, next to the regular kernel (forked from and joined back into the stream of the call
 *    with events: the call's stream order is unchanged, work enqueued behind the call sees all of its results).
 *  - Offset tables: in_off / out_off must be non-decreasing.  Host tables are checked (BRX_ERR_INVALID_ARGUMENT);
 *    in device memory a decreasing pair gives that stream an empty input (status 24) or zero capacity (status 25).
 *  - Per-stream limits of the 32-bit position arithmetic: output < 4 GiB - 256 B (more reports status 25 however
 *    large the capacity), input < 256 MiB for the fast path. */

/* Create a decoder context on HIP device `device` (0-based).  Fails with BRX_ERR_NO_DEVICE when no GPU is
 * present -- the product path never falls back to a CPU decoder. */
int brx_ctx_create(brx_ctx **out, int device);
void brx_ctx_destroy(brx_ctx *ctx);

/* Tuning and A/B knobs of a context: explicit arguments -- the library reads NO environment variable.  Takes effect for the
 * launches enqueued after the call; unknown options return BRX_ERR_INVALID_ARGUMENT, and so does a value outside an option's range
 * (checked first, before the context is looked at).  The defaults are the measured best; the
 * test suite uses these to reach every path (the C++-only command loops, both builds of the assembly loop, the wider kernel
 * instances behind / next to the regular one, the lean instance for short streams). */
enum {
    BRX_OPTION_COMMAND_LOOP = 1,  /* 0 = assembly loop with the C++ loop as its safety net (default); 8 = the C++ loop alone, whole
                                     meta-blocks; 7 = the C++ loop alone, re-entered after every command; 6 = the default loop with every
                                     meta-block treated as one the assembly loop cannot take (also honoured by bounded readers made after it) */
    BRX_OPTION_LOOP_BUILD = 2,    /* -1 = by occupancy (default); 0 = bit window in VGPRs (full chip); 1 = in SGPRs (sparse launch) */
    BRX_OPTION_QUEUE_ORDER = 3,   /* 1 = longest compressed stream first on the host path (default); 0 = index order */
    BRX_OPTION_HAND_UP = 4,       /* 1 = streams whose tables spill a kernel's LDS go to the wider instance that holds them (default);
                                     0 = they stay, tables in an HBM slab */
    BRX_OPTION_LEVELS = 5,        /* how the wider instances are launched: 0 = one catch-all launch behind the regular kernel, 2 = a
                                     header-only classification pre-pass, then all four instances next to each other, each on
                                     its own list; 1 (default) = the latter for contexts that listed a stream within their last
                                     64 launches */
    BRX_OPTION_TINY_BYTES = 6,    /* compressed size up to which the regular kernel runs a stream in its C++ loop alone (128) */
    BRX_OPTION_HOST_IN_PLACE = 7, /* 1 = pinned host buffers are read / written by the kernel itself (default); 0 = staged copies */
    BRX_OPTION_GRID_CAP = 8,      /* 0 = none (default); else at most this many resident waves of the regular kernel */
    BRX_OPTION_SMALL_BYTES = 9,   /* compressed size up to which a stream goes to the lean instance first (default 128, at most
                                     500; 0 = no lean instance) */
    BRX_OPTION_SMALL_WAVES = 10,  /* waves per CU of the lean instance's grid (default 32) */
    BRX_OPTION_TRACE = 11,        /* 1 = every launch records when and where each stream was decoded (brx_last_trace); default 0 */
    BRX_OPTION_READER_WINDOW = 12, /* compressed bytes a bounded / pulled stream keeps resident on the device (default 8 MiB; 1 .. 256
                                     MiB): streams started afterwards */
    BRX_OPTION_LEVEL4 = 13,       /* 1 = behind every batch launch one more (usually empty, 4 us) launch of the level-4 instance -- 150 KiB
                                     of LDS, one per CU -- takes the streams whose prefix-code tables spill even level 3 (pieces of several
                                     MiB compressed in one go) (default); 0 = no such launch: those meta-blocks run in the C++ loop from a
                                     slab (~3 MB/s per stream).  For callers whose batches are tens of microseconds long and never hold
                                     such streams */
    BRX_OPTION_READER_MB_ROOM = 14, /* 1 = a bounded / pulled stream pauses in front of a compressed meta-block that does not fit behind its output
                                     window and lets the buffer grow to window + meta-block (at most ~34 MiB), so that the fast loop runs it
                                     (default); 0 = such meta-blocks decode command by command in the ~22 MiB buffer (~8 x slower): streams
                                     started afterwards */
    BRX_OPTION_READER_BATCH = 15, /* 1 = the slices of bounded / pulled streams that are asked for at the same time go out together, one launch
                                     per round (default; brx_stream_advance, and brx_stream_read on many threads); 0 = every slice is a launch
                                     of its own, read back from the device (the A/B switch) */
    BRX_OPTION_PRIO_SHIFT = 16    /* 0 .. 31: the waves of a SIMD take the four issue
                                     priorities by turns, level = ((100 MHz realtime clock >> this) + the wave's rank) & 3 -- a level lasts
                                     2^this x 10 ns (default 16: 655 us); 31 = the levels never change.  Results do not depend on it */
};
int brx_ctx_set_option(brx_ctx *ctx, uint32_t option, int64_t value);

/* Decode `n` independent Brotli streams (the batch analogue of constructing n reference Decompressors and
 * calling read_to_end on each: benches/lib.rs:45-46, tests/lib.rs everywhere).
 *   in       concatenated compressed streams; stream i is in[in_off[i] .. in_off[i+1])
 *   in_off   n+1 offsets
 *   out      output arena; stream i may write out[out_off[i] .. out_off[i+1])  (capacity, not size)
 *   out_off  n+1 offsets
 *   out_len  n  decoded sizes (valid for status 0; "needed so far" for status 25).  For the other statuses: how far the decoder got --
 *               the slot's bytes [0, min(out_len, capacity)) are the stream's output in front of the error (the prefix a streaming
 *               reader has been handed; tools/prefix_fuzz.py holds it to the oracle); how far INTO the failing command that is, is
 *               not specified (nor by the reference: src/lib.rs:2173-2193 drops what the failing decompress() call had written)
 *   status   n  per-stream status codes (see above).  One bad stream never affects another.
 * Synchronous with respect to the host unless opts->hip_stream is given and BRX_MEM_DEVICE is set, in
 * which case the call only enqueues work on that stream -- EXCEPT under launch plan B (BRX_OPTION_LEVELS = 2, or a context that
 * met streams for the wider instances within its last 64 launches): the call then waits on the host for its classification
 * pre-pass (0.3 .. 1 ms: it reads six counters to size the instances' grids) before it enqueues the decode kernels and returns.
 * Everything it enqueues stays stream-ordered; only the host thread is held.  BRX_OPTION_LEVELS = 0 never waits.
 * Returns BRX_SUCCESS or a BRX_ERR_* code. */
int brx_decode_batch(brx_ctx *ctx, const uint8_t *in, const uint64_t *in_off, uint32_t n, uint8_t *out,
                     const uint64_t *out_off, uint64_t *out_len, int32_t *status, const brx_opts *opts);

/* The reference's exact error description strings (src/lib.rs:331-354, typos included) for 1..24. */
const char *brx_status_str(int32_t status);

/* Text of the last library-level error on this thread. */
const char *brx_last_error(void);

/* Timing of the most recent brx_decode_batch call made with BRX_OPT_TIMING (milliseconds, HIP events on
 * the launch stream).  which: 0 = whole device section, 1 = decode kernels. Returns <0 if unavailable.
 * which = 2 .. 7 (no BRX_OPT_TIMING needed; waits for the most recent launch): counters of that launch.  Streams whose
 * prefix-code tables do not fit the regular 6 912 B of LDS table memory are handed over on the device to the instance of the
 * kernel that holds them -- 9 472 / 17 152 / 37 632 B of table memory, 12 / 8 / 4 instead of 16 streams per CU:
 *   2, 3, 4  streams decoded at level >= 1, >= 2, 3 (2 = every stream that left the regular kernel)
 *   5        streams the lean instance (short streams, 32 per CU, launched in front of the regular kernel) left to the regular
 *            kernel -- the ones above its size limit plus the short ones it gave up on (any error, block switches, large tables);
 *            0 when the launch had no lean instance in front (BRX_OPTION_SMALL_BYTES 0, no stream within the limit, a reader round)
 *   6        streams that were handed up at a LATER meta-block, with their decoder state (resumed there, not restarted)
 *   7        output bytes decoded twice because of hand-overs (0 = every such stream was resumed where it stood)
 *   8        (since the context was made) slices of bounded / pulled streams that paused in front of an item -- a header, an
 *            uncompressed block, a command -- that the RESIDENT input did not hold, to run it with more (brx_stream_new_reader)
 *   9        (since the context was made) pauses of bounded / pulled streams in front of ONE item (a long copy or insert, an uncompressed
 *            meta-block) that did not fit the room behind the output window: the window slides, and if that is not enough the buffer
 *            grows to hold the item
 *   10       streams of the most recent launch whose fast loop had read on past the end of the input (truncated / corrupted streams
 *            only; 0 for valid ones): they went back to a checkpoint a few dozen dwords in front of the end and were finished with
 *            the exact end-of-input rules (round 5 took the whole meta-block back: a cut 1 MiB stream stalled its batch)
 *   11       streams of the most recent launch that the level-3 kernels handed on to the level-4 instance (150 KiB of LDS, one per
 *            CU: meta-blocks with more than 37.6 KiB of prefix-code tables -- one piece of several MiB from an encoder)
 *   12       (since the context was made) waves that did not get a spill slab at their first pass over the pool.  0 by construction
 *            since round 6: the pool has a slab for every wave of every launch in flight on the context (BRX_INTERNAL_WATCHDOG)
 *   13       slabs of the context's spill pool (896 KiB each; it grows with the launches in flight, to at most what the chip runs at a time)
 *   14, 15   (since the context was made) batches the Read facade launched for queued streams / streams in them: how well the host's
 *            threads coalesce (brx_stream_new below; a status-25 retry counts again)
 *   16, 17   (since the context was made) slice launches of bounded / pulled streams / slices in them: how well their slices coalesce
 *            into rounds (brx_stream_advance below; with BRX_OPTION_READER_BATCH = 0 every launch holds one slice)
 */
double brx_last_timing(brx_ctx *ctx, int which);

/* Diagnostics (BRX_OPTION_TRACE = 1): 4 words per stream of the most recent launch -- start and end of its decode on the GPU's
 * 100 MHz realtime counter, place of the wave that decoded it | kernel level << 32, workgroup index | grid size << 32.  The place:
 * bits 15:0 of the HW_ID register (wave slot 3:0, SIMD 5:4, pipe 7:6, CU 11:8, SH 12, SE 15:13), XCC_ID in bits 19:16, the wave's
 * rank in the priority rotation in bits 21:20 and BRX_OPTION_PRIO_SHIFT in bits 28:24.  Streams decoded by the lean instance have all-zero records.  Waits for that launch.
 * While the option is on, the host-pointer path decodes a batch in ONE launch (no chunks on separate HIP streams). */
int brx_last_trace(brx_ctx *ctx, uint64_t *dst, uint32_t n);

/* Blocks until everything enqueued on the context's stream (or `hip_stream`) has finished. */
int brx_synchronize(brx_ctx *ctx, void *hip_stream);

/* Pinned (page-locked, device-mapped) host memory for the host-pointer path.  With buffers from brx_host_alloc (or
 * hipHostMalloc / hipHostRegister with the mapped flag) brx_decode_batch makes no copies around the kernel: the kernel
 * reads the compressed bytes in place (a wave stages its input 256 bytes ahead of its cursor, the PCIe round trip hides
 * behind ~40 us of decoding) and stores every output byte to the host buffer itself while it decodes, next to the copy
 * in HBM that serves as the stream's window -- the device-to-host transfer rides on the decode as 1 KiB writes.  The
 * output pointer must sit at the 16-byte phase of its offsets (out + out_off[0] 16-byte aligned), else -- and with
 * pageable memory -- the batch is staged: input copy, decode, output copy, in chunks on their own HIP streams from the
 * second grid-full of streams on.  With the output stored in place only the stream's bytes are written; a staged copy
 * brings a slot's slack along.  (Ingest shape of the reference's file walker, src/main.rs:49-70: read files straight
 * into such a buffer, decode, write out -- brotli-rs_amd/host/brx_walk.cpp.) */
void *brx_host_alloc(size_t bytes);
void brx_host_free(void *p);

/* ---- Stream generator (the reference has no encoder, README.md:1) -------------------------------
 * Makes n valid Brotli streams ON THE DEVICE from n inputs: a minimal encoder, one GPU thread per stream -- greedy LZ77
 * over a 2048-entry hash table, the input cut into meta-blocks of `metablock_bytes` (0 = 65536, at most 2^24), every
 * meta-block with one block type per category and three static complete prefix codes sent in complex form (literals
 * 8 bits, insert&copy symbols 9/10 bits, distances 6 bits + extra; csrc/brx_gen.hip).  For batches of real, compressible
 * streams of any size without committed fixtures and for differential fuzzing: every stream it makes decodes back to its
 * input with brx_decode_batch and with any conforming decoder.
 *   src / src_off   n inputs, concatenated (input i is src[src_off[i] .. src_off[i+1]), may be empty)
 *   out / out_off   n output slots; a slot of  len + len / 8 + 256 * (len / metablock_bytes + 2)  bytes always suffices
 *   out_len         n  compressed sizes
 *   status          n  0, or 25 when the slot was too small (out_len then says how much was needed)
 * Pointers are host memory (staged) or, with BRX_MEM_DEVICE in opts->flags, device memory (opts->hip_stream as for
 * brx_decode_batch).  BRX_GEN_SWITCHES in opts->flags: every meta-block declares two literal block types (sharing the
 * one literal tree) and switches between them every 100 literals -- the block-switch commands of the format, 4 bits each.  Returns BRX_SUCCESS or a BRX_ERR_* code.
 * The generator's hash tables live in ONE scratch buffer per context: device-pointer calls on different HIP streams of one
 * context are not concurrent-safe (use one context per stream); a call that needs a larger scratch synchronizes the device
 * before it replaces the old one. */
int brx_generate_batch(brx_ctx *ctx, const uint8_t *src, const uint64_t *src_off, uint32_t n, uint8_t *out,
                       const uint64_t *out_off, uint64_t *out_len, int32_t *status, uint32_t metablock_bytes,
                       const brx_opts *opts);

/* ---- the decoded bytes of a batch, back to back (device memory only) ------------------------------------
 * brx_decode_batch leaves stream i in a slot sized for the worst case; whoever ships the results on (the ragged gather of
 * SURVEY 8e, a writer of one concatenated file) wants them without the slack:
 *   dst[dst_off[i] .. dst_off[i] + len[i])  =  out[out_off[i] .. out_off[i] + len[i])      for i < n
 * `len` is brx_decode_batch's out_len (zero the entries of failed streams first); dst_off is its exclusive prefix sum
 * (n entries, computed by the caller, e.g. torch.cumsum) and `total` its grand total.  All pointers are DEVICE memory.
 * hip_stream NULL = the context's own stream and the call returns when the copy is done; otherwise it is enqueued.
 * One pass at HBM rate (reads `total`, writes `total`); no reference counterpart (a `Decompressor` owns one stream). */
int brx_compact_batch(brx_ctx *ctx, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                      uint8_t *dst, const uint64_t *dst_off, uint64_t total, void *hip_stream);

/* ---- checksums of the decoded bytes of a batch (device memory only) --------------------------------------
 * Brotli carries no checksum; the containers around it keep one of the DECODED bytes, nearly always one of these two.  A batch
 * that stays on the device is verified there: nothing but the digests (or n mismatch words) ever crosses to the host.
 *   digest[i] = CRC of out[out_off[i] .. out_off[i] + len[i])                                   for i < n
 * `len` is brx_decode_batch's out_len (zero the entries of failed streams first), exactly as for brx_compact_batch; len[i] = 0
 * gives 0, the CRC of the empty string.  Bytes of a slot beyond len[i] never enter the result; out_off needs no alignment; len[i]
 * runs up to the per-stream limit (4 GiB - 256 B).  All pointers are DEVICE memory.
 *   expect / mismatch   both NULL, or both n entries: mismatch[i] = 1 where digest[i] != expect[i], else 0.  No total is written
 *                       (there is no mismatch[n]): the caller sums the array -- one n-word readback verifies a batch.
 * hip_stream NULL = the context's own stream and the call returns when the digests are there; otherwise it is enqueued (behind a
 * brx_decode_batch on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.
 * Scratch (per-stream accumulators, tile prefix sums, a ticket counter) belongs to the context, every launch has a region of its
 * own, so calls on different HIP streams of one context may overlap; a call with a larger n than any before synchronises the
 * device once to grow it, and the 17th call in flight waits on the host for the first.  The tables are built by the host from the
 * generator polynomial the first time a context uses a kind (one blocking 28 KiB upload).
 * BRX_ERR_INVALID_ARGUMENT: an unknown kind, digest NULL, only one of expect / mismatch.  n = 0 returns BRX_SUCCESS, no launch.
 * One pass over the bytes (reads sum(len), writes 4 n); no reference counterpart. */
#define BRX_DIGEST_CRC32 1u  /* reflected 0xEDB88320, init / xorout 0xFFFFFFFF: zlib, gzip, zip, PNG */
#define BRX_DIGEST_CRC32C 2u /* reflected 0x82F63B78, same init / xorout: iSCSI, ext4, most object stores */
int brx_digest_batch(brx_ctx *ctx, uint32_t kind, const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                     uint32_t *digest, const uint32_t *expect, uint32_t *mismatch, void *hip_stream);

/* ---- record boundaries of the decoded bytes of a batch (device memory only) -------------------------------
 * Nearly everything that is decoded is delimited text, and the first thing a consumer on the device (a tokenizer, a parser, a data
 * loader) does with a batch is find where its records start.  This pass knows the slot layout and does it at memory rate:
 *   count[i]              = number of bytes equal to `delim` in out[out_off[i] .. out_off[i] + len[i])          for i < n
 *   pos[pos_off[i] + k]   = offset WITHIN stream i of its k-th such byte, ascending in k                          (fill mode)
 * out, out_off, len and n are exactly as for brx_compact_batch and brx_digest_batch: `len` is brx_decode_batch's out_len with the
 * entries of failed streams zeroed, out_off needs no alignment, bytes of a slot beyond len[i] never enter a result.  All pointers
 * are DEVICE memory.
 *   span      the size in bytes of the arena `out` points into.  The caller guarantees out_off[i] + len[i] <= span and that slots do
 *             not overlap.  The host uses it for one thing: to bound the work items (at most span / 65536 + 2 n tiles of 64 KiB), so
 *             that scratch is sized without a length read back.  Nothing at or beyond out + span (or in front of out) is ever
 *             loaded; a batch with more tiles than `span` allows has the surplus ignored, never written out of bounds.
 *   count mode (pos_off == NULL and pos == NULL; count required): count[i] as above, n entries.
 *   fill mode  (pos_off and pos both given; count may be NULL, and if given it is written as in count mode): pos_off is the exclusive
 *             prefix sum of the counts (n entries, computed by the caller, e.g. torch.cumsum -- the convention of dst_off of
 *             brx_compact_batch) and `total` the number of entries pos has room for: an entry whose index is >= total is not
 *             written, so a caller whose counts went stale corrupts nothing.
 * Record k of stream i is the bytes [pos[k-1] + 1, pos[k]] of the stream (from 0 for k = 0), its delimiter included; a trailing
 * record without a delimiter runs from behind the last position to len[i].
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued (behind a
 * brx_decode_batch on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.
 * Scratch (tile prefix sums, per-tile counts, two ticket counters) belongs to the context and is sized from n and span; every
 * launch has a region of its own, so calls on different HIP streams of one context may overlap; a call with a larger n or span than
 * any before synchronises the device once to grow it, and the 17th call in flight waits on the host for the first.
 * BRX_ERR_INVALID_ARGUMENT: ctx NULL, out_off or len NULL with n > 0, only one of pos_off / pos, count NULL in count mode.
 * n = 0 returns BRX_SUCCESS, no launch.  Count mode is one pass over the bytes (reads sum(len), writes 8 n), fill mode two (the
 * second mostly from cache) plus 8 bytes per delimiter; no reference counterpart. */
int brx_index_batch(brx_ctx *ctx, uint8_t delim,
                    const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                    uint64_t span,
                    uint64_t *count,
                    const uint64_t *pos_off, uint64_t *pos, uint64_t total,
                    void *hip_stream);

/* ---- record boundaries that respect quoted fields (device memory only) -----------------------------------
 * The commonest delimited text is CSV (RFC 4180), and there a delimiter inside a quoted field is data: a consumer that splits a
 * decoded CSV batch at the positions of brx_index_batch tears records.  This pass applies the quoting rule on the device.  Stream i is
 * s = out[out_off[i] .. out_off[i] + len[i]); let q(j) be the number of bytes equal to `quote` in s[0 .. j).  Then
 *   s[j] == delim is a RECORD DELIMITER iff q(j) is even (an embedded quote is doubled, so it toggles twice and changes nothing)
 *   count[i]              = number of record delimiters of stream i                                            for i < n
 *   pos[pos_off[i] + k]   = offset WITHIN stream i of its k-th record delimiter, ascending in k                 (fill mode)
 *   open[i]               = q(len[i]) & 1: 1 where the stream ends inside a quoted field (truncated or malformed CSV), else 0
 * Every stream starts outside quotes, whatever bytes lie in front of it in its slot.  With delim = ',' the same call gives the field
 * separators outside quotes.
 * Not in scope: escape characters (here a quote is a quote wherever it stands; for backslash dialects see brx_index_escaped_batch
 * below), delimiters of more than one byte, and CR handling (for CRLF text the consumer trims the CR in front of a position).
 * Everything else is as for brx_index_batch: device pointers only; out, out_off, len, n and span as there; count mode (pos_off ==
 * NULL and pos == NULL; count required) and fill mode (pos_off and pos both given; count may be NULL, and if given it is written as
 * in count mode; `total` bounds the entries written to pos); hip_stream NULL = the context's own stream and the call returns when
 * the results are there, otherwise it is enqueued.  `open` (n entries of 32 bits) may be NULL in either mode.  The context's lock is
 * held to enqueue only.  Scratch (tile prefix sums, one word per tile and one more, two ticket counters) belongs to the context and
 * is sized from n and span with no length read back; every launch has a region of its own, so calls on different HIP streams of one
 * context may overlap; a call with a larger n or span than any before synchronises the device once to grow it, and the 17th call
 * in flight waits on the host for the first.
 * BRX_ERR_INVALID_ARGUMENT: ctx NULL, delim == quote, out_off or len NULL with n > 0, only one of pos_off / pos, count NULL in count
 * mode.  n = 0 returns BRX_SUCCESS, no launch.  Count mode is one pass over the bytes and a one-workgroup pass over the tiles, fill
 * mode a second pass over the bytes plus 8 bytes per record delimiter; no reference counterpart. */
int brx_index_quoted_batch(brx_ctx *ctx, uint8_t delim, uint8_t quote,
                           const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                           uint64_t span,
                           uint64_t *count, uint32_t *open,
                           const uint64_t *pos_off, uint64_t *pos, uint64_t total,
                           void *hip_stream);

/* ---- record boundaries under a dialect with an escape byte (device memory only) --------------------------
 * The largest family of delimited text escapes instead of (or on top of) quoting: JSON and JSON Lines write a quote inside a string
 * as \", PostgreSQL COPY text, MySQL / MariaDB tab dumps and Hive text tables have no quoting at all and put a backslash in front of
 * a delimiter that is data, and CSV is written with an escape character in place of doubled quotes (Python's escapechar, SQL's ESCAPED
 * BY).  Split at the positions of brx_index_batch or brx_index_quoted_batch such text tears.  This pass applies the rule on the device.
 * Stream i is s = out[out_off[i] .. out_off[i] + len[i]); D = delim, Q = quote, E = escape.
 *   esc(0) = 0 and esc(j + 1) = (s[j] == E && !esc(j)).  Byte j is ESCAPED iff esc(j): equivalently, iff the maximal run of E bytes
 *       directly in front of it, inside the stream, has odd length.  An escaped byte is data whatever its value, an E included.
 *   an ACTIVE QUOTE is a byte equal to Q that is not escaped; q(j) is the number of active quotes in s[0 .. j)
 *   s[j] is a RECORD DELIMITER iff s[j] == D, byte j is not escaped, and q(j) is even.  The escape acts inside and outside quoted
 *       fields alike; a doubled quote still toggles twice, so RFC 4180 text with an escape dialect on top behaves as expected.
 *   count[i]              = number of record delimiters of stream i                                            for i < n
 *   pos[pos_off[i] + k]   = offset WITHIN stream i of its k-th record delimiter, ascending in k                 (fill mode)
 *   open[i]               = two bits.  bit 0 = q(len[i]) & 1: the stream ends inside a quoted field.  bit 1 = esc(len[i]): the stream
 *                           ends on an active escape, one that has nothing to escape (truncated text).
 * Every stream starts unescaped and outside quotes, whatever bytes lie in front of it in its slot, and nothing behind the stream
 * (slack, a neighbouring stream) takes part: an escape on a stream's last byte does not escape the first byte of the next stream.
 *   flags     BRX_INDEX_NO_QUOTE: no byte is a quote -- the `quote` argument is ignored and bit 0 of open[i] is 0 -- for the quote-less
 *             dialects above.  Other bits must be 0.
 * With delim = ',' the same call gives the field separators; for JSON Lines those are the commas outside strings.
 * Not in scope: delimiters, quotes or escapes of more than one byte; escapes that act only inside quotes; decoding what an escape
 * sequence means (\n, \uXXXX); CR handling.  Several delimiters in one call (',' and '\n', the structural characters of JSON) and
 * an RFC 4180 dialect without an escape are brx_index_set_batch below.
 * Everything else is as for brx_index_quoted_batch: device pointers only; out, out_off, len, n and span as there (nothing at or beyond
 * out + span, or in front of out, is ever loaded); count mode (pos_off == NULL and pos == NULL; count required) and fill mode (pos_off
 * and pos both given; count may be NULL, and if given it is written as in count mode; `total` bounds the entries written to pos);
 * `open` (n entries of 32 bits) may be NULL in either mode; hip_stream NULL = the context's own stream and the call returns when the
 * results are there, otherwise it is enqueued.  The context's lock is held to enqueue only.  Scratch (tile prefix sums, two words per
 * tile and one more, two ticket counters) belongs to the context and is sized from n and span with no length read back; every launch
 * has a region of its own (a ring of 16, separate from the other passes'), so calls on different HIP streams of one context may
 * overlap; a call with a larger n or span than any before synchronises the device once to grow it, and the 17th call in flight waits
 * on the host for the first.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits; delim == escape; without
 * BRX_INDEX_NO_QUOTE quote == delim or quote == escape; only one of pos_off / pos; count NULL in count mode; then n = 0 returns
 * BRX_SUCCESS, no launch; then out_off or len NULL, span out of range.
 * Count mode is one pass over the bytes and a one-workgroup pass over the tiles, fill mode a second pass over the bytes plus 8 bytes
 * per record delimiter; no reference counterpart. */
#define BRX_INDEX_NO_QUOTE 1u
int brx_index_escaped_batch(brx_ctx *ctx, uint8_t delim, uint8_t quote, uint8_t escape, uint32_t flags,
                            const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                            uint64_t span,
                            uint64_t *count, uint32_t *open,
                            const uint64_t *pos_off, uint64_t *pos, uint64_t total,
                            void *hip_stream);

/* ---- boundaries at a set of delimiter bytes, with optional quote and escape (device memory only) ---------
 * Hardly any consumer of delimited text wants one kind of boundary: a CSV reader needs the field separators and the record ends (','
 * '\n', often '\r'), a JSON Lines parser the structural characters outside strings ('{' '}' '[' ']' ':' ',' and the line feed),
 * universal newlines are '\r' or '\n'.  With the passes above that is one fill-mode call per byte value, each walking the bytes twice,
 * and a merge of sorted position lists.  This pass takes a SET of 1 .. 8 delimiter bytes, delims[0 .. n_delims), in one call and says
 * for every position which of them stands there.
 * Stream i is s = out[out_off[i] .. out_off[i] + len[i]).  esc(j), ACTIVE QUOTES, q(j) and open[i] are word for word those of
 * brx_index_escaped_batch.
 *   s[j] is a BOUNDARY iff s[j] is one of delims[0 .. n_delims), byte j is not escaped, and q(j) is even
 *   count[i]              = number of boundaries of stream i                                                     for i < n
 *   pos[pos_off[i] + k]   = offset WITHIN stream i of its k-th boundary, ascending in k                           (fill mode)
 *   what[pos_off[i] + k]  = the byte found there, s[pos[pos_off[i] + k]]: the delimiter's VALUE, not its index in delims  (fill mode)
 *   open[i]               = two bits, as for brx_index_escaped_batch
 * Every stream starts unescaped and outside quotes, and nothing behind a stream takes part, as there.
 *   delims    HOST memory, whatever the other pointers are: n_delims bytes, 1 <= n_delims <= BRX_INDEX_SET_MAX = 8, no value twice,
 *             read before the call returns.  They travel to the kernels as launch arguments (one 64-bit word and a count) -- no
 *             upload, no table, no synchronisation -- so the call stays enqueue-only on a caller's stream.
 *   flags     BRX_INDEX_NO_QUOTE: no byte is a quote -- the `quote` argument is ignored and bit 0 of open[i] is 0.
 *             BRX_INDEX_NO_ESCAPE: no byte is an escape -- the `escape` argument is ignored and bit 1 of open[i] is 0.  Alone it is
 *             the rule of RFC 4180 (brx_index_quoted_batch with a set); both flags give a plain index of the byte set.  Other bits
 *             must be 0.  (brx_index_escaped_batch does not take BRX_INDEX_NO_ESCAPE.)
 *   what      DEVICE memory, `total` entries of one byte, bounded by `total` as pos is.  May be NULL; allowed only together with pos.
 * Check values: s = {"a":"x,\"y:}","b":[1,2]}\n{"c":"\\"}\n{"open":"[\  (48 bytes), delims "{}[]:,\n", quote '"', escape '\', flags 0:
 * pos 0 4 14 18 19 21 23 24 25 26 30 35 36 37 44, what {:,:[,]}\n{:}\n{: and open 3.  s = a,"b,c\n",d\r\ne,"f""g",h\n"x (25 bytes),
 * delims ",\n\r", quote '"': with BRX_INDEX_NO_ESCAPE pos 1 8 10 11 13 20 22 and open 1; with both flags pos 1 4 6 8 10 11 13 20 22
 * and open 0.
 * Not in scope: more than 8 delimiters; byte ranges or classes; delimiters, quotes or escapes of more than one byte (brx_find_batch
 * finds a sequence); escapes that act only inside quotes; decoding what an escape sequence means; and the three index entry points
 * above are not re-expressed over this pass's kernels: their code paths stay as they shipped.
 * Everything else is as for brx_index_escaped_batch: all other pointers are device memory; out, out_off, len, n and span as there
 * (nothing at or beyond out + span, or in front of out, is ever loaded); count mode (pos_off == NULL and pos == NULL; count required)
 * and fill mode (pos_off and pos both given; count may be NULL; `total` bounds the entries written to pos and what); `open` may be
 * NULL in either mode; hip_stream as there.  Scratch is sized as there and is a ring of 16 regions of this pass's own.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits; delims NULL; n_delims 0
 * or above 8; a value twice in delims; without BRX_INDEX_NO_ESCAPE a delimiter equal to escape; without BRX_INDEX_NO_QUOTE quote equal
 * to a delimiter; with neither flag quote == escape; only one of pos_off / pos; what without pos; count NULL in count mode; then
 * n = 0 returns BRX_SUCCESS, no launch; then out_off or len NULL, span out of range.
 * Count mode is one pass over the bytes and a one-workgroup pass over the tiles, fill mode a second pass over the bytes plus 9 bytes
 * per boundary; no reference counterpart. */
#define BRX_INDEX_NO_ESCAPE 2u /* brx_index_set_batch only */
#define BRX_INDEX_SET_MAX 8u
int brx_index_set_batch(brx_ctx *ctx, const uint8_t *delims, uint32_t n_delims, uint8_t quote, uint8_t escape, uint32_t flags,
                        const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                        uint64_t span,
                        uint64_t *count, uint32_t *open,
                        const uint64_t *pos_off, uint64_t *pos, uint8_t *what, uint64_t total,
                        void *hip_stream);

/* ---- occurrences of a byte sequence in the decoded bytes of a batch (device memory only) -----------------
 * Much delimited text does not end its records with one byte: CRLF text ("\r\n", a lone "\n" is data), blank-line separated records
 * ("\n\n"), HTTP, WARC and MIME header blocks ("\r\n\r\n"), markup terminators ("</doc>\n"), multi-byte UTF-8 separators (U+2028 is
 * e2 80 a8).  This pass finds a byte sequence, the needle p[0 .. m) with m = needle_len, 1 <= m <= 16.  Stream i is
 * s = out[out_off[i] .. out_off[i] + len[i]).
 *   an OCCURRENCE is an offset j with j + m <= len[i] and s[j + k] == p[k] for all k < m
 *   count[i]              = number of occurrences in stream i                                                    for i < n
 *   pos[pos_off[i] + k]   = offset WITHIN stream i of the first byte of its k-th occurrence, ascending in k      (fill mode)
 * ALL occurrences are reported, overlapping ones included: "aa" in "aaa" occurs at 0 and 1.  For a needle that does not overlap
 * itself ("\r\n", "</doc>") these are exactly the non-overlapping ones; for one that does ("\n\n") the consumer takes every
 * occurrence that starts at least m behind the one it took last.  No byte outside the stream ever takes part in a match: not the
 * bytes in front of it in its slot, not the slack behind it, not a neighbouring stream that starts where this one ends.  A stream
 * shorter than m has no occurrence.  With m = 1 the results equal those of brx_index_batch(delim = p[0]).
 * Not in scope: needles longer than 16 bytes, several needles in one call, character classes, case folding, and leftmost
 * non-overlapping selection on the device.  For quote-aware matching with a multi-byte delimiter use brx_index_quoted_batch and trim.
 *   needle    HOST memory, whatever the other pointers are: needle_len bytes, read before the call returns (the caller may reuse the
 *             buffer at once).  They travel to the kernels as launch arguments -- no upload, no table, no synchronisation -- so the
 *             call stays enqueue-only on a caller's stream.
 * Everything else is as for brx_index_batch: out, out_off, len, count, pos_off and pos are DEVICE pointers; out, out_off, len, n and
 * span as there (nothing at or beyond out + span, or in front of out, is ever loaded); count mode (pos_off == NULL and pos == NULL;
 * count required) and fill mode (pos_off and pos both given; count may be NULL, and if given it is written as in count mode; `total`
 * bounds the entries written to pos); hip_stream NULL = the context's own stream and the call returns when the results are there,
 * otherwise it is enqueued.  The context's lock is held to enqueue only.  Scratch (tile prefix sums, per-tile counts, two ticket
 * counters) belongs to the context and is sized from n and span with no length read back; every launch has a region of its own (a
 * ring of 16, separate from the index passes'), so calls on different HIP streams of one context may overlap; a call with a larger n
 * or span than any before synchronises the device once to grow it, and the 17th call in flight waits on the host for the first.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order: ctx NULL, needle NULL, needle_len 0 or above 16, only one of pos_off / pos, count
 * NULL in count mode; then n = 0 returns BRX_SUCCESS, no launch; then out_off or len NULL, span out of range.
 * Count mode is one pass over the bytes (reads sum(len) and 16 bytes more per 64 KiB tile, writes 8 n), fill mode two plus 8 bytes
 * per occurrence; no reference counterpart. */
int brx_find_batch(brx_ctx *ctx, const uint8_t *needle, uint32_t needle_len,
                   const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n,
                   uint64_t span,
                   uint64_t *count,
                   const uint64_t *pos_off, uint64_t *pos, uint64_t total,
                   void *hip_stream);

/* ---- selected records of the decoded bytes of a batch, as lengths or as bytes (device memory only) --------
 * The five passes above end at pos[], a list of offsets; what every consumer does next is take records: a data loader draws a
 * shuffled sample and wants it packed back to back, a tokenizer wants every line in a fixed-stride row, a writer wants the batch
 * without delimiters and without CRs.  This pass is that step: it takes the positions of any of the five passes plus a SELECTION of
 * (stream, record) pairs and returns the records' lengths (size mode) or copies their bytes into a destination (fill mode).
 * out, out_off, len, n and span are exactly as for brx_index_batch; nothing at or beyond out + span, or in front of out, is ever
 * loaded.  count (n entries), pos_off (n entries, the exclusive prefix sum of count) and pos are what a fill-mode call of any of the
 * five passes left behind, n_pos the number of entries pos holds.  All pointers are DEVICE memory.
 * THE RULE.  Stream i is s = out[out_off[i] .. out_off[i] + len[i]); D = delim_len, 1 for the four index passes and needle_len for
 * brx_find_batch, 1 <= D <= BRX_TAKE_MAX_DELIM = 16.  For 0 <= k < count[i]
 *   P(i,k) = min(pos[pos_off[i] + k], len[i])  if pos_off[i] + k < n_pos,   else len[i] (pos is not loaded then)
 * Record k of stream i exists for 0 <= k <= count[i]; record count[i] is the TRAILING one without a delimiter, empty when the stream
 * ends on a delimiter.
 *   start = 0 if k = 0, else min(P(i,k-1) + D, len[i])
 *   end   = min(P(i,k) + D, len[i]) if k < count[i], else len[i]                       (no flags: the delimiter is part of the record)
 *   end   = P(i,k)                  if k < count[i], else len[i]                       (BRX_TAKE_NO_DELIM)
 *   end   = max(end, start)
 *   BRX_TAKE_TRIM_CR: if end > start and s[end - 1] == 0x0D then end -= 1              (once; the trailing record too)
 *   L     = end - start
 * The clamps are part of the contract: stale, decreasing or garbage positions -- and the overlapping occurrences of a needle that
 * overlaps itself -- yield short or empty records, never a load outside the stream and never a negative length.
 * SELECTION.  Pairs mode (sel_stream and sel_rec both given, m entries each): entry j is record sel_rec[j] of stream sel_stream[j];
 * with sel_stream[j] >= n or sel_rec[j] > count[sel_stream[j]] the entry selects nothing (L = 0).  Any order; a record may be named
 * more than once.  All-records mode (both NULL): entry j is record j - (pos_off[i] + i) of stream i, the last stream with
 * pos_off[i] + i <= j (every stream has count[i] + 1 records, so these keys are strictly increasing); an entry whose record index
 * comes out above count[i] selects nothing; a consistent caller passes m = sum(count) + n.
 * SIZE MODE (dst_off == NULL and dst == NULL; rec_len required): rec_len[j] = L_j for j < m.
 * FILL MODE (dst_off and dst both given; rec_len may be NULL, and if given it is written as in size mode): dst_off has m entries and
 * is non-decreasing; the ROOM of entry j is dst_off[j+1] - dst_off[j], for the last entry total - dst_off[m-1].
 *   dst[dst_off[j] + t] = s[start_j + t]     for t < min(L_j, room_j)
 * A record's bytes beyond its room are not written, a room's bytes beyond its record are left as they were, and no byte at index >=
 * total is written.  With dst_off the exclusive prefix sum of rec_len the records come out back to back (the convention of
 * brx_compact_batch); with dst_off[j] = j * stride every record sits in a row of its own, truncated at the stride.  Both follow from
 * one rule: a destination byte belongs to the last entry whose dst_off is not behind it.  dst must not overlap the arena and needs
 * no alignment.
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued (behind an
 * index call on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.  No scratch, no
 * upload, no read back: calls on different HIP streams may overlap without limit.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits; BRX_TAKE_TRIM_CR without
 * BRX_TAKE_NO_DELIM; delim_len 0 or above 16; only one of sel_stream / sel_rec; only one of dst_off / dst; rec_len NULL in size mode;
 * then m = 0 returns BRX_SUCCESS, no launch; then out_off, len, count or pos_off NULL; pos NULL with n_pos > 0; all-records mode with
 * n = 0; span out of range (and m or total beyond what one launch addresses).
 * Not in scope: decoding what a record means (unquoting, unescaping, number parsing); field selection within a record (index with
 * ',' and take fields the same way); padding values other than "left as it was".
 * Size mode reads the tables of the selected entries (and one byte per entry with BRX_TAKE_TRIM_CR) and writes 8 m; fill mode reads
 * and writes the bytes taken, one pass; no reference counterpart. */
#define BRX_TAKE_NO_DELIM 1u /* a record ends in front of its delimiter */
#define BRX_TAKE_TRIM_CR  2u /* only with BRX_TAKE_NO_DELIM: then one trailing 0x0D is dropped as well */
#define BRX_TAKE_MAX_DELIM 16u
int brx_take_batch(brx_ctx *ctx,
                   const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                   const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos,
                   uint32_t delim_len, uint32_t flags,
                   const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                   uint64_t *rec_len,
                   const uint64_t *dst_off, uint8_t *dst, uint64_t total,
                   void *hip_stream);

/* ---- a 64-bit key of every selected record of the decoded bytes of a batch (device memory only) -----------
 * What a consumer does with records is nearly always keyed on their content: exact de-duplication, hash partitioning (key % G),
 * joins and membership tests.  This pass is the verb between "index" and "take": hash[j] is a 64-bit key of the bytes of entry j,
 * and with it torch.unique / a sort gives the distinct records and brx_take_batch in pairs mode gathers exactly the survivors,
 * without the bytes ever being copied in between.
 * Every argument up to m means word for word what it means for brx_take_batch: the arena (out, out_off, len, n, span), the
 * positions (count, pos_off, pos, n_pos), delim_len, THE RULE with all its clamps, the flags BRX_TAKE_NO_DELIM / BRX_TAKE_TRIM_CR
 * (BRX_TAKE_TRIM_CR only with BRX_TAKE_NO_DELIM), pairs mode and all-records mode.  An entry that selects nothing is the empty
 * record.  All pointers are DEVICE memory.  hash (m entries) is required; rec_len (m entries) is optional and, if given, is written
 * exactly as the size mode of brx_take_batch writes it.  Nothing at or beyond out + span, or in front of out, is ever loaded.
 * THE HASH, fixed here so that a CPU can reproduce it.  Arithmetic on non-negative integers, p = 2^61 - 1.
 *   mix(x), on 64-bit words: x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *           (the splitmix64 finalizer: a bijection, mix(0) = 0)
 *   K(seed) = 2 + mix((seed + 0x9E3779B97F4A7C15) mod 2^64) mod (p - 3)
 * For a record r[0 .. L):  U = ceil(L / 4);  c_u = the little-endian 32-bit word of r[4u .. 4u + 4), bytes at or behind L taken as 0
 * (where those bytes lie outside the record's stream they are never loaded);
 *   h(r)  = ( L + sum_{u < U} c_u * K^(U - u) ) mod p,  in [0, p)
 *   hash  = mix(h(r))
 * The empty record hashes to 0.
 * Equal records (same bytes, same length) get equal hashes under one seed, wherever they lie and at whatever alignment.  Two
 * different records of at most Lmax bytes collide with probability at most ceil(Lmax / 4) / p over the choice of seed: they are
 * different polynomials in K of degree at most ceil(Lmax / 4), because the constant term carries L (and mix is a bijection).  For a
 * batch of 14.8 M records of at most 128 bytes (4096 x alice29 by lines) the bound over all 1.1e14 pairs is 1.1e14 * 32 / 2.3e18 =
 * 1.5e-3 that ANY two different records share a key; a caller that needs more calls twice with two seeds (122 bits, 2e-20 for
 * that batch) or confirms with the bytes.  The hash is not cryptographic -- whoever knows the seed can construct collisions -- and
 * it is not stable across different seeds.
 * Composition law (the kernel relies on it; so may a caller who joins keys of pieces): with S(r) = h(r) - L and A a whole number
 * of words,  S(A || B) = S(A) * K^(U_B) + S(B)  (mod p).
 * Check values (hash; K first):
 *   seed 0:        K = 0x220a8397b1dcdcd    "a" 0xba350051cabf3ed3   "a\0" 0xbb6016563a245eba   "abcd" 0xada6cd48c13c1c39
 *                  "abcde" 0xf35fc97551548103   "hello, world\n" 0x0be5baf8a63cf33d   bytes 0..255 0x5bb278495e403ce2
 *                  before mix: h("a") = 0x0e5fbdc7a64afab4, h("abcd") = 0x1117ffd3c0071df7
 *   seed 1:        K = 0x110a2dec89025cd3   "a" 0x4d210b0efb807995   "a\0" 0x201b4b401d4bfd95   "abcd" 0x48e414395e8656fd
 *                  "abcde" 0x78061f9a959b2150   "hello, world\n" 0x6879e40593ee90c8   bytes 0..255 0x4540b5719777dafd
 *   seed 2^64 - 1: K = 0x4d971771b652c3e    "a" 0xc98a66ada32c9c2d   "abcd" 0x5032cab1b617812b
 *                  "hello, world\n" 0x4e8c2d5bfbc9d732   bytes 0..255 0x0bc6190075701881
 * With count all zero, n_pos = 0, all-records mode and m = n, entry i is the whole of stream i: whole-stream keys need no other call.
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued (behind an
 * index call on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.  No scratch, no
 * upload, no read back: calls on different HIP streams may overlap without limit.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits; BRX_TAKE_TRIM_CR without
 * BRX_TAKE_NO_DELIM; delim_len 0 or above 16; only one of sel_stream / sel_rec; hash NULL; then m = 0 returns BRX_SUCCESS, no
 * launch; then out_off, len, count or pos_off NULL; pos NULL with n_pos > 0; all-records mode with n = 0; span out of range (and m
 * beyond what one launch addresses).
 * Not in scope: other hash functions (xxHash, FNV, a CRC per record, whose 32 bits are too few for de-duplication); case folding or
 * normalisation before hashing; the de-duplication itself (torch.unique or a sort over the keys); hashing fields within records
 * (index with ',' and hash those the same way).
 * Reads the tables of the selected entries and every byte of their records once, writes 8 m (16 m with rec_len); one launch; no
 * reference counterpart. */
int brx_hash_batch(brx_ctx *ctx,
                   const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                   const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos,
                   uint32_t delim_len, uint32_t flags,
                   const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                   uint64_t seed,
                   uint64_t *hash, uint64_t *rec_len,
                   void *hip_stream);

/* ---- every selected record of the decoded bytes of a batch as a 64-bit number (device memory only) --------
 * With delims = ",\n" every field of a table is a record, and most fields of a table or a log are numbers.  This pass is the step
 * behind "index": val[j] is the number that entry j of a selection spells and status[j] says whether it spelled one, straight from
 * the arena -- no bytes gathered, nothing read back, and all of it exact integer arithmetic that a CPU reproduces bit for bit.
 * Every argument up to m means word for word what it means for brx_take_batch / brx_hash_batch: the arena (out, out_off, len, n,
 * span), the positions (count, pos_off, pos, n_pos), delim_len, THE RULE with all its clamps, the flags BRX_TAKE_NO_DELIM /
 * BRX_TAKE_TRIM_CR (BRX_TAKE_TRIM_CR only with BRX_TAKE_NO_DELIM), pairs mode and all-records mode.  An entry that selects nothing
 * is the empty record.  All pointers are DEVICE memory.  val and status (m entries each) are both required.  Nothing at or beyond
 * out + span, or in front of out, is ever loaded.
 * Two more bits of the same flags word: BRX_PARSE_SPACES, BRX_PARSE_QUOTED.  kind: BRX_PARSE_INT, BRX_PARSE_DEC, BRX_PARSE_HEX.
 * scale: 0 .. BRX_PARSE_MAX_SCALE = 18 for BRX_PARSE_DEC, 0 for the other two.  status[j] is one of BRX_PARSE_OK .. BRX_PARSE_LONG.
 * THE PARSE, for the record r[0 .. L) that the rule gives (after BRX_TAKE_TRIM_CR):
 *   1. L > BRX_PARSE_MAX_LEN = 64: LONG, val = 0.  None of the record's bytes is loaded (beyond the one BRX_TAKE_TRIM_CR looks at):
 *      every entry's work is bounded, and whole streams as records are harmless.
 *   2. With BRX_PARSE_SPACES: leading and trailing bytes 0x20 and 0x09 are dropped.
 *   3. With BRX_PARSE_QUOTED: if at least 2 bytes remain and the first and the last both equal `quote`, both are dropped -- once;
 *      spaces inside the quotes are not dropped.  Without the flag `quote` is ignored.
 *   4. What remains is t[0 .. T).  T = 0: EMPTY, val = 0 (a missing value, distinct from BAD).
 *   5. Grammar, matched against all of t, D = 0-9, H = 0-9a-fA-F:
 *        INT  [+-]? D+          DEC  [+-]? ( D+ ( '.' D* )? | '.' D+ )          HEX  ( '0' [xX] )? H+
 *      No exponent, no digit separators, no inf / nan.  A mismatch: BAD, val = 0.
 *   6. INT / DEC: with I the integer digits (none: 0) and F the fraction digits, V = sign * (I followed by the first `scale` digits of
 *      F, padded with '0' up to `scale` digits) read as a decimal integer of unbounded size: x * 10^scale truncated toward zero.
 *      V > 2^63 - 1: RANGE, val = INT64_MAX.  V < -2^63: RANGE, val = INT64_MIN.  Otherwise val = V, and the status is INEXACT if
 *      any digit of F behind the first `scale` is not '0', else OK.  RANGE wins over INEXACT.  Any number of leading zeros is
 *      allowed (the bound is the 64 bytes, not a digit count); -0 is 0.
 *   7. HEX: V = the value of the H digits.  V >= 2^64: RANGE, val = all ones.  Otherwise val = the 64-bit pattern of V, OK.  No sign.
 * Check values, val / status, MAX = 9223372036854775807, MIN = -9223372036854775808:
 *   INT:  "0" 0 / OK   "-0" 0 / OK   "+17" 17 / OK   "9223372036854775807" MAX / OK   "9223372036854775808" MAX / RANGE
 *         "-9223372036854775808" MIN / OK   "-9223372036854775809" MIN / RANGE   45 zeros + "9223372036854775807" (64 bytes) MAX / OK
 *         the same with 46 zeros (65 bytes) 0 / LONG   "12.5" 0 / BAD   "" 0 / EMPTY   "-" 0 / BAD   "1 " 0 / BAD
 *   DEC, scale 2:  "12.34" 1234 / OK   "12.345" 1234 / INEXACT   "12.340" 1234 / OK   "-.5" -50 / OK   "5." 500 / OK   "." 0 / BAD
 *         "-0.009" 0 / INEXACT   "1e3" 0 / BAD   "92233720368547758.07" MAX / OK   "92233720368547758.08" MAX / RANGE
 *         "-92233720368547758.089" MIN / INEXACT
 *   DEC, scale 0:  "12.5" 12 / INEXACT.      DEC, scale 18:  "9.223372036854775807" MAX / OK   "9.3" MAX / RANGE
 *   HEX:  "ff" 255 / OK   "0xFFFFFFFFFFFFFFFF" all ones / OK   "0x10000000000000000" all ones / RANGE   "0x" 0 / BAD   "x1" 0 / BAD
 *         "0X0000000000000000000000001f" 31 / OK
 *   INT with BRX_PARSE_SPACES | BRX_PARSE_QUOTED, quote '"' (the text between the brackets):
 *         [ "42"\t] 42 / OK   [" 42"] 0 / BAD   ["42] 0 / BAD   ["] 0 / BAD   [""] 0 / EMPTY   [two spaces] 0 / EMPTY
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued (behind an
 * index call on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.  No scratch, no
 * upload, no read back, one launch: calls on different HIP streams may overlap without limit.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits; BRX_TAKE_TRIM_CR without
 * BRX_TAKE_NO_DELIM; delim_len 0 or above 16; only one of sel_stream / sel_rec; kind above 2; scale above 18, or non-zero with
 * BRX_PARSE_INT / BRX_PARSE_HEX; val or status NULL; then m = 0 returns BRX_SUCCESS, no launch; then out_off, len, count or pos_off
 * NULL; pos NULL with n_pos > 0; all-records mode with n = 0; span out of range (and m beyond what one launch addresses).
 * Not in scope: binary floating point (a correctly rounded double needs a power-of-ten table and a slow path: the named follow-up;
 * BRX_PARSE_DEC with a scale is the exact substitute); exponents, thousands separators, locale decimal commas; dates and times (brx_parse_time_batch below);
 * unescaping; records above 64 bytes.  (The follow-up is brx_parse_f64_batch below: doubles, with exponents, as a call of its own.)
 * Reads the tables of the selected entries and every byte of their records of at most 64 bytes once, writes 9 m; one launch; no
 * reference counterpart. */
#define BRX_PARSE_SPACES 16u /* leading and trailing 0x20 / 0x09 are dropped */
#define BRX_PARSE_QUOTED 32u /* then one pair of enclosing `quote` bytes is dropped */
#define BRX_PARSE_INT 0u
#define BRX_PARSE_DEC 1u
#define BRX_PARSE_HEX 2u
#define BRX_PARSE_MAX_SCALE 18u
#define BRX_PARSE_MAX_LEN 64u
#define BRX_PARSE_OK      0u
#define BRX_PARSE_INEXACT 1u /* DEC: a non-zero digit behind the first `scale` fraction digits was cut off */
#define BRX_PARSE_EMPTY   2u /* nothing to parse: a missing value */
#define BRX_PARSE_RANGE   3u /* a number, but outside 64 bits: val is the nearest bound */
#define BRX_PARSE_BAD     4u /* not a number of this kind */
#define BRX_PARSE_LONG    5u /* a record above BRX_PARSE_MAX_LEN bytes: not looked at */
int brx_parse_batch(brx_ctx *ctx,
                    const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                    const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos,
                    uint32_t delim_len, uint32_t flags,
                    const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                    uint32_t kind, uint32_t scale, uint8_t quote,
                    int64_t *val, uint8_t *status,
                    void *hip_stream);

/* ---- every selected record of the decoded bytes of a batch as a correctly rounded double (device memory only) --------
 * The numeric columns that brx_parse_batch stops short of: "3.25", "1e-7", "6.02E23".  val[j] is the binary64 that entry j of a
 * selection spells and status[j] says whether it spelled one, straight from the arena -- no bytes gathered, nothing read back, integer
 * arithmetic only, so that a CPU reproduces every bit and every status.
 * Every argument up to m means word for word what it means for brx_take_batch / brx_hash_batch / brx_parse_batch: the arena (out,
 * out_off, len, n, span), the positions (count, pos_off, pos, n_pos), delim_len, THE RULE with all its clamps, the flags
 * BRX_TAKE_NO_DELIM / BRX_TAKE_TRIM_CR (BRX_TAKE_TRIM_CR only with BRX_TAKE_NO_DELIM), pairs mode and all-records mode.  An entry that
 * selects nothing is the empty record.  All pointers are DEVICE memory.  val and status (m entries each) are both required.  Nothing
 * at or beyond out + span, or in front of out, is ever loaded.
 * Three more bits of the same flags word: BRX_PARSE_SPACES, BRX_PARSE_QUOTED and BRX_PARSE_WORDS (this call only: brx_parse_batch
 * refuses it).  status[j] is one of BRX_PARSE_OK, _EMPTY, _RANGE, _BAD, _LONG, _HARD.  val is given below as a bit pattern; +0 is
 * 0x0000000000000000.
 * THE PARSE, F64, for the record r[0 .. L) that the rule gives (after BRX_TAKE_TRIM_CR); steps 1 - 4 are those of brx_parse_batch:
 *   1. L > BRX_PARSE_MAX_LEN = 64: LONG, val = +0.  None of the record's bytes is loaded (beyond the one BRX_TAKE_TRIM_CR looks at).
 *   2. With BRX_PARSE_SPACES: leading and trailing bytes 0x20 and 0x09 are dropped.
 *   3. With BRX_PARSE_QUOTED: if at least 2 bytes remain and the first and the last both equal `quote`, both are dropped -- once.
 *      Without the flag `quote` is ignored.
 *   4. What remains is t[0 .. T).  T = 0: EMPTY, val = +0.
 *   5. Grammar, matched against all of t, D = 0-9:   [+-]? ( D+ ( '.' D* )? | '.' D+ ) ( [eE] [+-]? D+ )?
 *      With BRX_PARSE_WORDS also [+-]? followed by nan, inf or infinity in any letter case: status OK, val = 0x7FF8000000000000 for nan,
 *      0x7FF0000000000000 for the other two, bit 63 set behind a '-'.  Without the flag those words are BAD.  No hex float, no digit
 *      separator, no locale comma.  A mismatch: BAD, val = +0.
 *   6. Value: x = the exact rational value of the text; any number of leading zeros anywhere, the exponent's digits included (the
 *      bound is the 64 bytes).  val = x rounded to binary64, round to nearest, ties to even, subnormals included, with the sign of the
 *      text: "-0" is 0x8000000000000000 (unlike INT).  An x that rounds beyond the largest finite double: +-inf, RANGE.  A non-zero x
 *      that rounds to +-0: +-0, RANGE.  Everything else OK.
 *   7. The bound on a lane's work.  s = the digits of the integer and the fraction part together, leading zeros stripped.  At most 19
 *      digits, or nothing but '0' behind the 19th: never HARD.  Otherwise w = the first 19 digits and q the power of ten with
 *      w * 10^q < |x| < (w + 1) * 10^q; a = RN(w * 10^q), b = RN((w + 1) * 10^q).  a = b: val = a under step 6's statuses (rounding
 *      is monotone).  a != b: status HARD, val = a with the text's sign; HARD wins over RANGE.  The correctly rounded result is then val
 *      or the next double away from zero, the bit pattern plus 1 (w >= 10^18, so a and b are neighbours).  The status is a function
 *      of the text alone: the caller knows exactly which entries to finish elsewhere.  Text printed with up to 17 digits never meets
 *      it; of random numbers of 20 - 40 digits about one in 600 does.
 * Check values, val (hex) / status:
 *   "0" 0000000000000000 / OK   "-0" 8000000000000000 / OK   "1" 3FF0000000000000 / OK   "-1.5" BFF8000000000000 / OK
 *   "0.1" 3FB999999999999A / OK   ".5" 3FE0000000000000 / OK   "5." 4014000000000000 / OK   "1e23" 44B52D02C7E14AF6 / OK
 *   "1E+2" 4059000000000000 / OK   "1e-2" 3F847AE147AE147B / OK   "9007199254740993" 4340000000000000 / OK
 *   "9007199254740995" 4340000000000002 / OK   "1.7976931348623157e308" 7FEFFFFFFFFFFFFF / OK
 *   "1.7976931348623158e308" 7FEFFFFFFFFFFFFF / OK   "1.7976931348623159e308" 7FF0000000000000 / RANGE
 *   "-1e309" FFF0000000000000 / RANGE   "4.9e-324" 0000000000000001 / OK   "2.4703282292062328e-324" 0000000000000001 / OK
 *   "2.4703282292062327e-324" 0000000000000000 / RANGE   "1e-400" 0000000000000000 / RANGE
 *   "2.2250738585072014e-308" 0010000000000000 / OK   "2.2250738585072011e-308" 000FFFFFFFFFFFFF / OK
 *   "0.1000000000000000055511151231257827" 3FB999999999999A / OK   "123456789012345678901234567890" 45F8EE90FF6C373E / OK
 *   "9007199254740993.0000000000000000" 4340000000000000 / OK   "9007199254740993.0000000000000001" 4340000000000000 / HARD
 *   "0e99999" 0000000000000000 / OK   "1e" + 59 zeros + "5" (62 bytes) 40F86A0000000000 / OK
 *   "1e" + 61 zeros + "5" (64 bytes) 40F86A0000000000 / OK
 *   63 zeros + "1" (64 bytes) 3FF0000000000000 / OK   the same with one more zero (65 bytes) 0000000000000000 / LONG
 *   "1e" 0000000000000000 / BAD   "e5" 0000000000000000 / BAD   "." 0000000000000000 / BAD   "1.2.3" 0000000000000000 / BAD
 *   "+.e1" 0000000000000000 / BAD   "0x10" 0000000000000000 / BAD   "1e+" 0000000000000000 / BAD
 *   "nan" without BRX_PARSE_WORDS 0000000000000000 / BAD   "-Infinity" with BRX_PARSE_WORDS FFF0000000000000 / OK
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued (behind an
 * index call on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.  No scratch, no
 * upload, no read back, one launch: calls on different HIP streams may overlap without limit.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits; BRX_TAKE_TRIM_CR without
 * BRX_TAKE_NO_DELIM; delim_len 0 or above 16; only one of sel_stream / sel_rec; val or status NULL; then m = 0 returns BRX_SUCCESS, no
 * launch; then out_off, len, count or pos_off NULL; pos NULL with n_pos > 0; all-records mode with n = 0; span out of range (and m
 * beyond what one launch addresses).
 * Not in scope: a slow path for HARD on the device (big-integer comparison per lane: the named follow-up); float32 output; hex float,
 * thousands separators, decimal commas; records above 64 bytes.
 * Reads the tables of the selected entries, every byte of their records of at most 64 bytes once and 16 or 32 bytes of a 10.4 KB
 * table of powers of five per number, writes 9 m; one launch; no reference counterpart. */
#define BRX_PARSE_WORDS 64u /* brx_parse_f64_batch only: [+-]? nan / inf / infinity in any letter case are values, not BAD */
#define BRX_PARSE_HARD   6u /* brx_parse_f64_batch only: more than 19 digits and too close to call; val or its successor is the answer */
int brx_parse_f64_batch(brx_ctx *ctx,
                        const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                        const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos,
                        uint32_t delim_len, uint32_t flags,
                        const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                        uint8_t quote,
                        double *val, uint8_t *status,
                        void *hip_stream);

/* ---- every selected record of the decoded bytes of a batch as a date, a time of day or a timestamp (device memory only) --------
 * The column type that brx_parse_batch and brx_parse_f64_batch both call BAD: "2024-03-10T07:08:09.123+05:30".  val[j] is the day
 * number or the instant that entry j of a selection spells, status[j] says whether it spelled one, zone[j] which offset it carried,
 * straight from the arena -- no bytes gathered, nothing read back, exact integer arithmetic that a CPU reproduces bit for bit.
 * Every argument up to m means word for word what it means for brx_take_batch / brx_hash_batch / brx_parse_batch: the arena (out,
 * out_off, len, n, span), the positions (count, pos_off, pos, n_pos), delim_len, THE RULE with all its clamps, the flags
 * BRX_TAKE_NO_DELIM / BRX_TAKE_TRIM_CR (BRX_TAKE_TRIM_CR only with BRX_TAKE_NO_DELIM), pairs mode and all-records mode.  An entry that
 * selects nothing is the empty record.  All pointers are DEVICE memory.  val and status (m entries each) are both required; zone (m
 * entries) may be NULL.  Nothing at or beyond out + span, or in front of out, is ever loaded.
 * Two more bits of the same flags word: BRX_PARSE_SPACES, BRX_PARSE_QUOTED (BRX_PARSE_WORDS and every other bit are refused).  kind:
 * BRX_TIME_DATE, BRX_TIME_TIME, BRX_TIME_STAMP.  scale: 0 .. BRX_TIME_MAX_SCALE = 9 for BRX_TIME_TIME and BRX_TIME_STAMP (0 seconds, 3
 * milliseconds, 6 microseconds, 9 nanoseconds), 0 for BRX_TIME_DATE.  status[j] is one of BRX_PARSE_OK, _INEXACT, _EMPTY, _RANGE, _BAD,
 * _LONG: there is no new status value.
 * THE PARSE, TIME, for the record r[0 .. L) that the rule gives (after BRX_TAKE_TRIM_CR):
 *   1. L > BRX_PARSE_MAX_LEN = 64: LONG, val = 0.  None of the record's bytes is loaded (beyond the one BRX_TAKE_TRIM_CR looks at).
 *   2. With BRX_PARSE_SPACES: leading and trailing bytes 0x20 and 0x09 are dropped.
 *   3. With BRX_PARSE_QUOTED: if at least 2 bytes remain and the first and the last both equal `quote`, both are dropped -- once.
 *      Without the flag `quote` is ignored.
 *   4. What remains is t[0 .. T).  T = 0: EMPTY, val = 0.
 *   5. Grammar, matched against all of t, D = 0-9:
 *        date = DDDD '-' DD '-' DD                      (the year has exactly four digits, 0000 .. 9999)
 *        time = DD ':' DD ( ':' DD ( [.,] D+ )? )?
 *        zone = [Zz] | [+-] DD ':' DD | [+-] DDDD | [+-] DD
 *        DATE: date        TIME: time        STAMP: date ( [Tt ] time zone? )?
 *      A date alone is midnight.  A comma is accepted as the decimal mark because Python's logging default prints one.  A mismatch:
 *      BAD, val = 0.
 *   6. Field ranges; a violation is BAD.  Month 01 .. 12.  Day 01 .. the month's length in the proleptic Gregorian calendar: year y is
 *      leap iff y % 4 == 0 and (y % 100 != 0 or y % 400 == 0); year 0000 is leap.  Hour 00 .. 23, minute 00 .. 59, second 00 .. 59.
 *      Zone hours 00 .. 23, zone minutes 00 .. 59.  There is no 24:00 and no second 60.
 *   7. Value.  days = days from 1970-01-01 to the date, 0 for TIME.  off = the zone's offset in seconds east of UTC, 0 for Z, for no
 *      zone and for -00:00.  secs = days * 86400 + hh * 3600 + mm * 60 + ss - off.  With F the fraction digits (none: empty):
 *      V = secs * 10^scale + (the first `scale` digits of F, padded with '0' up to `scale` digits, read as an integer): the instant in
 *      units of 10^-scale s, rounded toward minus infinity.  DATE: scale must be 0 and V = days.
 *      V > 2^63 - 1: RANGE, val = INT64_MAX.  V < -2^63: RANGE, val = INT64_MIN.  Otherwise val = V, and the status is INEXACT if a
 *      digit of F behind the first `scale` is not '0', else OK.  RANGE wins over INEXACT.  Only scales 8 and 9 can reach RANGE within
 *      years 0000 .. 9999.
 *   8. zone[j], if given: the offset in minutes east of UTC, -1439 .. 1439, when the status is OK or INEXACT and the text carried a
 *      zone (Z is 0); BRX_TIME_NO_ZONE in every other case: no zone in the text, DATE, TIME, and every other status.  The caller can
 *      tell naive stamps from aware ones and can rebuild the wall-clock time.
 * Check values, val / status, MAX = 9223372036854775807, MIN = -9223372036854775808:
 *   DATE:  "1970-01-01" 0 / OK   "1969-12-31" -1 / OK   "0000-01-01" -719528 / OK   "0000-02-29" -719469 / OK
 *         "2000-02-29" 11016 / OK   "9999-12-31" 2932896 / OK   "1900-02-29" 0 / BAD   "2100-02-29" 0 / BAD   "2024-02-30" 0 / BAD
 *         "2023-04-31" 0 / BAD   "2023-00-10" 0 / BAD   "2023-13-01" 0 / BAD   "2023-01-00" 0 / BAD   "2023-1-01" 0 / BAD
 *         "20230101" 0 / BAD   "+2023-01-01" 0 / BAD   "2023-01-01T00:00" 0 / BAD   "" 0 / EMPTY
 *   TIME, scale 0:  "00:00" 0 / OK   "23:59:59" 86399 / OK   "24:00:00" 0 / BAD   "12:60" 0 / BAD   "23:59:60" 0 / BAD
 *         "12:34:56." 0 / BAD   "12:34.5" 0 / BAD   "12:34:56Z" 0 / BAD   "1:02:03" 0 / BAD
 *   TIME, scale 3:  "12:34:56.789" 45296789 / OK   "12:34:56,7891" 45296789 / INEXACT
 *   TIME, scale 9:  "23:59:59.999999999" 86399999999999 / OK
 *   STAMP, scale 0:  "1970-01-01T00:00:00Z" 0 / OK   "2024-03-10" 1710028800 / OK   "2024-03-10 07:08" 1710054480 / OK
 *         "2024-03-10T07:08Z" 1710054480 / OK   "2024-03-10t07:08:09z" 1710054489 / OK
 *         "2024-03-10T07:08:09-0800" 1710083289 / OK, zone -480   "2024-03-10T07:08:09+01" 1710050889 / OK, zone 60
 *         "2024-03-10T07:08:09-00:00" 1710054489 / OK, zone 0   "1969-12-31T23:59:59.5Z" -1 / INEXACT
 *         "0000-01-01T00:00:00+23:59" -62167305540 / OK   "9999-12-31T23:59:59-23:59" 253402387139 / OK
 *         "2024-03-10T07:08:09+24:00" 0 / BAD   "2024-03-10T07:08:09+05:60" 0 / BAD   "2024-03-10T07:08:09+5" 0 / BAD
 *         "2024-03-10T07:08:09+05:3" 0 / BAD   "2024-03-10T07:08:09 Z" 0 / BAD   "2024-03-10T07:08:60Z" 0 / BAD
 *         "2024-03-10T24:00:00Z" 0 / BAD   "2024-03-10T07:08:09.Z" 0 / BAD   "2024-03-10T07Z" 0 / BAD   "2024-03-10T" 0 / BAD
 *         "2024-02-30T00:00:00Z" 0 / BAD   "2024-03-10_07:08:09" 0 / BAD   "2024-03-10T07:08:09ZZ" 0 / BAD
 *   STAMP, scale 3:  "2024-03-10 07:08:09,123" 1710054489123 / OK, zone BRX_TIME_NO_ZONE   "2024-03-10T07:08:09.1239" 1710054489123 / INEXACT
 *         "1969-12-31T23:59:59.5Z" -500 / OK   "2024-03-10T07:08:09." + 38 zeros + "+05:30" (64 bytes) 1710034689000 / OK
 *         the same with 39 zeros (65 bytes) 0 / LONG   "2024-03-10T07:08:09.123" + 40 zeros + "1" (64 bytes) 1710054489123 / INEXACT
 *   STAMP, scale 6:  "2024-03-10T07:08:09.5+05:30" 1710034689500000 / OK, zone 330
 *   STAMP, scale 9:  "2262-04-11T23:47:16.854775807Z" MAX / OK   "2262-04-11T23:47:16.854775808Z" MAX / RANGE
 *         "2262-04-11T23:47:16.8547758079Z" MAX / INEXACT   "1677-09-21T00:12:43.145224192Z" MIN / OK
 *         "1677-09-21T00:12:43.145224191Z" MIN / RANGE   "1677-09-21T00:12:43.1452241919Z" MIN / RANGE
 *         "9999-12-31T23:59:59Z" MAX / RANGE   "0000-01-01T00:00:00Z" MIN / RANGE
 *   STAMP, scale 0, with BRX_PARSE_SPACES | BRX_PARSE_QUOTED, quote '"' (the text between the brackets):
 *         [ "2024-03-10T07:08:09Z"\t] 1710054489 / OK   [" 2024-03-10"] 0 / BAD   [""] 0 / EMPTY
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued (behind an
 * index call on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.  No scratch, no
 * upload, no read back, one launch: calls on different HIP streams may overlap without limit.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits (64 is one of them);
 * BRX_TAKE_TRIM_CR without BRX_TAKE_NO_DELIM; delim_len 0 or above 16; only one of sel_stream / sel_rec; kind above 2; scale above 9, or
 * non-zero with BRX_TIME_DATE; val or status NULL; then m = 0 returns BRX_SUCCESS, no launch; then out_off, len, count or pos_off
 * NULL; pos NULL with n_pos > 0; all-records mode with n = 0; span out of range (and m beyond what one launch addresses).
 * Not in scope: the basic format without separators, week dates and ordinal dates; years outside 0000 .. 9999, expanded or signed
 * years; month names (RFC 2822, Common Log Format); 12-hour clocks; zone names and DST rules; leap seconds and 24:00; durations and
 * intervals; records above 64 bytes.
 * Reads the tables of the selected entries and every byte of their records of at most 64 bytes once, writes 9 m (11 m with zone); one
 * launch; no reference counterpart. */
#define BRX_TIME_DATE  0u /* DDDD-DD-DD: val = days since 1970-01-01 */
#define BRX_TIME_TIME  1u /* DD:DD[:DD[.D+]]: val = units of 10^-scale s since midnight */
#define BRX_TIME_STAMP 2u /* date, then optionally a time and a zone: val = units of 10^-scale s since 1970-01-01T00:00:00Z */
#define BRX_TIME_MAX_SCALE 9u
#define BRX_TIME_NO_ZONE (-32768) /* zone[j] where no offset is reported */
int brx_parse_time_batch(brx_ctx *ctx,
                         const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                         const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos,
                         uint32_t delim_len, uint32_t flags,
                         const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                         uint32_t kind, uint32_t scale, uint8_t quote,
                         int64_t *val, uint8_t *status, int16_t *zone,
                         void *hip_stream);

/* ---- selected records of the decoded bytes of a batch as the strings they spell (device memory only) -----------
 * The column type that is left: strings.  brx_take_batch copies a record's bytes as they stand, so the "text": "..." of a JSON Lines
 * row still carries its \n, \" and \uXXXX, and a CSV field its "" -- this call resolves them on the device: u_j is the string that
 * entry j of a selection spells, status[j] says how it was written, straight from the arena into a destination.
 * Every argument up to m means word for word what it means for brx_take_batch / brx_hash_batch / brx_parse_batch: the arena (out,
 * out_off, len, n, span), the positions (count, pos_off, pos, n_pos), delim_len, THE RULE with all its clamps, the flags
 * BRX_TAKE_NO_DELIM / BRX_TAKE_TRIM_CR (BRX_TAKE_TRIM_CR only with BRX_TAKE_NO_DELIM), pairs mode and all-records mode.  An entry that
 * selects nothing is the empty record.  All pointers are DEVICE memory.  One more bit of the same flags word: BRX_PARSE_SPACES; every
 * other bit is refused.  dialect: BRX_TEXT_CSV, BRX_TEXT_JSON, BRX_TEXT_BACKSLASH; quote and escape are byte values (q, e below).
 * dst_off, dst, total and the ROOM of an entry are exactly those of brx_take_batch's fill mode.  Nothing at or beyond out + span, or
 * in front of out, is ever loaded; in fact no byte outside an entry's record is: the look-ahead of an escape ends at the record's end,
 * whatever follows it in the arena is never loaded.
 * SIZE MODE (dst_off == NULL and dst == NULL; text_len and status required): text_len[j] = L'_j, the length of u_j, and status[j].
 * FILL MODE (dst_off and dst both given; text_len and status may each be NULL, and if given they are written as in size mode):
 *   dst[dst_off[j] + t] = u_j[t]     for t < min(L'_j, room_j)
 * A room's bytes behind its text are left as they were, and no byte at index >= total is written.  A text cut by its room is cut at
 * the byte: that may be inside a UTF-8 sequence (the caller sees it from text_len[j] > room_j).
 * L' <= T <= L holds in every case, so a caller may size the rooms from brx_take_batch's rec_len (or use one stride that holds the
 * longest record) without a size-mode call.
 * THE TEXT, for the record r[0 .. L) that the rule gives (after BRX_TAKE_TRIM_CR).  With BRX_PARSE_SPACES leading and trailing bytes
 * 0x20 and 0x09 are dropped first; what remains is t[0 .. T).  Every output is defined, also for malformed input: BAD means
 * "malformed somewhere; the text is what the walk below emitted".
 *   BRX_TEXT_CSV (RFC 4180; e is ignored).  T = 0 or t[0] != q: BARE, u = t (so an unquoted empty field and "" are told apart).
 *     t[0] = q and (T < 2 or t[T-1] != q): BAD, u = t.  Otherwise walk the body t[1 .. T-1) from the left: a q followed by a q inside
 *     the body emits one q and skips both; a q otherwise emits q and sets BAD; any other byte is emitted.  OK unless BAD was set.
 *   BRX_TEXT_JSON (q != e required).  T = 0 or t[0] != q: BARE, u = t (null, numbers and true come out this way).  Otherwise walk from
 *     i = 1.  At e that is the last byte of t: emit e, BAD, advance 1.  At e with c = t[i+1]: c is q, e or '/': emit c, advance 2;
 *     c is b f n r t: emit 08 0C 0A 0D 09, advance 2; c is u and t[i+2 .. i+6) lies inside t and is four hex digits of either case,
 *     a code unit cu: not a surrogate: emit its UTF-8 (1 to 3 bytes; \u0000 emits one zero byte), advance 6; cu in D800..DBFF and
 *     t[i+6 .. i+12) lies inside t and is e, u and four hex digits of a code unit in DC00..DFFF: emit the 4 UTF-8 bytes of the
 *     pair, advance 12; any other surrogate: emit EF BF BD, BAD, advance 6.  Anything else (unknown letter, short or non-hex \u): emit
 *     e, BAD, advance 1.  At q: if i = T-1 it is the closing quote and the walk ends, otherwise emit q, BAD, advance 1.  Any other byte
 *     is emitted: raw control bytes and the UTF-8 of the raw bytes pass unchecked.  A walk that reaches T without the closing quote
 *     sets BAD.  The tests on c are made in this order (it matters only for odd choices of q and e).
 *   BRX_TEXT_BACKSLASH (PostgreSQL COPY text, MySQL tab dumps; q is ignored, no quoting).  t is exactly e 'N': NULL, L' = 0.
 *     Otherwise walk from 0: e as the last byte: emit e, BAD; e followed by b f n r t v 0: emit 08 0C 0A 0D 09 0B 00; e followed by
 *     any other byte c: emit c (e itself, a delimiter, a quote); any other byte is emitted.  Never BARE.
 * Check values, q = '"', e = '\', record and text between brackets, text bytes in hex where they are not printable:
 *   JSON:  ["a\tb"] 61 09 62 / OK   ["\u00e9"] C3 A9 / OK   ["\ud83d\ude00"] F0 9F 98 80 / OK   ["\\"] 5C / OK   [""] empty / OK
 *          [null] [null] / BARE   ["\ud83d"] EF BF BD / BAD   ["\ud83d\u0041"] EF BF BD 41 / BAD   ["\ude00x"] EF BF BD 78 / BAD
 *          ["\u12"] [\u12] / BAD   ["\x"] [\x] / BAD   ["a"b"] [a"b] / BAD   ["abc\"] [abc"] / BAD   ["abc] [abc] / BAD
 *          ["] empty / BAD
 *   JSON with BRX_PARSE_SPACES:  [ "x"<09>] [x] / OK
 *   CSV:   ["a""b"] [a"b] / OK   [""""] ["] / OK   [""] empty / OK   [] empty / BARE   [abc] [abc] / BARE   ["""] ["] / BAD
 *          ["a"b"] [a"b] / BAD   ["abc] ["abc] / BAD   ["] ["] / BAD
 *   BACKSLASH:  [a\tb] 61 09 62 / OK   [\,] [,] / OK   [\\N] [\N] / OK   [x\N] [xN] / OK   [\N] empty / NULL   [a\] [a\] / BAD
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued (behind an
 * index call on the same stream it needs no synchronisation in between).  The context's lock is held to enqueue only.  No scratch, no
 * upload, no read back, one launch: calls on different HIP streams may overlap without limit.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; unknown flag bits; BRX_TAKE_TRIM_CR without
 * BRX_TAKE_NO_DELIM; delim_len 0 or above 16; only one of sel_stream / sel_rec; dialect above 2; quote or escape above 255;
 * BRX_TEXT_JSON with quote == escape; only one of dst_off / dst; text_len or status NULL in size mode; then m = 0 returns BRX_SUCCESS,
 * no launch; then out_off, len, count or pos_off NULL; pos NULL with n_pos > 0; all-records mode with n = 0; span out of range (and m
 * or total beyond what one launch addresses).
 * Not in scope: octal and \x escapes; validation of UTF-8 or of raw control bytes; JSON values other than strings (no nested
 * parsing); escapes that act only inside quotes; re-quoting; padding values other than "left as it was".
 * Reads the tables of the selected entries and the bytes of their records, writes the texts and 9 m; one launch; no reference
 * counterpart.  Two cases are computed by one lane per record, whatever its length, while the other lanes of its wavefront wait:
 * BRX_TEXT_JSON with an escape byte that is a hex digit, and, with BRX_PARSE_SPACES, the blanks around a record, which are dropped
 * byte by byte before anything else (a record of some KiB of blanks costs its wavefront a serial walk of that length). */
#define BRX_TEXT_CSV       0u
#define BRX_TEXT_JSON      1u
#define BRX_TEXT_BACKSLASH 2u
#define BRX_TEXT_OK   0u /* quoted (CSV, JSON) or plain (BACKSLASH), and well-formed */
#define BRX_TEXT_BARE 1u /* CSV, JSON: not quoted; the text is the record (after BRX_PARSE_SPACES) */
#define BRX_TEXT_NULL 2u /* BACKSLASH: the record is e 'N'; the text is empty */
#define BRX_TEXT_BAD  3u /* malformed somewhere; the text is what the walk emitted */
int brx_unescape_batch(brx_ctx *ctx,
                       const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                       const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, uint64_t n_pos,
                       uint32_t delim_len, uint32_t flags,
                       const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                       uint32_t dialect, uint32_t quote, uint32_t escape,
                       uint64_t *text_len, uint8_t *status,
                       const uint64_t *dst_off, uint8_t *dst, uint64_t total,
                       void *hip_stream);

/* ---- named members of JSON Lines objects as selections for the record calls (device memory only) -----------------
 * The record calls above take (sel_stream, sel_rec) pairs.  For JSON Lines nobody can say on the device which record holds the value
 * of "text" in line 17: keys come in any order, some are missing, values may be objects and arrays, a name may repeat inside a nested
 * value, a key may be duplicated.  This pass is the verb in front of the record calls: from `what` it emits, per line and per
 * requested name, the pair that the record calls take as they are, and the kind of value that stands there.
 * out, out_off, len, n and span are exactly as for brx_take_batch.  count, pos_off, pos, what and n_pos are what a fill-mode
 * brx_index_set_batch call left behind, with quote '"', escape '\' and a delimiter set that contains { } [ ] : , and the line feed;
 * pos_off is the exclusive prefix sum of count.
 *   names, name_len   HOST memory, whatever the other pointers are, read before the call returns.  Name q is names[32 q .. 32 q +
 *             name_len[q]); 1 <= n_names <= BRX_MEMBER_MAX_NAMES = 8, 1 <= name_len[q] <= BRX_MEMBER_MAX_NAME = 32, no name twice.  They
 *             travel to the kernels as launch arguments (8 x 32 = 256 bytes), as find's needle does: no upload, and the call stays
 *             enqueue-only.
 * Everything else is DEVICE memory.
 * THE RULE.  Boundary k of stream i is w_k = what[pos_off[i] + k], at P(i,k) with the clamps of brx_take_batch's RULE.  An index
 * pos_off[i] + k >= n_pos is not loaded, neither from what nor from pos: such a boundary counts as a neutral byte.
 *   LINES.  Line r of stream i holds the boundaries behind the r-th '\n' boundary, up to and including the (r + 1)-th.  Every stream
 *       has lines[i] = (number of '\n' boundaries) + 1 lines; the last one is the TRAILING line, empty when the stream ends on a
 *       line feed (take's convention for records).  Line r of stream i is entry j = line_off[i] + r.
 *   DEPTH.  d(k) = the sum of +1 for every '{' or '[' and -1 for every '}' or ']' among the boundaries of the same line in front of
 *       k.  It is signed and restarts at 0 behind every '\n' boundary: a malformed line cannot spoil the next.  Other bytes are neutral.
 *   MEMBER.  A ':' boundary k with d(k) == 1.  Its KEY RECORD is record k of the stream under BRX_TAKE_NO_DELIM with D = 1, leading
 *       and trailing 0x20, 0x09 and 0x0D dropped.  The member CARRIES name q iff what is left is '"', the bytes of name q, '"':
 *       bytewise, no escape is resolved.  A key record longer than BRX_MEMBER_MAX_KEY = 64 bytes before trimming is not looked at and
 *       matches nothing (parse's LONG).
 *   VALUE of the member at k.  w_{k+1} in the same line and ',' or '}': SCALAR, the value is record k + 1.  '{': OBJECT.  '[': ARRAY
 *       (for both, record k + 1 is the blank in front of the opener).  Anything else, or no further boundary in the line: BAD.  In
 *       all four cases sel_rec = k + 1.
 *   LAST WINS.  For entry (q, j) the LAST member of line j that carries name q wins, as json.loads has it with duplicates.  None:
 *       kind = MISSING and sel_rec = UINT64_MAX, which by take's pairs-mode rule selects nothing.  sel_stream is i in every case.
 *   Results are column-major: entry (q, j) is at index q * m + j, so one name's column is a contiguous selection for a record call.
 *   line_flags[j] (optional): BRX_MEMBER_LONG_KEY: a depth-1 member of the line had a key record above 64 bytes.
 *       BRX_MEMBER_ESCAPED_KEY: a depth-1 key record that was looked at contains 0x5C (it may spell a name with an escape).
 *       BRX_MEMBER_UNBALANCED: the depth fell below 0 somewhere in the line, or is not 0 behind the line's last boundary other than
 *       its '\n'.  A line with flags 0 whose members are all SCALAR or MISSING is one the caller need not look at again.
 * COUNT MODE (line_off, sel_stream, sel_rec and kind all NULL; lines required): lines[i] for i < n.
 * FILL MODE (all four given; lines may be NULL, and if given it is written as in count mode): every slot (q, j) with j < m that belongs
 * to a line is written, MISSING included; a line with j >= m is not written: m bounds the results as `total` bounds pos.  Nothing at
 * index >= n_names * m is written; line_flags, when given, for j < m only.  While the call runs, sel_rec[0 .. n_names * m) and
 * sel_stream[0 .. m) are the pass's own (cleared first, then raised); a slot j < m that is no stream's line (a line_off that is not
 * the prefix sum of lines) comes out MISSING with sel_stream = n.
 * Nothing at or beyond out + span, in front of out, outside a stream, or at or beyond what + n_pos or pos + n_pos is ever loaded.
 * Stale or garbage pos, what or count give wrong members, never a load or a store outside these bounds.
 * Check values, from the check stream of brx_index_set_batch (pos and what as printed there, count 15); stream between brackets, per
 * line the names found as name KIND sel_rec, the others MISSING:
 *   names a, b, c, open:
 *   [{"a":"x,\"y:}","b":[1,2]}\n{"c":"\\"}\n{"open":"[\] line 0: a SCALAR 2 b ARRAY 4 flags 0; line 1: c SCALAR 11 flags 0; line 2: open BAD 15 flags 4
 *   (lines = 3; record 11 is "\\")
 *   [{"a":1,"a":2}] line 0: a SCALAR 4 flags 0
 *   [{"user":{"text":1},"text":2}] line 0: text SCALAR 7 user OBJECT 2 flags 0
 *   [{ "a"<09>:1}] line 0: a SCALAR 2 flags 0
 *   [{<30 x 20>"<32 x k>":1}] line 0: k32 SCALAR 2 flags 0                    (a key record of 64 bytes; k32 = 32 x k)
 *   [{<31 x 20>"<32 x k>":1}] line 0: none flags 1                            (... of 65)
 *   [{"a":1}}] line 0: a SCALAR 2 flags 4
 *   [}{"a":1}] line 0: none flags 4
 *   [{"a\u0062":1}\n] line 0: none flags 2; line 1: none flags 0              (name ab)
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued, and behind a
 * brx_index_set_batch call on the same stream it needs no synchronisation in between.  The context's lock is held to enqueue only.
 * Scratch (tile prefix sums, lines per stream, two small records per tile of 4096 boundaries) belongs to the context and is sized from
 * n and n_pos with no count read back; every launch has a region of its own (a ring of 16 of this pass's own).
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; names or name_len NULL; n_names 0 or above
 * 8; a name_len of 0 or above 32; a name twice; only some of line_off / sel_stream / sel_rec / kind; line_flags in count mode; lines
 * NULL in count mode; then n = 0 returns BRX_SUCCESS, no launch; then out_off, len, count or pos_off NULL; pos or what NULL with
 * n_pos > 0; span, m or n_pos out of range of one launch (the bound on m keeps n_names * m in range too).
 * Not in scope: paths into nested values, and the extent of a nested value (of a nested array, with its elements: brx_elements_batch
 * below; of a nested object, with its named members: brx_object_batch below that); resolving escapes in keys; names longer than 32 bytes or
 * more than 8 names; validating JSON; pretty-printed JSON with line feeds inside an object; any change to brx_index_set_batch or to
 * the record calls.
 * Count mode reads `what` once, fill mode twice, plus the key records of the depth-1 members; no reference counterpart. */
#define BRX_MEMBER_MAX_NAMES 8u
#define BRX_MEMBER_MAX_NAME  32u
#define BRX_MEMBER_MAX_KEY   64u
#define BRX_MEMBER_MISSING 0u /* no depth-1 member of the line carries the name; sel_rec = UINT64_MAX */
#define BRX_MEMBER_SCALAR  1u /* the value is record sel_rec */
#define BRX_MEMBER_OBJECT  2u /* a nested object starts behind record sel_rec */
#define BRX_MEMBER_ARRAY   3u /* a nested array starts behind record sel_rec */
#define BRX_MEMBER_BAD     4u /* something else follows the ':' */
#define BRX_MEMBER_LONG_KEY    1u
#define BRX_MEMBER_ESCAPED_KEY 2u
#define BRX_MEMBER_UNBALANCED  4u
int brx_member_batch(brx_ctx *ctx,
                     const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                     const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, const uint8_t *what, uint64_t n_pos,
                     const uint8_t *names, const uint32_t *name_len, uint32_t n_names,
                     uint64_t *lines,
                     const uint64_t *line_off, uint64_t m,
                     uint32_t *sel_stream, uint64_t *sel_rec, uint8_t *kind, uint8_t *line_flags,
                     void *hip_stream);

/* ---- the elements of JSON arrays as selections for the record calls (device memory only) -----------------------------
 * brx_member_batch answers kind = BRX_MEMBER_ARRAY and sel_rec = the boundary of the '[' for "emb":[0.12,-3.4e-2,...], and there the
 * pipeline ended.  This pass is the verb between member and the record calls: for a selection of array openers it gives the number of
 * elements, the closing bracket (the extent of the nested value) and the (stream, record) pair and kind of every element.  The pairs
 * are a selection that the record calls take as they stand: brx_parse_f64_batch over them is the embedding matrix.
 * Everything is DEVICE memory.  out ... n_pos are exactly as for brx_member_batch: the tables of a fill-mode brx_index_set_batch call
 * at { } [ ] : , and the line feed, quote '"', escape '\'.  (sel_stream, sel_rec) is a pairs-mode selection of m entries as
 * brx_member_batch emits it: sel_rec = the boundary index of the opener.  A whole column of member's output may be passed, MISSING
 * and SCALAR entries included.
 * THE RULE.  Boundary k of stream i, w_k and C(i) = min(count[i], n_pos - pos_off[i]) (0 where pos_off[i] >= n_pos), the boundaries
 * that count, are as in brx_member_batch's RULE.  Nothing at or behind n_pos is loaded, neither from what nor from pos.  Entry j has
 * i = sel_stream[j], r = sel_rec[j].
 *   BRX_ELEMENTS_NONE.  i >= n or r >= C(i): n_elem = 0, end = UINT64_MAX.  Member's MISSING (sel_rec = UINT64_MAX) lands here.
 *   BRX_ELEMENTS_NOT_ARRAY.  w_r is not '[': n_elem = 0, end = UINT64_MAX.
 *   THE WALK.  Otherwise k = r + 1, r + 2, ... with the relative depth e = 1 and the separator s = r.  '{' and '[' give e += 1.  '}'
 *       and ']' give e -= 1; at e = 0 the array ends at k: status BRX_ELEMENTS_OK for ']', BRX_ELEMENTS_MISMATCH for '}', end = k, and
 *       the last element ends here.  A ',' at e = 1 ends an element, then s = k.  Every other byte is neutral.  A '\n' boundary stops
 *       the walk (BRX_ELEMENTS_UNCLOSED, end = k), as does k = C(i) (BRX_ELEMENTS_UNCLOSED, end = C(i)); the elements ended so far
 *       stand, the partial one behind the last separator is not an element.
 *   AN ELEMENT that begins behind separator s has el_rec = s + 1 and el_stream = i.  Its kind follows from w_{s+1}: ',' ']' '}':
 *       BRX_MEMBER_SCALAR, the element is record s + 1 under BRX_TAKE_NO_DELIM with D = 1.  '{': BRX_MEMBER_OBJECT.  '[':
 *       BRX_MEMBER_ARRAY, and el_rec is again an opener, so a second call takes nested arrays as they are.  ':' and anything else:
 *       BRX_MEMBER_BAD.
 *   EMPTY ARRAY.  [] and [1] look alike in what.  Where the closer stands at r + 1 and record r + 1 is at most
 *       BRX_ELEMENTS_MAX_BLANK = 64 bytes and holds nothing but 0x20, 0x09 and 0x0D, n_elem = 0.  A record above 64 bytes is not
 *       looked at and counts as one element (parse's LONG).
 *   Consequences: [1,] and [,] have a blank SCALAR element, which brx_parse_batch reports as EMPTY.
 * COUNT MODE (el_off, el_stream, el_rec and el_kind all NULL; n_elem required; status and end optional): n_elem[j], status[j] and
 * end[j] for j < m.
 * FILL MODE (all four given; n_elem, status and end optional, written as in count mode): element t of entry j goes to slot el_off[j] +
 * t iff t is below the room of j and the slot is below total; the room of j is (j + 1 < m ? el_off[j + 1] : total) - el_off[j], 0 where
 * that is negative.  Other slots are not touched; nothing at or beyond total is written.
 * Nothing outside the bounds that brx_member_batch's contract names is ever loaded.  Stale or garbage tables give wrong elements,
 * never a load or a store outside these bounds.
 * Check values, r = 2 (the '[' of {"a":[ ) where not said otherwise; stream between brackets, then the status, n_elem, the elements
 * as (el_rec KIND) and end:
 *   [{"a":[]}] r 2: OK 0 end 3
 *   [{"a":[ ]}] r 2: OK 0 end 3
 *   [{"a":[1,]}] r 2: OK 2 (3 SCALAR)(4 SCALAR) end 4
 *   [{"a":[1:2]}] r 2: OK 1 (3 BAD) end 4
 *   [{"a":[1}] r 2: MISMATCH 1 (3 SCALAR) end 3
 *   [{"a":[1,2\n] r 2: UNCLOSED 1 (3 SCALAR) end 4
 *   [{"a":[1,[2] r 2: UNCLOSED 1 (3 SCALAR) end 5
 *   [{"a":[[1,2],{"b":[3]},4]}] r 2: OK 3 (3 ARRAY)(7 OBJECT)(13 SCALAR) end 13
 *   [{"a":["],[",2]}] r 2: OK 2 (3 SCALAR)(4 SCALAR) end 4
 *   [{"a":[<64 x 20>]}] r 2: OK 0 end 3
 *   [{"a":[<65 x 20>]}] r 2: OK 1 (3 SCALAR) end 3
 *   [{"a":[,]}] r 2: OK 2 (3 SCALAR)(4 SCALAR) end 4
 *   [{"a":{}}] r 2: NOT_ARRAY 0
 *   [{"a":[1]}] r 9: NONE 0
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued, and behind
 * brx_index_set_batch and brx_member_batch calls on the same stream it needs no synchronisation in between.  The context's lock is
 * held to enqueue only.  One launch, no scratch of the context's.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; only one of sel_stream / sel_rec; only some
 * of el_off / el_stream / el_rec / el_kind; n_elem NULL in count mode; then m = 0 returns BRX_SUCCESS, no launch; then sel_stream
 * NULL; out_off, len, count or pos_off NULL with n > 0; pos or what NULL with n_pos > 0; span, m, n_pos or total out of range of one
 * launch.
 * Not in scope: objects ('{' gives NOT_ARRAY: the members of a nested object are the next verb, brx_object_batch below); paths;
 * validating JSON;
 * pretty-printed JSON with line feeds inside an array; any change to brx_index_set_batch, brx_member_batch or the record calls.
 * Reads `what` behind every opener up to its stop, once per call, and record r + 1 of the arrays whose closer stands at r + 1; no
 * reference counterpart.  An array that has not ended 64 boundaries behind its opener is taken by its whole wavefront, 1024
 * boundaries per step. */
#define BRX_ELEMENTS_MAX_BLANK 64u
#define BRX_ELEMENTS_OK        0u /* the array ended at a ']' */
#define BRX_ELEMENTS_NONE      1u /* the entry selects no boundary that counts */
#define BRX_ELEMENTS_NOT_ARRAY 2u /* the boundary is not a '[' */
#define BRX_ELEMENTS_UNCLOSED  3u /* a line feed or the stream's end came first */
#define BRX_ELEMENTS_MISMATCH  4u /* the array ended at a '}' */
int brx_elements_batch(brx_ctx *ctx,
                       const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                       const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, const uint8_t *what, uint64_t n_pos,
                       const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                       uint64_t *n_elem, uint8_t *status, uint64_t *end,
                       const uint64_t *el_off, uint64_t total, uint32_t *el_stream, uint64_t *el_rec, uint8_t *el_kind,
                       void *hip_stream);

/* ---- the named members of nested JSON objects as selections for the record calls (device memory only) ----------------
 * brx_member_batch answers kind = BRX_MEMBER_OBJECT and sel_rec = the boundary of the '{' for "meta":{"lang":"en","score":0.93}, and
 * brx_elements_batch answers BRX_MEMBER_OBJECT for every object of "items":[{"id":1,"price":2.5},...]; there the pipeline ended.  This
 * pass takes it from there: for a selection of object openers it gives, per requested name, the (stream, record) pair and the kind of
 * the member's value, and per object the number of members and the closing bracket (the extent of the nested value).  Its input is
 * what member and elements emit, its output what they and the record calls take: a path a.b.c is member, object, object; an array of
 * objects is member, elements, object, parse.
 * out ... n_pos are exactly as for brx_elements_batch: the tables of a fill-mode brx_index_set_batch call at { } [ ] : , and the line
 * feed, quote '"', escape '\'.  (sel_stream, sel_rec) is a pairs-mode selection of m openers: sel_rec = the boundary index of the
 * '{'.  A whole column of member's output, or elements' el_stream / el_rec, may be passed with the entries that are no object left in.
 *   names, name_len   HOST memory, whatever the other pointers are, read before the call returns, exactly as for brx_member_batch:
 *             name q is names[32 q .. 32 q + name_len[q]); 0 <= n_names <= BRX_MEMBER_MAX_NAMES = 8, 1 <= name_len[q] <=
 *             BRX_MEMBER_MAX_NAME = 32, no name twice.  They travel to the kernel as launch arguments: no upload, and the call stays
 *             enqueue-only.  n_names = 0 is the EXTENT MODE: n_members, status and end alone.
 * Everything else is DEVICE memory.
 * THE RULE.  Boundary k of stream i, w_k and C(i) = min(count[i], n_pos - pos_off[i]) (0 where pos_off[i] >= n_pos), the boundaries
 * that count, are as in brx_member_batch's RULE.  Nothing at or behind n_pos is loaded, neither from what nor from pos.  Entry j has
 * i = sel_stream[j], r = sel_rec[j].
 *   BRX_OBJECT_NONE.  i >= n or r >= C(i): n_members = 0, end = UINT64_MAX.  Member's MISSING (sel_rec = UINT64_MAX) lands here.
 *   BRX_OBJECT_NOT_OBJECT.  w_r is not '{': n_members = 0, end = UINT64_MAX.
 *   THE WALK.  Otherwise k = r + 1, r + 2, ... with the relative depth e = 1.  '{' and '[' give e += 1.  '}' and ']' give e -= 1; at
 *       e = 0 the object ends at k: status BRX_OBJECT_OK for '}', BRX_OBJECT_MISMATCH for ']', end = k.  A '\n' boundary stops the walk
 *       (BRX_OBJECT_UNCLOSED, end = k), as does k = C(i) (BRX_OBJECT_UNCLOSED, end = C(i)).  Every other byte is neutral.  The members
 *       seen before the stop stand.
 *   A MEMBER is a ':' boundary k met with e = 1; n_members counts them.  Its KEY RECORD (record k of the stream under
 *       BRX_TAKE_NO_DELIM with D = 1), the trim of 0x20, 0x09 and 0x0D, "carries name q" (bytewise, no escape is resolved), the limit of
 *       BRX_MEMBER_MAX_KEY = 64 bytes before trimming and the backslash flag are word for word brx_member_batch's.
 *   VALUE of the member at k: mem_rec = k + 1, and its kind follows from w_{k+1} as in member's RULE: ',' or '}': BRX_MEMBER_SCALAR,
 *       the value is record k + 1.  '{': BRX_MEMBER_OBJECT, again an opener for this call.  '[': BRX_MEMBER_ARRAY, an opener for
 *       brx_elements_batch.  Anything else -- a '\n', a ']', k + 1 = C(i) -- BRX_MEMBER_BAD.
 *   LAST WINS among the members of the walk, as json.loads has it with duplicates.  None carries name q: mem_kind = BRX_MEMBER_MISSING
 *       and mem_rec = UINT64_MAX, which selects nothing.  mem_stream is sel_stream[j] in every case, whatever it is.
 *   Results are column-major: entry (q, j) is at index q * m + j, so one name's column is a contiguous selection for a record call or
 *   for this one.  Every slot with j < m is written, for NONE and NOT_OBJECT entries too; nothing at or beyond n_names * m is written.
 *   obj_flags[j] (optional): BRX_MEMBER_LONG_KEY | BRX_MEMBER_ESCAPED_KEY over the entry's own members only (0 for NONE and
 *       NOT_OBJECT).  n_members, status and end are each optional; with n_names = 0, n_members is required.
 * Nothing outside the bounds that brx_member_batch's contract names is ever loaded.  Stale or garbage tables give wrong members,
 * never a load or a store outside these bounds.
 * Check values; stream between brackets, names a, b, c, u, x where not said otherwise, then the status, n_members, end, the names
 * found as name KIND mem_rec (the others MISSING) and obj_flags:
 *   [{"u":{"a":1,"b":[2,3],"a":4},"a":5}] r 2: OK members 3 end 11; a SCALAR 11 b ARRAY 6 flags 0
 *   [{"u":{"a":1,"b":[2,3],"a":4},"a":5}] r 0: OK members 2 end 14; a SCALAR 14 u OBJECT 2 flags 0
 *   [{"a":{}}] r 2: OK members 0 end 3 flags 0
 *   [{"a":{"b":1]}] r 2: MISMATCH members 1 end 4; b BAD 4 flags 0
 *   [{"a":{"b":1,"c":2\n] r 2: UNCLOSED members 2 end 6; b SCALAR 4 c BAD 6 flags 0
 *   [{"a":{"b":] r 2: UNCLOSED members 1 end 4; b BAD 4 flags 0
 *   [{"a":{"x":{"b":1},"b":2}}] r 2: OK members 2 end 9; b SCALAR 9 x OBJECT 4 flags 0
 *   [{"a":{"x":{"b":1},"b":2}}] r 4: OK members 1 end 6; b SCALAR 6 flags 0
 *   [{"items":[{"id":1},{"id":2}]}] r 3: OK members 1 end 5; id SCALAR 5 flags 0   (name id)
 *   [{"items":[{"id":1},{"id":2}]}] r 7: OK members 1 end 9; id SCALAR 9 flags 0   (name id)
 *   [{"a":{<30 x 20>"<32 x k>":1}}] r 2: OK members 1 end 4; k32 SCALAR 4 flags 0   (name k32 = 32 x k; a key record of 64 bytes)
 *   [{"a":{<31 x 20>"<32 x k>":1}}] r 2: OK members 1 end 4 flags 1   (name k32 = 32 x k; a key record of 65 bytes)
 *   [{"a":{"a\u0062":1}}] r 2: OK members 1 end 4 flags 2   (name ab)
 *   [{"a":[1]}] r 2: NOT_OBJECT flags 0
 *   [{"a":[1]}] r 9: NONE flags 0
 * hip_stream NULL = the context's own stream and the call returns when the results are there; otherwise it is enqueued, and behind
 * brx_index_set_batch, brx_member_batch and brx_elements_batch calls on the same stream it needs no synchronisation in between.  The
 * context's lock is held to enqueue only.  One launch, no scratch of the context's.
 * BRX_ERR_INVALID_ARGUMENT, checked in this order before anything touches HIP: ctx NULL; n_names above 8; names or name_len NULL with
 * n_names > 0; a name_len of 0 or above 32; a name twice; only one of sel_stream / sel_rec; with n_names > 0 any of mem_stream /
 * mem_rec / mem_kind NULL; with n_names = 0 any of them or obj_flags given, or n_members NULL; then m = 0 returns BRX_SUCCESS, no
 * launch; then sel_stream NULL; out_off, len, count or pos_off NULL with n > 0; pos or what NULL with n_pos > 0; span, m or n_pos
 * out of range of one launch (the bound on m keeps n_names * m in range too).
 * Not in scope: enumerating every member of an object; resolving escapes in keys; more than 8 names or names above 32 bytes;
 * validating JSON; pretty-printed JSON with line feeds inside an object; a single-call path syntax; any change to
 * brx_index_set_batch, brx_member_batch, brx_elements_batch or the record calls.
 * Reads `what` behind every opener up to its stop, once per call, and the key records of the object's own members (none in extent
 * mode); no reference counterpart.  An object that has not ended 64 boundaries behind its opener is taken by its whole wavefront,
 * 1024 boundaries per step. */
#define BRX_OBJECT_OK         0u /* the object ended at a '}' */
#define BRX_OBJECT_NONE       1u /* the entry selects no boundary that counts */
#define BRX_OBJECT_NOT_OBJECT 2u /* the boundary is not a '{' */
#define BRX_OBJECT_UNCLOSED   3u /* a line feed or the stream's end came first */
#define BRX_OBJECT_MISMATCH   4u /* the object ended at a ']' */
int brx_object_batch(brx_ctx *ctx,
                     const uint8_t *out, const uint64_t *out_off, const uint64_t *len, uint32_t n, uint64_t span,
                     const uint64_t *count, const uint64_t *pos_off, const uint64_t *pos, const uint8_t *what, uint64_t n_pos,
                     const uint32_t *sel_stream, const uint64_t *sel_rec, uint64_t m,
                     const uint8_t *names, const uint32_t *name_len, uint32_t n_names,
                     uint64_t *n_members, uint8_t *status, uint64_t *end,
                     uint32_t *mem_stream, uint64_t *mem_rec, uint8_t *mem_kind, uint8_t *obj_flags,
                     void *hip_stream);

/* ---- Read-shaped stream facade (one object = one stream, like one reference Decompressor) ----------
 * brx_stream_new copies the compressed bytes and queues the stream on its context.  The first brx_stream_read of
 * ANY queued stream decodes ALL streams queued on that context in one batch (N live Decompressors cost about one
 * batch, not N launches).  Threads coalesce by themselves (round 6): making a stream never waits for a running batch, so the streams
 * that other threads make while one batch runs go out together as the next one -- ONE reader leads it, the others wait for their
 * own stream only (T threads that each make a stream, read it and free it ride batches of T / 2 .. T -- the leading reader waits a moment, 120 us of
 * quiet and 1.5 ms at most, for the others while batches are small: 16 threads on alice29 324 MB/s, 64 threads 1.15 GB/s, 512 threads 2.9 GB/s, where turns of one stream each gave 24 MB/s; profiles/r06_stream_threads.txt; the context keeps the pinned staging of its largest facade batch, at most 1 GiB).  Later reads serve slices:  n>0 bytes read, 0 at end of stream forever after (reference
 * src/lib.rs:2155-2166).  For an invalid stream the bytes produced before the error are served first, then every
 * read returns -status (the reference returns io::ErrorKind::InvalidData carrying brx_status_str(status) after an
 * unspecified prefix, src/lib.rs:2177).  Values below -900 are library failures (-1000 + BRX_ERR_*),
 * e.g. a stream that expands past the 4 GiB - 256 B per-stream limit; brx_last_error() has the text. */
typedef struct brx_stream brx_stream;
brx_stream *brx_stream_new(brx_ctx *ctx, const uint8_t *in, size_t n);
/* The same object in BOUNDED mode (brx_stream_new picks it by itself for compressed inputs of 4 MiB and more): the stream
 * is decoded slice by slice -- about 4 MiB of output per brx_stream_read that runs dry -- by a resumable kernel into a
 * sliding window on the device (the slices that readers of one context ask for at the same time share a launch: see rounds below), so the output resident at any time is bounded by the largest Brotli window (16 MiB) plus
 * one slice plus slack (~22 MiB) however large the stream (like the reference's Decompressor, whose state is its window,
 * src/lib.rs:377-394, 1560-1567).  Reads see decoded bytes as the slices complete; an invalid stream serves everything
 * decoded before the error.  A single command that produces more than the slack (a > 1 MiB copy, insert or uncompressed
 * meta-block) is taken back by the kernel, which pauses in front of it; the window slides and, if the command still does not fit, the
 * buffer grows to hold it (at most ~48 MiB more: brx_last_timing 9 counts such pauses);
 * only if that allocation fails does the stream fall back to whole-stream decoding. */
brx_stream *brx_stream_new_bounded(brx_ctx *ctx, const uint8_t *in, size_t n);
/* The bounded reader over a SOURCE instead of a buffer: the reference's Decompressor::new(r: R) with R: Read
 * (src/lib.rs:398-410), which pulls its input through a BufReader as it decodes (src/bitreader/mod.rs:21-53).  `read` is called
 * -- from inside brx_stream_read, on the caller's thread -- for up to `cap` more compressed bytes; it returns how many it gave,
 * 0 = end of input (and is not called again).  Compressed input is held in a sliding 8 MiB device window the same way the
 * output is (BRX_OPTION_READER_WINDOW): a stream of any length decodes with about 32 MiB of buffers on the device and 1 MiB on the
 * host.  A slice pauses before its resident input runs out -- in front of the header, uncompressed block or command that would
 * not fit -- and goes on once more is resident.  One item that needs more than the window holds (an uncompressed meta-block is
 * up to 16 MiB) makes the window grow, doubling up to 256 MiB; one command that produces more than the slack makes the output
 * buffer grow (see above).  `read` runs with the context's lock released: it may itself read from another brx_stream of the
 * same context (a Decompressor over a Decompressor).  A callback that returns more than `cap` fails the stream
 * (BRX_ERR_INVALID_ARGUMENT).  The context must outlive every read. */
typedef size_t (*brx_read_fn)(void *user, uint8_t *buf, size_t cap);
brx_stream *brx_stream_new_reader(brx_ctx *ctx, brx_read_fn read, void *user);
int64_t brx_stream_read(brx_stream *s, uint8_t *buf, size_t len);
void brx_stream_free(brx_stream *s);
/* Rounds (round 7).  A slice is one wavefront's work, so the slices of many bounded / pulled streams of a context run as ONE launch:
 * a reader round.  Two ways in:
 *  - Threads: a brx_stream_read that needs a slice queues it; one reader leads a round over everything queued (at most what the chip
 *    runs at a time, 16 waves per CU; the rest goes out with the next one) while the others wait for their own stream.  Slices are
 *    long, so the slices asked for while one round runs form the next one.  The leader holds the context's lock only to enqueue a round
 *    and to settle its results: owners prepare their next slices -- and their pull callbacks run -- while the GPU decodes.
 *  - brx_stream_advance, for a host that multiplexes many streams on one thread (an event loop over sockets): every listed stream
 *    that is bounded or pulled, unfinished, and has no decoded bytes left to read moves on by one slice, all of them in shared
 *    launches; the call returns when they have run.  The others -- streams with bytes to read, finished ones, whole-stream facade
 *    streams -- are left alone.  All streams must be on one context (else, or for a NULL entry, BRX_ERR_INVALID_ARGUMENT).  Returns how
 *    many streams it moved on (0: none could), or a BRX_ERR_* code.
 * Pull callbacks keep their contract: a stream's callback runs on the thread that reads or advances it, with the context's lock
 * released; the leader of a round never calls another stream's.  A slice decoded in a round is copied to pinned host memory of the
 * stream's (~5 MiB while it is being read; at most 1 GiB per context, streams beyond read from the device): brx_stream_read serves it
 * with no HIP call and without the context's lock.  brx_stream_free of a stream whose slice a round is running waits for that round.
 * BRX_OPTION_READER_BATCH = 0 gives every slice a launch of its own, as before round 7; it may be changed at any time and holds from
 * the next slice a stream asks for.  A round is not "the most recent launch" of brx_last_timing 2 .. 7, 10 .. 12 and brx_last_trace
 * (those keep describing the context's batches and single slices, and do not wait for a round); it has a work counter of its own, so
 * BRX_OPTION_GRID_CAP holds for rounds too. */
int brx_stream_advance(brx_stream *const *streams, uint32_t n);
/* Decoded bytes of the stream that brx_stream_read hands out without decoding anything (0 for a whole-stream facade stream that has not
 * been decoded yet).  No HIP call, no lock: for the thread that owns the stream, e.g. to read between brx_stream_advance calls. */
int64_t brx_stream_ready(const brx_stream *s);

/* ---- The node: the GPUs of one machine behind ONE call (round 6) ---------------------------------------------
 * Streams are independent -- a reference Decompressor owns all of its state (src/lib.rs:378-394) -- so a batch shards trivially: a
 * brx_node owns one brx_ctx per GPU (one process, one host thread per GPU), deals the streams of a batch over them, decodes the
 * shards at the same time and leaves every result where the caller said, exactly as brx_decode_batch would have.  This is how a
 * host that is not Python (the Rust `Decompressor` pool of INTEGRATION.md) reaches GPUs 1 .. 7.
 *   BRX_MEM_HOST    every GPU reads its streams from, and writes its results to, the caller's buffers: no exchange between GPUs at
 *                   all (pinned buffers -- brx_host_alloc -- are used in place by every GPU's kernel; pageable ones are staged per GPU).
 *   BRX_MEM_DEVICE  every pointer is memory of the ROOT rank's GPU.  The other ranks get exactly their shard of the compressed bytes
 *                   over xGMI (scatter), decode, compact their results and send them back (ragged gather); the root expands them
 *                   into the caller's slots.  One grouped exchange each way: RCCL (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd,
 *                   one communicator per GPU in this process; librccl is loaded the first time it is needed) or plain peer copies
 *                   (hipMemcpyPeerAsync) -- BRX_NODE_OPTION_TRANSPORT.  No collective ever runs inside the decode.
 * Dealing (brx_node_opts::deal):
 *   BRX_NODE_DEAL_RANGES  rank r of G takes the contiguous index range [r * n / G, (r + 1) * n / G)            (default)
 *   BRX_NODE_DEAL_BYTES   contiguous ranges cut at equal shares of the COMPRESSED bytes (a batch that is sorted or drifts in size)
 *   BRX_NODE_DEAL_SNAKE   the streams sorted by compressed size, largest first, and dealt 0 .. G-1, G-1 .. 0, ... with every rank
 *                         keeping the stream count of its index range: a ragged batch within a few percent of equal bytes AND equal
 *                         counts per GPU.  Not contiguous, so every rank's shard is packed and its results are unpacked (one more
 *                         pass over the data: host memcpy under BRX_MEM_HOST, an HBM-rate gather kernel under BRX_MEM_DEVICE).
 * How many GPUs a batch is dealt over (brx_node_opts::use_gpus = 0): one per BRX_NODE_OPTION_MIN_STREAMS streams (default: what one
 * GPU decodes at a time, 16 per CU = 4096 on MI355X) -- a stream is a serial job of one wavefront, and 512 of them take a GPU about as
 * long as 4096; give use_gpus (or lower the option) to trade GPUs for latency.
 * The devices of a node need not differ: several ranks on one GPU ("virtual ranks") run the same code -- contexts, threads,
 * dealing, scatter, gather -- which is how the path is tested on a one-GPU box.
 * Results, status codes and error behaviour per stream are those of brx_decode_batch.  The call returns when everything is done. */
typedef struct brx_node brx_node;

#define BRX_NODE_DEAL_RANGES 0u
#define BRX_NODE_DEAL_BYTES 1u
#define BRX_NODE_DEAL_SNAKE 2u

typedef struct brx_node_opts {
    uint32_t flags;   /* BRX_MEM_HOST | BRX_MEM_DEVICE | BRX_OPT_TIMING */
    uint32_t deal;    /* BRX_NODE_DEAL_* */
    int32_t use_gpus; /* 0 = the library picks (see above); else the batch is dealt over ranks 0 .. use_gpus - 1 (root included) */
    int32_t root;     /* BRX_MEM_DEVICE: the rank whose GPU holds the buffers (0 <= root < use_gpus) */
    void *hip_stream; /* BRX_MEM_DEVICE: a stream of the root's GPU the call's work is ordered behind (NULL: none) */
} brx_node_opts;

enum {
    BRX_NODE_OPTION_TRANSPORT = 100,    /* 0 = RCCL where every rank has a GPU of its own, peer copies otherwise (default); 1 = peer
                                           copies (hipMemcpyPeerAsync); 2 = RCCL (fails with BRX_ERR_INVALID_ARGUMENT for virtual ranks,
                                           BRX_ERR_HIP if librccl cannot be loaded) */
    BRX_NODE_OPTION_MIN_STREAMS = 101,  /* streams per GPU below which use_gpus = 0 does not add a GPU (0 = the default, see above) */
    BRX_NODE_OPTION_EXCHANGE_ROOT = 102 /* 1 = under BRX_MEM_DEVICE the root's own shard travels through the transport as well (to
                                           itself) instead of being decoded in place: exercises the send / receive pair on one GPU */
};

/* devices: n_devices HIP device indices, rank r on devices[r]; NULL / 0 = every visible GPU, one rank each.  Fails like
 * brx_ctx_create (BRX_ERR_NO_DEVICE without a GPU: there is no CPU fallback). */
int brx_node_create(brx_node **out, const int *devices, int n_devices);
void brx_node_destroy(brx_node *node); /* (not while a call on the node is in flight on another thread) */
int brx_node_size(const brx_node *node);
/* The context of a rank (owned by the node): for brx_ctx_set_option / brx_last_timing on one GPU.  Do not destroy it. */
brx_ctx *brx_node_ctx(brx_node *node, int rank);
/* BRX_OPTION_* : applied to every rank's context.  BRX_NODE_OPTION_* : the node's own. */
int brx_node_set_option(brx_node *node, uint32_t option, int64_t value);
/* brx_decode_batch over the node.  Arguments as there; see the block comment above for where the pointers live. */
int brx_node_decode_batch(brx_node *node, const uint8_t *in, const uint64_t *in_off, uint32_t n, uint8_t *out,
                          const uint64_t *out_off, uint64_t *out_len, int32_t *status, const brx_node_opts *opts);
/* The dealing of brx_node_decode_batch on its own (host arithmetic, no GPU is touched): order[k] = the caller's index of the k-th
 * stream in dealt order (the identity for the two contiguous deals), rank r takes order[cut[r] .. cut[r + 1]).  in_off: n + 1
 * offsets in host memory; order: n entries; cut: gpus + 1 entries.  For callers that place their data themselves, and for tests. */
int brx_node_deal(const uint64_t *in_off, uint32_t n, int gpus, uint32_t deal, uint32_t *order, uint32_t *cut);
/* Of the most recent brx_node_decode_batch.  which: 0 = ranks the batch was dealt over; 1 = streams of `rank`; 2 = compressed
 * bytes of `rank`; 3 = decode-kernel milliseconds of `rank` (BRX_OPT_TIMING, else -1); 4 = wall milliseconds of the whole call;
 * 5 = wall milliseconds until every shard was on its GPU (BRX_MEM_DEVICE: the scatter; else 0); 6 = 1 if the exchange went through
 * RCCL, 0 for peer copies / no exchange.  Returns < 0 if unavailable. */
double brx_node_last_timing(brx_node *node, int which, int rank);

#ifdef __cplusplus
}
#endif
#endif
