/* zmi355.h -- C ABI of the MI355X-native DEFLATE engine (libzmi355.so).
 *
 * Two layers, both plain C (pointers + sizes, no C++ / torch types):
 *
 *  1. The zlib stream ABI of the reference, unchanged: z_stream, deflateInit2_/deflate/deflateEnd,
 *     inflateInit2_/inflate/inflateEnd, compress2/uncompress, adler32/crc32 (+_combine) ...
 *     Declared in zmi355_zlib.h with the reference line each symbol replaces
 *     (libz-rs-sys/src/lib.rs) and exported by the drop-in library libz_mi355.so, which is built on this one:
 *     a caller of libz-rs-sys relinks against libz_mi355.so.
 *
 *  2. The batch entry points below (new, additive).  The reference's ABI is one stream per call
 *     (libz-rs-sys/src/lib.rs:1281 deflate, :636 inflate); the north-star workload is thousands of
 *     independent 1 MiB shards, which need one launch per batch, not per stream.  Semantics per
 *     shard are exactly those of
 *         deflateInit2_(level, Z_DEFLATED, windowBits(wrap), 8, strategy) + deflate(Z_FINISH) + deflateEnd
 *         (test-libz-rs-sys/examples/blogpost-compress.rs:43-122), and
 *         inflateInit2_(windowBits(wrap)) + inflate(Z_FINISH) + inflateEnd
 *         (test-libz-rs-sys/examples/blogpost-uncompress.rs:6-44)
 *     with the per-shard return code reported in status[] using zlib's numbering
 *     (zlib-rs/src/c_api.rs:140-148): 0 ok, -3 Z_DATA_ERROR, -5 Z_BUF_ERROR, 2 Z_NEED_DICT.
 *
 * Every function here requires a gfx950 device; there is no CPU fallback (ZMI_E_NODEVICE).
 */
#ifndef ZMI355_H
#define ZMI355_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zmi_ctx zmi_ctx;

/* wrapper selection (windowBits of the reference: -15 raw, 15 zlib, 31 gzip, 47 auto-detect) */
#define ZMI_WRAP_RAW 0
#define ZMI_WRAP_ZLIB 1
#define ZMI_WRAP_GZIP 2
#define ZMI_WRAP_AUTO 3 /* inflate only */

/* library-level return codes (per-shard codes use zlib numbering, see above) */
#define ZMI_E_OK 0
#define ZMI_E_NODEVICE (-101)
#define ZMI_E_HIP (-102)
#define ZMI_E_ARG (-103)
#define ZMI_E_NOMEM (-104)
#define ZMI_E_NORCCL (-105) /* the multi-GPU entry points need RCCL (librccl.so.1) and it could not be loaded */
#define ZMI_E_RCCL (-106)   /* an RCCL call failed; zmi_last_error() holds ncclGetErrorString's text */

const char* zmi_version(void);
const char* zmi_last_error(void);

int zmi_ctx_create(zmi_ctx** ctx, int device);
int zmi_ctx_destroy(zmi_ctx* ctx);
/* upper bound of scratch the context may allocate on the device (default 8 GiB; env ZMI_SCRATCH_MB) */
int zmi_ctx_set_scratch_limit(zmi_ctx* ctx, uint64_t bytes);
/* total output capacity (sum of d_out_cap) one inflate batch may cover.  Inflate keeps 1 bit of scratch
 * per output byte; the capacities live on the device, so the bound comes from here (default: the scratch
 * limit, i.e. 8 GiB of output -> 1 GiB of bitmap).  Streams beyond it report Z_MEM_ERROR (-4). */
int zmi_ctx_set_inflate_out_limit(zmi_ctx* ctx, uint64_t bytes);

/* Host-buffer batches (zmi_deflate_batch / zmi_inflate_batch) stage their chunks through pinned host memory and device slots
 * that the context keeps for the next call (three slots; up to ~6.4 GiB pinned + as much HBM after a multi-GiB batch).
 * zmi_ctx_set_pinned_limit bounds the pinned part (default 10 GiB, env ZMI_PINNED_MB; >= 64 MiB): chunk sizes follow it and a
 * call that ends above it releases the staging.  zmi_ctx_trim releases it now.  If pinned memory cannot be had at all
 * (memlock / container limits) the calls fall back to plain copies instead of failing. */
int zmi_ctx_set_pinned_limit(zmi_ctx* ctx, uint64_t bytes);
int zmi_ctx_trim(zmi_ctx* ctx);

/* hipStream_t the single-stream host wrappers of this context (zmi_inflate_resume) copy and launch on, and the only thing
 * they wait for; default: the null stream.  One context per thread, each with its own stream, run concurrently. */
int zmi_ctx_set_stream(zmi_ctx* ctx, void* stream);

/* Decode-table entries (literal/length + distance tables) the device built for the most recent dynamic block that
 * zmi_inflate_resume calls on this context met; 0 before the first one.  The reference's inflateCodesUsed
 * (libz-rs-sys/src/lib.rs:1252, zlib-rs/src/inflate.rs:2372: state.next) reports the same quantity for its own tables
 * (roots 10 / 9, ENOUGH 1332 + 592); the device tables use roots 9 / 8 with exact-fit sub-tables (at most 852 + 400). */
int zmi_ctx_last_codes_used(zmi_ctx* ctx, uint32_t* entries);
int zmi_ctx_reset_codes_used(zmi_ctx* ctx);

/* per-kernel HIP-event timing for benchmarking: kernels 0 checksum, 1 lz77, 2 encode, 3 inflate (decode),
 * 4 verify, 5 cost parse (deflate levels 3-9) / window scan (zmi_inflate_stream_dev), 6 inflate (resolve), 7 pack / stitch copies.  zmi_ctx_get_timing synchronises, returns the sums (ms) / launch counts since the
 * previous call (arrays of 8) and resets them. */
int zmi_ctx_set_timing(zmi_ctx* ctx, int on);
int zmi_ctx_get_timing(zmi_ctx* ctx, double* ms_sums, uint32_t* counts);

/* worst-case compressed size of an n-byte shard; same formula as the reference's compress_bound
 * (zlib-rs/src/deflate.rs:2975-2991) with the wrapper overhead of `wrap`, rounded up to 16. */
uint64_t zmi_deflate_bound(uint64_t n, int wrap);

/* ---- device-resident batch API (all d_* pointers are device memory; stream is a hipStream_t) ---- */

/* shard i = d_in[d_in_off[i] .. + d_in_len[i]); compressed stream i is written at
 * d_out + i*out_stride (out_stride multiple of 16, >= zmi_deflate_bound(max_len, wrap)),
 * its length to d_out_len[i], its zlib return code to d_status[i].
 * level 0..9 or -1, strategy 0..4 as deflateInit2_ (libz-rs-sys/src/lib.rs:2005-2041). */
int zmi_deflate_batch_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                          uint32_t n_shards, uint32_t max_len, int level, int strategy, int wrap, void* d_out,
                          uint64_t out_stride, uint32_t* d_out_len, int32_t* d_status, void* stream);

/* stream i = d_in[d_in_off[i] .. + d_in_len[i]); output i is written at d_out + d_out_off[i]
 * (capacity d_out_cap[i]); d_out_len[i] receives the number of bytes produced, d_status[i] the
 * zlib return code (0 = stream complete and check value correct). */
int zmi_inflate_batch_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                          uint32_t n_streams, int wrap, void* d_out, const uint64_t* d_out_off,
                          const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status, void* stream);

/* Chained form used by the zlib stream ABI (libz_mi355.so): the shards are consecutive segments of
 * ONE raw deflate stream, contiguous in d_in.  Each starts byte aligned (the empty stored block of
 * Z_SYNC_FLUSH, zlib-rs/src/deflate.rs:2733-2738) and matches into the up to 27 KiB in front of it
 * (window carry-over); finish != 0 makes the last shard end the stream.  The _dict form also treats the
 * dict_len bytes in front of the first segment as history: a preset dictionary (deflateSetDictionary,
 * deflate.rs:499-564) or the tail of the input of an earlier call on the same stream.
 * out_stride: zmi_deflate_bound(max_len, raw) + 16 -- a segment that does not end the stream carries the 5-byte sync
 * marker behind its last block, which the bound of a finished stream does not cover for segments of a few bytes. */
int zmi_deflate_chain_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                          uint32_t n_shards, uint32_t max_len, int level, int strategy, int finish, void* d_out,
                          uint64_t out_stride, uint32_t* d_out_len, int32_t* d_status, void* stream);
int zmi_deflate_chain_dict_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                               uint32_t n_shards, uint32_t max_len, int level, int strategy, int finish,
                               uint32_t dict_len, void* d_out, uint64_t out_stride, uint32_t* d_out_len,
                               int32_t* d_status, void* stream);
/* The chained form for a stream opened with windowBits 9..14 (deflateInit2_, zlib-rs/src/deflate.rs:252-312):
 * back-references reach at most 2^window_bits - 262 bytes (the reference's max_dist, deflate.rs:1423-1425), so an
 * inflater that allocates only the announced window can read the stream.  window_bits 15 = zmi_deflate_chain_dict_dev. */
int zmi_deflate_chain_window_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                 uint32_t n_shards, uint32_t max_len, int level, int strategy, int finish,
                                 uint32_t dict_len, uint32_t window_bits, void* d_out, uint64_t out_stride,
                                 uint32_t* d_out_len, int32_t* d_status, void* stream);
/* As zmi_inflate_batch_dev, additionally reporting the consumed input bytes and why a stream
 * stopped (d_detail: 0 done/error, 1 needs more input, 2 needs more output space; a data error inside the deflate data: 16 + k,
 * k the index of the reference's message).  d_in_used of a stream that fails inside its deflate data is the reference's
 * total_in: all of the input when it ran out, otherwise the bytes up to the last bit read (the end of the token, repeat or
 * header field that is wrong; an invalid code counts with the bits of its table entry: one bit for the unused half of a
 * single-code form).  zmi_inflate_resume_dev and the calls built on it report the same count. */
int zmi_inflate_batch_dev_ex(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                             uint32_t n_streams, int wrap, void* d_out, const uint64_t* d_out_off,
                             const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status, uint32_t* d_in_used,
                             int32_t* d_detail, void* stream);
/* As zmi_inflate_batch_dev_ex with preset dictionaries: d_out_hist[i] (array may be NULL) bytes directly in front
 * of stream i's output region are history the stream may refer to (inflateSetDictionary,
 * zlib-rs/src/inflate.rs:2492-2536).  A zlib stream with FDICT set reports Z_NEED_DICT (2) when its entry is 0;
 * checking its DICTID against the dictionary is the caller's job. */
int zmi_inflate_batch_dict_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                               uint32_t n_streams, int wrap, void* d_out, const uint64_t* d_out_off,
                               const uint32_t* d_out_cap, const uint32_t* d_out_hist, uint32_t* d_out_len,
                               int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, void* stream);
/* ---- one shared preset dictionary for a whole batch (small records: pages, log lines, messages, rows) ----
 * Per shard exactly deflateInit2_(level, Z_DEFLATED, -15 | 15, 8, strategy) + deflateSetDictionary(dict) + deflate(Z_FINISH)
 * (zlib-rs/src/deflate.rs:499-564, header :1572-1601), per stream inflateInit2_ + inflateSetDictionary(dict) +
 * inflate(Z_FINISH) (zlib-rs/src/inflate.rs:2492-2536, :1036-1062), with ONE copy of the dictionary in device memory for
 * every shard of the call.
 *   wrap     ZMI_WRAP_RAW or ZMI_WRAP_ZLIB; gzip and auto return ZMI_E_ARG (a gzip member has no dictionary field).
 *   d_dict   any device address at any alignment, any dict_len.  Deflate matches into the tail the search can reach:
 *            32768 - 5 * 1024 = 27 648 bytes, rounded down to a multiple of 16 (a dictionary shorter than 16 bytes is
 *            announced but not matched into) -- the cap a chained segment's carry-over has; the shorter reach is this
 *            engine's existing max_dist deviation (farthest back-reference 27 632), not a new one.  Inflate uses the
 *            last 32 768 bytes.  d_dict NULL or dict_len 0: the call is zmi_deflate_batch_dev / zmi_inflate_batch_dev_ex,
 *            byte for byte.
 *   DICTID   Adler-32 of all dict_len bytes, computed on the device by the checksum kernel; the encoder and the check
 *            of the decoder read it from a device word.  Neither call synchronises with the host.
 * Deflate: out_stride a multiple of 16, >= zmi_deflate_dict_bound(max_len, wrap).  With the zlib wrapper FDICT is set,
 * FCHECK follows it and the DICTID stands big-endian behind the two header bytes -- at every level and strategy, also
 * level 0 / Z_HUFFMAN_ONLY / Z_RLE, where the dictionary is announced and not (Z_RLE: hardly) used, as in zlib; the Adler-32
 * trailer covers the shard only.  A shard's bytes depend on (dictionary, shard bytes, level, strategy, wrap) alone -- not on
 * n_shards, its index, the alignment of d_in_off or d_dict, the scratch limit or the launch grouping.
 * Inflate: the output regions need no room in front of them.  A zlib stream with FDICT whose DICTID is not the
 * dictionary's reports Z_DATA_ERROR (-3) and no output, as inflateSetDictionary refuses it; a stream without FDICT and any
 * raw stream decodes with the dictionary available and reports 0; a distance that reaches in front of the first
 * dictionary byte is Z_DATA_ERROR; d_in_used and d_detail as in zmi_inflate_batch_dev_ex.  Back-references are always
 * resolved by the one-wave-per-stream pass (never by pointer jumping): the call's case is many small streams. */
/* zmi_deflate_bound + the 4 DICTID bytes of the zlib wrapper, rounded up to 16 */
uint64_t zmi_deflate_dict_bound(uint64_t n, int wrap);
int zmi_deflate_batch_shared_dict_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                      uint32_t n_shards, uint32_t max_len, int level, int strategy, int wrap,
                                      const void* d_dict, uint32_t dict_len, void* d_out, uint64_t out_stride,
                                      uint32_t* d_out_len, int32_t* d_status, void* stream);
int zmi_inflate_batch_shared_dict_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                      uint32_t n_streams, int wrap, const void* d_dict, uint32_t dict_len, void* d_out,
                                      const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len,
                                      int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, void* stream);
/* ---- batch inflate without an output size table ----
 * A raw or zlib stream carries no size and a gzip ISIZE is untrusted, so a caller who kept only the compressed bytes has no
 * d_out_off / d_out_cap to give.  Both calls are asynchronous on `stream`, no value passes through the host.
 *
 * zmi_inflate_sizes_dev   the decode kernel walking every stream's true token chain and adding up the output bytes; nothing is
 *   stored, no bitmap scratch is used, no check value is computed.
 *   d_size[i]    what inflateInit2_ + inflate(Z_FINISH) would produce with unlimited room; for a stream that ends in an error the
 *                count up to the error -- the number zmi_inflate_batch_dev_ex reports in d_out_len given ample room.
 *   d_status, d_in_used, d_detail (the last two may be NULL)   those of zmi_inflate_batch_dev_ex, with ONE difference: check values
 *                are not compared -- Adler-32, CRC-32 and ISIZE are skipped.  0 = the deflate data is well formed, ends, and a
 *                full-length trailer follows; a trailer cut short is truncation (Z_BUF_ERROR, detail 1).
 *   hist         bytes of preset dictionary every stream may reach, 0 .. 32768 (above: ZMI_E_ARG); for the shared-dictionary call
 *                min(dict_len, 32768).  With hist 0 a zlib stream with FDICT reports Z_NEED_DICT (2); DICTID is not checked here.
 *   size_limit   0 = 2^32 - 1.  A stream that would produce more stops with Z_BUF_ERROR, detail 2, d_size[i] = size_limit: the
 *                guard against decompression bombs and the overflow rule in one -- a size never wraps.
 *
 * zmi_inflate_batch_packed_dev   the size pass, a plan kernel, then zmi_inflate_batch_dev_ex (d_dict non-NULL and dict_len > 0:
 *   zmi_inflate_batch_shared_dict_dev, raw or zlib only, otherwise ZMI_E_ARG) with the planned tables: the batch decoded densely
 *   into one buffer.
 *   d_out_off[i] (n_streams + 1 words)  where stream i's output stands: the sizes in front of it, each rounded up to out_align (a
 *                power of two, 1 .. 4096, otherwise ZMI_E_ARG).  d_out_off[n_streams] = the room the whole batch needs -- exact
 *                whether or not it fitted, it comes from the size pass.  n_streams 0 writes d_out_off[0] = 0.
 *   out_cap      bytes at d_out.  When d_out_off[n_streams] > out_cap the streams whose bytes end at or before out_cap are decoded
 *                and are right; every other stream reports Z_BUF_ERROR, detail 2, d_out_len 0 (d_in_used 0); nothing at or behind
 *                d_out + out_cap and nothing in the alignment gaps is written.  The caller reads one word and calls again.
 *   size_limit   as above; a stream that hit it gets a region of size_limit bytes (rounded up) and reports Z_BUF_ERROR, detail 2.
 *   For every stream that fits d_out_len, d_status, d_in_used, d_detail and the bytes are exactly those of
 *   zmi_inflate_batch_dev_ex (or the shared-dictionary call) given d_out_off and the sizes as capacities.
 *   Scratch: the bitmap is sized from out_cap (1 bit per byte) for this call; there are no launch groups yet, so a buffer whose
 *   bitmap cannot be reserved returns ZMI_E_NOMEM -- decode such a batch in parts. */
int zmi_inflate_sizes_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                          uint32_t n_streams, int wrap, uint32_t hist, uint32_t size_limit, uint32_t* d_size,
                          int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, void* stream);
int zmi_inflate_batch_packed_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                 uint32_t n_streams, int wrap, const void* d_dict, uint32_t dict_len, uint32_t size_limit,
                                 uint32_t out_align, void* d_out, uint64_t out_cap, uint64_t* d_out_off /* n_streams + 1 */,
                                 uint32_t* d_out_len, int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, void* stream);
/* Resumable decode of raw deflate streams -- the device half of a streaming inflate() that is fed partial input
 * (the reference keeps Mode / BitReader / Window for this, zlib-rs/src/inflate.rs:288-320; here the state is a
 * block-boundary checkpoint).  Stream i starts at bit d_in_bit[i] (0..7, array may be NULL) of its first byte, with
 * d_out_hist[i] bytes of earlier output directly in front of its output region.  d_resume[4i..4i+3] receives
 * {byte, bit, output bytes, complete}: the start of the block the decode stopped in (status Z_BUF_ERROR, d_detail
 * 1 = more input / 2 = more room needed), or the first bit behind the final block (complete = 1, status Z_OK).
 * d_out_len[i] counts everything decoded including the valid part of the unfinished block; a later call that
 * starts at the checkpoint, with the output in front of it as history, reproduces those bytes and continues.
 * Stops on request (what inflate(Z_BLOCK) / inflate(Z_TREES) are built on, zlib-rs/src/inflate.rs:1276-1284,1323,1369,
 * 1772): bits 8..23 of d_in_bit[i] = stop at the block boundary behind that many complete blocks (0: none), bit 24 = stop
 * behind the header of the first block (code tables read, none of its data decoded).  Both report status Z_BUF_ERROR
 * with d_detail 3; a boundary stop leaves the usual checkpoint, a header stop leaves {byte, bit of the first bit behind
 * the header, output bytes, 2 | BFINAL << 2} in d_resume. */
int zmi_inflate_resume_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                           const uint32_t* d_in_bit, uint32_t n_streams, void* d_out, const uint64_t* d_out_off,
                           const uint32_t* d_out_cap, const uint32_t* d_out_hist, uint32_t* d_out_len,
                           int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, uint32_t* d_resume, void* stream);

/* Adler-32 (kind bit 0) and/or CRC-32 (kind bit 1) of every shard (zlib-rs/src/adler32.rs:19, crc32.rs:19) */
int zmi_checksum_batch_dev(zmi_ctx* ctx, const void* d_data, const uint64_t* d_off, const uint32_t* d_len,
                           uint32_t n_shards, int kind, uint32_t* d_adler, uint32_t* d_crc, void* stream);

/* synthetic Silesia-like benchmark shards (csrc/shardgen.h): shard first_shard+i at d_out + i*shard_bytes */
int zmi_gen_shards_dev(zmi_ctx* ctx, void* d_out, uint64_t seed, uint32_t first_shard, uint32_t n_shards,
                       uint32_t shard_bytes, void* stream);

/* shard first_shard + i*shard_step at d_out + i*shard_bytes: a step of `world` is the round-robin shard ownership of a
 * multi-GPU job (rank r owns the shards g with g % world == r, BASELINE.json configs[4]) */
int zmi_gen_shards_strided_dev(zmi_ctx* ctx, void* d_out, uint64_t seed, uint32_t first_shard, uint32_t shard_step,
                               uint32_t n_shards, uint32_t shard_bytes, void* stream);

/* ---- the stitch (replaces the append loop of the reference's parallel-deflate recipe, zlib-rs/src/deflate.rs:4145-4221
 * `split_deflate`; multi-member gzip as read by libz-rs-sys/src/gz.rs:1464-1506): the batch leaves its compressed
 * shards in out_stride-strided slots; these calls turn them into dense, ordered bytes on the device ----
 * zmi_scan_sizes_dev   d_off[0..n] = exclusive prefix sum of d_len[0..n) (u64; d_off[n] = total)
 * zmi_copy_ranges_dev  range i: d_len[i] bytes from d_src + (d_src_off ? d_src_off[i] : i*src_stride) to
 *                      d_dst + d_dst_off[i]; ranges that would end behind dst_cap are skipped (the offsets tell).
 *                      max_len bounds d_len[] (it only shapes the launch).
 * zmi_pack_slab_dev    both: the slots of one batch -> one dense slab + its offsets.  One D2H copy / one send per
 *                      peer then moves the batch; after a slab exchange zmi_copy_ranges_dev scatters a peer's slab into
 *                      the globally ordered output (d_src_off = the peer's scan, d_dst_off = global offsets). */
int zmi_scan_sizes_dev(zmi_ctx* ctx, const uint32_t* d_len, uint32_t n, uint64_t* d_off, void* stream);
int zmi_copy_ranges_dev(zmi_ctx* ctx, const void* d_src, const uint64_t* d_src_off, uint64_t src_stride, const uint32_t* d_len,
                        uint32_t n, uint32_t max_len, void* d_dst, const uint64_t* d_dst_off, uint64_t dst_cap, void* stream);
int zmi_pack_slab_dev(zmi_ctx* ctx, const void* d_slots, uint64_t slot_stride, const uint32_t* d_len, uint32_t n,
                      void* d_slab, uint64_t slab_cap, uint64_t* d_off, void* stream);

/* ---- the stitch across the GPUs of a node (BASELINE.json configs[4]; csrc/exchange.hip) -------------------------------
 * Shard g of a job lives on rank g % world (round-robin); every rank compresses its shards with zmi_deflate_batch_dev (no
 * collective in the compression) and packs them into one dense slab (zmi_pack_slab_dev).  "Append the pieces in order" --
 * the loop of the reference's parallel-deflate recipe, zlib-rs/src/deflate.rs:4145-4221 -- then is:
 *   zmi_exchange_sizes        all-gather of the u32 size tables: d_table[r * n_local + j] = size of shard j * world + r.
 *                             Every rank passes the SAME n_local: a shard count that does not divide by the world size is
 *                             padded with zero sizes on the short ranks (checked: ZMI_E_ARG on every rank otherwise; the
 *                             call waits for `stream` when world > 1)
 *   zmi_stitch_plan_dev       from the table alone: d_goff[r * n_local + j] = byte offset of that shard in the stitched
 *                             output, d_soff[r * (n_local + 1) + j] = its offset inside rank r's slab (last entry of a row =
 *                             the slab's size), d_totals[r] = slab size of rank r, d_totals[world] = size of the output;
 *                             totals_host (may be NULL) receives a copy of d_totals (the call then waits for the stream)
 *   zmi_exchange_slabs        the slabs travel point to point: per round of chunk_bytes ONE ncclGroupStart / End holding an
 *                             ncclSend to and an ncclRecv from every peer -- xGMI is a full mesh, so the 7 transfers of a
 *                             round run side by side, one link each; there is no all-gather-v in RCCL and a ring is never
 *                             used.  root < 0: every rank receives every slab (d_recv[p] = room for slab_bytes[p] bytes;
 *                             the own entry is skipped); root >= 0: only that rank receives, the others may pass NULL.
 *                             A receiving rank MUST give room for every peer whose slab is not empty -- every such peer
 *                             sends, and a send without its receive would hang the group: a NULL entry is ZMI_E_ARG
 *   zmi_exchange_slabs_round  one round with bounded memory: peer p's bytes [lo, lo + chunk_bytes) arrive at the start of
 *                             d_stage[p]; the caller consumes them and reuses the staging for the next round
 *   zmi_copy_ranges_dev       (above) scatters a slab or a round of it into the ordered output: d_src_off = the peer's row
 *                             of d_soff, d_dst_off = its row of d_goff.
 * All operations are enqueued on `stream`; slab_bytes / d_recv / d_stage are HOST arrays of `world` entries.
 * The communicator: zmi_comm_unique_id on one rank, the 128 bytes carried to the others by whatever the host has (MPI, a
 * file, torch's store), zmi_comm_create on every rank (ncclCommInitRank on the context's device) -- or zmi_comm_adopt for a
 * host that already holds an ncclComm_t.  RCCL is loaded on first use (dlopen librccl.so.1; ZMI_RCCL_LIB overrides the
 * file): processes that never call these functions do not need it. */
#define ZMI_UNIQUE_ID_BYTES 128
typedef struct zmi_comm zmi_comm;
int zmi_comm_unique_id(void* id128);
int zmi_comm_create(zmi_comm** comm, zmi_ctx* ctx, int world, int rank, const void* id128);
int zmi_comm_adopt(zmi_comm** comm, zmi_ctx* ctx, void* nccl_comm);
int zmi_comm_destroy(zmi_comm* comm);
int zmi_comm_abort(zmi_comm* comm); /* ncclCommAbort: for a communicator whose peers are gone */
int zmi_comm_world(const zmi_comm* comm);
int zmi_comm_rank(const zmi_comm* comm);
int zmi_exchange_sizes(zmi_comm* comm, const uint32_t* d_sizes, uint32_t n_local, uint32_t* d_table, void* stream);
int zmi_stitch_plan_dev(zmi_ctx* ctx, const uint32_t* d_table, uint32_t world, uint32_t n_local, uint64_t* d_goff,
                        uint64_t* d_soff, uint64_t* d_totals, uint64_t* totals_host, void* stream);
int zmi_exchange_slabs(zmi_comm* comm, const void* d_slab, const uint64_t* slab_bytes, void* const* d_recv,
                       uint64_t chunk_bytes, int root, void* stream);
int zmi_exchange_slabs_round(zmi_comm* comm, const void* d_slab, const uint64_t* slab_bytes, uint64_t lo,
                             uint64_t chunk_bytes, void* const* d_stage, int root, void* stream);

/* ---- single-stream deflate (pigz-style): one complete raw / zlib / gzip stream from a device buffer ---------------------
 * The reference's parallel-deflate recipe, zlib-rs/src/deflate.rs:4145-4221 (split_deflate): the input is cut into pieces of
 * piece_bytes; every piece but the last ends with the empty stored block of a flush (00 00 00 FF FF after the bits of the block
 * in front: Z_SYNC_FLUSH, deflate.rs:2733-2738), the wrapper appears once, and the trailer carries the check value of the whole
 * input, combined on the device from the pieces' Adler-32 / CRC-32 (crc32/combine.rs:3-13, adler32.rs:58).  The header bytes are
 * those of deflateInit2_(level, Z_DEFLATED, 15 / 31, 8, strategy) + deflate() (no deflateSetHeader: MTIME 0, OS 3).
 *
 * zmi_deflate_stream_dev   d_in[0 .. n) -> d_out (out_cap bytes; zmi_deflate_stream_bound(n, piece_bytes, wrap) always
 *                          suffices).  Asynchronous on `stream`, no host synchronisation inside.  Device words written:
 *                          *d_out_len = stream length, *d_status = 0, or the zlib code of the first piece that failed, or
 *                          Z_BUF_ERROR (-5) when the stream does not fit out_cap (*d_out_len then tells the size it needs).
 *                          d_piece_off (NULL or n_pieces + 1 entries): byte offset in d_out of every piece's first deflate byte,
 *                          then the end of the deflate data.  Every piece starts behind a flush marker, so these minus the header
 *                          length are restart points for zmi_inflate_split's seg_start.  n_pieces = ceil(n / piece_bytes), 1 for
 *                          n = 0 (header, 03 00, trailer).  piece_bytes 1 .. 2^30 (ZMI_E_ARG otherwise).
 *   flags 0                      carry-over: every piece matches into the up to 27 KiB in front of it (Z_SYNC_FLUSH);
 *         ZMI_STREAM_INDEPENDENT pieces forget history (Z_FULL_FLUSH): [off[i], off[i+1]) inflates alone (raw) to piece i.
 *   Determinism: the bytes are a function of (input, n, piece_bytes, level, strategy, wrap, flags) alone -- not of the scratch
 *   limit or of how the call is cut into launch groups.  In independent mode a piece's deflate bytes depend only on its own bytes,
 *   the piece size min(piece_bytes, n), level, strategy and whether it is the last one: the multi-GPU form below, run with the same
 *   max_len, is byte-identical to one call on the whole input.
 *
 * The per-rank building blocks of the same stream across the GPUs of a node (round-robin pieces, as the stitch above):
 *   zmi_deflate_pieces_dev   a batch of pieces: d_out_len[i] / d_check[i] (Adler-32 for zlib, CRC-32 for gzip, of the raw bytes;
 *                            unused for raw) / d_status[i]; pieces at d_out + i * out_stride, out_stride >=
 *                            zmi_deflate_pieces_stride(max_len).  final_piece != 0: the batch's last piece ends the stream (BFINAL);
 *                            every other piece ends with the flush marker.  Carry mode needs the contiguous layout (the bytes in front
 *                            of a piece in d_in are its history); ZMI_STREAM_INDEPENDENT takes any layout.  For the bytes of
 *                            zmi_deflate_stream_dev pass max_len = min(piece_bytes, total n).
 *   zmi_checksum_combine_dev (check, raw length) pairs -> the check of the concatenation (*d_out_check) and the total length
 *                            (*d_out_len; either may be NULL), wrap zlib (Adler-32) or gzip (CRC-32).  Entry r * n_local + j is
 *                            piece j * world + r (the layout of zmi_exchange_sizes' tables; world 1 = plain order); entries of
 *                            length 0 count as nothing, whatever their check holds.
 *   zmi_stream_frame_dev     header at d_out[0 .. zmi_stream_header_bytes(wrap)), trailer behind the *d_payload_len bytes of deflate
 *                            data the caller packed at d_out + header (zmi_copy_ranges_dev into d_out + header), *d_out_len = total;
 *                            d_status (may be NULL) as above.
 *   A rank: pieces, zmi_pack_slab_dev, zmi_exchange_sizes of the sizes and of the checks (and of the raw lengths when the pieces are
 *   uneven), zmi_stitch_plan_dev, the slab exchange, zmi_copy_ranges_dev into d_out + header, combine, frame (payload length =
 *   d_totals[world] of the plan). */
#define ZMI_STREAM_INDEPENDENT 1u
uint64_t zmi_deflate_stream_bound(uint64_t n, uint32_t piece_bytes, int wrap);
uint32_t zmi_stream_header_bytes(int wrap);
uint64_t zmi_deflate_pieces_stride(uint32_t max_len);
int zmi_deflate_stream_dev(zmi_ctx* ctx, const void* d_in, uint64_t n, uint32_t piece_bytes, int level, int strategy, int wrap,
                           uint32_t flags, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_piece_off,
                           int32_t* d_status, void* stream);
int zmi_deflate_pieces_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_pieces,
                           uint32_t max_len, int level, int strategy, int wrap, uint32_t flags, int final_piece, void* d_out,
                           uint64_t out_stride, uint32_t* d_out_len, uint32_t* d_check, int32_t* d_status, void* stream);
int zmi_checksum_combine_dev(zmi_ctx* ctx, int wrap, const uint32_t* d_check, const uint32_t* d_len, uint32_t world, uint32_t n_local,
                             uint32_t* d_out_check, uint64_t* d_out_len, void* stream);
int zmi_stream_frame_dev(zmi_ctx* ctx, int wrap, int level, int strategy, const uint64_t* d_payload_len, const uint32_t* d_check,
                         const uint64_t* d_raw_len, void* d_out, uint64_t out_cap, uint64_t* d_out_len, int32_t* d_status,
                         void* stream);

/* ---- single-stream inflate (pigz-style): the inverse of zmi_deflate_stream_dev --------------------------------------------------
 * zmi_inflate_stream_dev    d_in[0 .. in_len) holds ONE member: raw, zlib, gzip, or ZMI_WRAP_AUTO (zlib or gzip by its first bytes).
 *                           d_cuts[0 .. n_cuts) are byte offsets in d_in where pieces start: entry 0 is the end of the header, the
 *                           rest ascend (the first n_pieces entries of zmi_deflate_stream_dev's index are valid as they stand).  Every
 *                           cut is only a proposal: it counts if the decode of the piece in front of it ended exactly there, on a block
 *                           boundary, with all its output complete (the rule of zmi_inflate_split).  piece_out_max (1 .. 2^30) bounds the
 *                           output of any one piece and sizes the decode regions (this library's streams: piece_bytes; pigz: 128 KiB).
 *                           Asynchronous on `stream`, no host synchronisation inside, any length.  Device words written:
 *                           *d_status  0: the stream ended and its check value (and gzip ISIZE, the low 32 bits of the length) match;
 *                                      Z_DATA_ERROR (-3): a corrupt block, a distance in front of the stream's start, a bad header, a
 *                                      wrong check value or length, a cut that did not verify; Z_BUF_ERROR (-5): truncated input, a piece
 *                                      that produced more than piece_out_max, or the output does not fit out_cap (*d_out_len then tells
 *                                      the size it needs); Z_NEED_DICT (2): the zlib FDICT flag (preset dictionaries are not supported).
 *                                      Never status 0 with wrong bytes.
 *                           *d_detail  which case (ZMI_SI_* below) in its low 8 bits; for ZMI_SI_CUT the index of the first cut that
 *                                      did not verify, for ZMI_SI_PIECE / ZMI_SI_DATA / ZMI_SI_FAR the index of the piece, above them.
 *                           *d_out_len the length of the output; *d_in_used header + deflate data + trailer (the next gzip member
 *                                      starts there).  Nothing at or behind d_out + out_cap is written.
 *                           The result does not depend on the scratch limit: pieces beyond it run in launch groups whose output offsets
 *                           and 32 KiB window carry over on the device.
 * zmi_stream_find_cuts_dev  parses the header and writes its end to d_cuts[0], then proposes the byte behind every byte-aligned
 *                           00 00 FF FF behind it, proposals at least min_gap input bytes apart, at most cap entries in all;
 *                           *d_n_cuts = entries written (a device word: reading it is the caller's one synchronisation).  False
 *                           proposals (a stored block holding the pattern) are caught by the cut verification above. */
#define ZMI_SI_HEADER 1  /* bad header (status Z_DATA_ERROR) */
#define ZMI_SI_TRUNC 2   /* the input ends inside the header, the deflate data or the trailer (Z_BUF_ERROR) */
#define ZMI_SI_CUT 3     /* a cut did not verify (Z_DATA_ERROR); index = the cut */
#define ZMI_SI_PIECE 4   /* a piece produced more than piece_out_max (Z_BUF_ERROR); index = the piece */
#define ZMI_SI_DATA 5    /* a corrupt block (Z_DATA_ERROR); index = the piece */
#define ZMI_SI_FAR 6     /* a distance reaches in front of the stream's start (Z_DATA_ERROR); index = the piece */
#define ZMI_SI_CHECK 7   /* wrong Adler-32 / CRC-32 (Z_DATA_ERROR) */
#define ZMI_SI_LENGTH 8  /* wrong gzip ISIZE (Z_DATA_ERROR) */
#define ZMI_SI_OUT 9     /* the output does not fit out_cap (Z_BUF_ERROR) */
#define ZMI_SI_DICT 10   /* zlib FDICT set (Z_NEED_DICT) */
int zmi_inflate_stream_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, int wrap, const uint64_t* d_cuts, uint32_t n_cuts,
                           uint32_t piece_out_max, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used,
                           int32_t* d_status, int32_t* d_detail, void* stream);
int zmi_stream_find_cuts_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, int wrap, uint64_t min_gap, uint64_t* d_cuts, uint32_t cap,
                             uint32_t* d_n_cuts, void* stream);

/* ---- single-stream inflate of streams WITHOUT flush points (what gzip, zlib and zlib-rs write at their default settings) ----------
 * zmi_stream_find_blocks_dev   the shape of zmi_stream_find_cuts_dev, but the entries are BIT offsets into d_in: d_cuts[0] = 8 x the
 *                              end of the header; every further entry is the first of the three header bits of a DYNAMIC block, found
 *                              by trying every bit position (csrc/blockscan.hip: a plausible header, then code lengths that decode
 *                              exactly).  Greedy and exact: entry k + 1 is the smallest position found >= d_cuts[k] + 8 x max(min_gap, 1);
 *                              ascending, at most cap entries, *d_n_cuts = entries written, the same entries on every run.  Any in_len
 *                              (the stream is scanned in windows of 64 MiB, positions are 64-bit), asynchronous on `stream`, no host
 *                              synchronisation.  Scratch of the context: about 9 / 16 of min(in_len, 64 MiB).  Overflow: 2 KiB of input
 *                              in which more than one bit position in 64 looks like a header (ordinary data: one in ~250) proposes
 *                              nothing; a window with more than one block per 64 bytes keeps its first ones.  Never an unvalidated entry.
 *                              NOT found: fixed and stored blocks -- three header bits prove nothing; they ride along in the piece of the
 *                              dynamic block in front of them.  So a stream of only such blocks (level-1 output of some encoders, level
 *                              0) is ONE piece, bounded by piece_out_max <= 2^30 bytes of output.  A proposal may be false (a stored
 *                              block that holds a deflate stream): the verification below catches it.
 * zmi_inflate_stream_bits_dev  zmi_inflate_stream_dev with d_cuts in BITS: piece g starts at bit d_cuts[g] & 7 of byte d_cuts[g] >> 3 and
 *                              reads up to the byte that holds the next cut.  d_cuts[0] must be 8 x the end of the header.  A cut counts
 *                              if the decode in front of it stopped for want of input in a block that starts exactly at that bit; the few
 *                              bits it saw behind the cut produce nothing that is kept.  Status, ZMI_SI_* details, indices, *d_out_len,
 *                              *d_in_used, out_cap and the independence of the scratch limit are those of zmi_inflate_stream_dev; with
 *                              cuts 8 x c[k] it writes the same four words and the same bytes as zmi_inflate_stream_dev with c[k].
 *                              Proposals of both kinds may be mixed (8 x find_cuts' entries merged with find_blocks').
 *                              One member per call; *d_in_used points at the next. */
int zmi_stream_find_blocks_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, int wrap, uint64_t min_gap, uint64_t* d_cuts, uint32_t cap,
                               uint32_t* d_n_cuts, void* stream);
int zmi_inflate_stream_bits_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, int wrap, const uint64_t* d_cuts, uint32_t n_cuts,
                                uint32_t piece_out_max, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used,
                                int32_t* d_status, int32_t* d_detail, void* stream);

/* ---- random access into ONE stream: an index kept while it is decoded once, byte ranges read from it afterwards -----------------------
 * A block start in the middle of an ordinary stream (gzip / zlib / zlib-rs at default settings, this library's carry-mode stream, pigz)
 * needs the 32 KiB of output in front of it.  With the reference one access is inflateInit2_(-15) + inflatePrime (the bits of the first
 * byte in front of the point) + inflateSetDictionary (the window) + inflate, per access, on one core: libz-rs-sys/src/lib.rs:968
 * (inflateInit2_), :1029 (inflatePrime), :1121 (inflateSetDictionary), :637 (inflate) -- zlib's examples/zran.c.  Here the index is a
 * by-product of the verified decode of zmi_inflate_stream_bits_dev, and a batch of ranges is one group of launches.  Both calls are
 * asynchronous on `stream` and do not synchronise with the host.  (gzip members and ZMI_STREAM_INDEPENDENT pieces forget history:
 * their indices -- d_member_off, d_piece_off -- are read through zmi_inflate_batch_dev, or through zmi_inflate_ranges_dev with
 * d_ix_win NULL.)
 *
 * zmi_inflate_stream_index_dev  the arguments of zmi_inflate_stream_bits_dev (cuts in BITS), then the index.  The four device words and
 *                               the bytes at d_out are those of zmi_inflate_stream_bits_dev on the same arguments.  A POINT is (bit
 *                               position in d_in, output offset, the 32 768 bytes of output in front of it).  Point 0 is (d_cuts[0], 0):
 *                               the end of the header, no window.  Greedy and exact: point k + 1 is the first verified piece start g
 *                               whose output offset is >= d_ix_out[k] + max(span, 1); the same entries on every run, whatever the
 *                               scratch limit (the selection continues across launch groups from device words).
 *                               d_ix_bit[ix_cap], d_ix_out[ix_cap + 1]: *d_n_points entries, d_ix_out[*d_n_points] = the total output
 *                               length.  *d_max_gap = the greatest d_ix_out[k + 1] - d_ix_out[k], k < *d_n_points.  If more points
 *                               qualify than ix_cap the first ix_cap are kept, and *d_max_gap includes the long tail behind them.
 *                               d_ix_win (NULL: offsets only; 16-byte aligned, ix_cap * 32768 bytes): window k at d_ix_win + k * 32768,
 *                               right-aligned -- its last byte is output byte d_ix_out[k] - 1, positions in front of the stream's
 *                               start are zero.
 *                               The index is valid only for a verified stream: with *d_status != 0 (a cut that failed, a wrong check
 *                               value, ZMI_SI_OUT: the output did not fit out_cap, ...) *d_n_points = 0.  An index cannot be built
 *                               without room for the whole output.  ix_cap 0 or a NULL d_ix_bit / d_ix_out / d_n_points / d_max_gap:
 *                               ZMI_E_ARG.
 * zmi_inflate_ranges_dev        n_ranges byte ranges of the stream's OUTPUT: range i = [d_lo[i], d_lo[i] + d_len[i]).  The bytes
 *                               [lo, min(lo + len, total)) are written at d_out + off_i (off_i = d_out_off[i], or i * out_stride with
 *                               d_out_off NULL; any alignment), d_got[i] = their count; nothing outside [off_i, off_i + got) is written.
 *                               d_ix_bit / d_ix_out / d_ix_win / n_points / max_gap: an index as built above (max_gap may be any bound
 *                               >= *d_max_gap; it sizes the scratch).  d_ix_win (16-byte aligned) NULL: the points have no history.
 *                               d_status[i]  0: the bytes are right; also for len 0 and for lo >= total (got 0), which decode nothing.
 *                                            Z_DATA_ERROR (-3): corrupt data behind the point, or a distance that reaches in front of
 *                                            the available history (d_ix_win NULL: any distance in front of the point).
 *                                            Z_BUF_ERROR (-5): the input ends inside the extent the range needs.
 *                                            ZMI_E_ARG (-103; the tables live on the device, so it arrives here): len > max_len; the
 *                                            entries around the range's point do not ascend, or the point's bit lies at or behind
 *                                            8 x in_len; lo - d_ix_out[k] >= max_gap or d_ix_out[k + 1] - d_ix_out[k] > max_gap.
 *                               Every non-zero status reports got 0 and writes no byte.
 *                               NO CHECK VALUE IS VERIFIED: the index was built from a verified stream, and a part of a stream has no
 *                               CRC.  A caller who hands in other input than the index was built from gets that input's bytes.
 *                               max_len 1 .. 2^30, max_gap <= 2^30, n_points >= 1 and non-NULL tables, otherwise ZMI_E_ARG as the
 *                               return value; n_ranges 0 is a no-op.  A range decodes from the last point at or in front of lo, up to
 *                               the byte that holds the first point at or behind its end.  Scratch of the context per range: 32 KiB +
 *                               max_gap + max_len, an eighth of that again, 128 bytes; ranges beyond the scratch limit run in launch
 *                               groups.  Bytes and words do not depend on the limit, the order of the ranges, n_ranges or the decode
 *                               kernel.  Event timing: 5 = plan and history, 3 / 6 = decode, resolve, 4 = the decode's status step,
 *                               7 = got / status and the trimmed copy. */
int zmi_inflate_stream_index_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, int wrap, const uint64_t* d_cuts, uint32_t n_cuts,
                                 uint32_t piece_out_max, void* d_out, uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used,
                                 int32_t* d_status, int32_t* d_detail, uint64_t span, uint64_t* d_ix_bit, uint64_t* d_ix_out, void* d_ix_win,
                                 uint32_t ix_cap, uint32_t* d_n_points, uint64_t* d_max_gap, void* stream);
int zmi_inflate_ranges_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, const uint64_t* d_ix_bit, const uint64_t* d_ix_out,
                           const void* d_ix_win, uint32_t n_points, uint64_t max_gap, const uint64_t* d_lo, const uint32_t* d_len,
                           uint32_t n_ranges, uint32_t max_len, void* d_out, const uint64_t* d_out_off, uint64_t out_stride, uint32_t* d_got,
                           int32_t* d_status, void* stream);

/* ---- multi-member gzip files: what zmi_pack_slab_dev and the exchange calls write with the gzip wrapper, bgzip / BGZF, `cat a.gz b.gz`,
 * pigz -i -- read by the reference one member after the other (libz-rs-sys/src/gz.rs:1464-1506).  Two calls, both asynchronous on
 * `stream`, neither synchronises with the host, every result is a device word.
 *
 * zmi_gzip_find_members_dev  proposals of member starts.  d_starts[0] = 0 whenever in_len > 0; every further entry is a byte offset p
 *                            with in[p .. p + 3) = 1f 8b 08, (FLG & 0xE0) == 0 and at least 18 bytes from p to the end.  Ascending and
 *                            exact: every such position, the first `cap` of them if there are more; *d_n_starts = entries written
 *                            (reading it is the caller's one synchronisation); the same entries on every run.  Any address, any
 *                            in_len below 2^45.  A proposal may be false: compressed bytes pass the filter about once in 2^27
 *                            positions (2^-24 for the three bytes, 1/8 for the flag bits), and a stored block may hold a whole gzip file.
 *                            Scratch of the context: 12 bytes per 16 KiB of input.
 * zmi_inflate_members_dev    decodes and verifies.  d_starts[0 .. n_starts): proposals, d_starts[0] = 0, strictly ascending, all below
 *                            in_len (find_members' list as it stands, or the caller's).  Proposal k owns the input up to the next
 *                            proposal (the last one to in_len); its output size is the ISIZE word that ends that range, its offset the
 *                            sum of the sizes in front: all members decode in one group of launches straight into d_out, through the
 *                            batch decoder (header incl. FEXTRA / FNAME / FCOMMENT / FHCRC, CRC-32 and ISIZE checked).
 *                            Verified are the members of the unbroken chain from offset 0: status 0, ended exactly on the next
 *                            proposal, produced exactly the planned size; the last one may end before in_len (*d_in_used tells).
 *                            After the first pass ZMI_MM_REPAIR_PASSES repair passes run, enqueued unconditionally, working from
 *                            device words (nothing to do: launches of empty streams): a member that wanted more input or room,
 *                            whose ISIZE is more than deflate can reach or whose planned region crosses out_cap drops the
 *                            proposal behind it, one that ended early exactly on a dropped proposal brings it back, offsets
 *                            are planned again and everything from the first member that failed is decoded again.  Then the first
 *                            member that still does not verify is decoded alone with all the input behind its start (at most
 *                            2^32 - 1 bytes) and all the room left: on a valid file every call verifies at least one member.
 *                            A valid file completes in ONE call if no two false proposals lie in the same member or in adjacent
 *                            members AND out_cap has room for what the first pass plans (a false proposal adds the size its
 *                            garbage ISIZE names, when deflate could reach it: with a tight out_cap a member pushed across
 *                            out_cap costs a repair pass of its own); any other valid file in a finite number of ZMI_MM_AGAIN
 *                            continuations.
 *   *d_status   0: every member to the end of the list verified.  Z_DATA_ERROR (-3): the first member that does not verify is corrupt;
 *               Z_BUF_ERROR (-5): truncated input, a member of 4 GiB or more, the output does not fit out_cap, or ZMI_MM_AGAIN;
 *               ZMI_MM_BIG also names a member whose output is above the scratch limit (only when out_cap exceeds that limit);
 *               ZMI_E_ARG (-103): d_starts[0] != 0, a list that does not ascend or reaches in_len -- the list
 *               lives on the device, so this one arrives in the status word, not as the return value.
 *               Never status 0 with wrong bytes; nothing at or behind d_out + out_cap is written.
 *   *d_detail   the case in its low 8 bits, the index (into d_starts) of the offending proposal above them.
 *               ZMI_MM_AGAIN: the passes ran out on a file that may be valid; continue at d_in + *d_in_used with the proposals
 *               behind that offset (minus it, 0 in front) -- Engine.inflate_members does.  ZMI_MM_OUT: *d_out_len holds the total
 *               the first pass planned, exact when no proposal was false.
 *   In every other case *d_members = verified members, *d_in_used = the end of the last of them, *d_out_len = their output, and the
 *   bytes d_out[0 .. *d_out_len) are right.  d_member_off (NULL or n_starts + 1 entries): the output offset of every verified member,
 *   then the total -- the random-access index of the file.
 *   Launch groups: the decode keeps one bit of scratch per byte of out_cap; an out_cap above the scratch limit
 *   (zmi_ctx_set_scratch_limit -- not the inflate-out limit, which batch callers size for their own calls) is decoded in
 *   out_cap / (limit / 2) + 1 launch groups per pass, a group holding the members planned into one window of limit / 2 bytes.
 *   Bytes and words do not depend on the limit.  A member above half the limit that shares its window with members in front does
 *   not fit its group's bitmap in the first pass; the next pass decodes from it on, where it leads its group and fits: each such
 *   member costs a repair pass, and beyond them the last resort (one member alone, up to the whole limit) and ZMI_MM_AGAIN.
 *   Event timing (zmi_ctx_get_timing): 5 = plan and group setup, 3 / 6 / 0 = decode, resolve, CRC-32, 4 = verify (the batch's and the
 *   chain's, with the repair kernels), 7 = the offset scans.
 *   in_len 0: status 0, no members, whatever n_starts is.  Scratch of the context: 88 bytes per proposal. */
#define ZMI_MM_REPAIR_PASSES 2
#define ZMI_MM_HEADER 1  /* bad member header (Z_DATA_ERROR) */
#define ZMI_MM_TRUNC 2   /* the input ends inside the member (Z_BUF_ERROR) */
#define ZMI_MM_DATA 3    /* a corrupt block (Z_DATA_ERROR) */
#define ZMI_MM_CHECK 4   /* wrong CRC-32 (Z_DATA_ERROR) */
#define ZMI_MM_LENGTH 5  /* wrong ISIZE (Z_DATA_ERROR) */
#define ZMI_MM_OUT 6     /* the output does not fit out_cap (Z_BUF_ERROR) */
#define ZMI_MM_BIG 7     /* a member of 4 GiB or more, compressed or raw, or with more output than the scratch limit (Z_BUF_ERROR) */
#define ZMI_MM_AGAIN 8   /* repair passes exhausted: continue at *d_in_used (Z_BUF_ERROR) */
int zmi_gzip_find_members_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, uint64_t* d_starts, uint32_t cap, uint32_t* d_n_starts,
                              void* stream);
int zmi_inflate_members_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, const uint64_t* d_starts, uint32_t n_starts, void* d_out,
                            uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_in_used, uint32_t* d_members, uint64_t* d_member_off,
                            int32_t* d_status, int32_t* d_detail, void* stream);

/* ---- writing BGZF: the blocked gzip file that samtools, tabix, bcftools and everything on htslib's bgzf_* seek in (the calls above
 * read it).  A block is a gzip member of at most 64 KiB that names its own size:
 *     1f 8b 08 04 | MTIME 0 0 0 0 | XFL 0 | OS ff | XLEN 06 00 | 'B' 'C' 02 00 | BSIZE u16 LE     (18 bytes; BSIZE = block size - 1)
 *     a complete raw deflate stream (BFINAL set) | CRC-32 u32 LE | ISIZE u32 LE
 * -- htslib's own header bytes -- and the file ends with the empty block
 *     1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00      (ZMI_BGZF_EOF bytes).
 * The deflate stream of a block is what zmi_deflate_batch_dev(..., ZMI_WRAP_RAW) writes for that shard (blocks of at most
 * ZMI_BGZF_BLOCK_MAX bytes are one encoder piece), so a block's bytes depend on its own bytes, level and strategy alone -- not on
 * n_blocks, its index, the alignment of the input, the scratch limit or the launch grouping.  One exception: where that stream is
 * longer than len + 5 bytes the block carries ONE stored block instead, 01 | LEN u16 | ~LEN u16 | the raw bytes (what htslib does when
 * a block overflows).  Every block is therefore at most len + 31 <= 65311 bytes and BSIZE fits, whatever the encoder's block splitting
 * does; an empty shard is the 28 bytes above (payload 03 00).
 *
 * zmi_bgzf_bound        the exact worst case: ceil(n / block_bytes) blocks of 31 + their length, plus ZMI_BGZF_EOF; block_bytes 0: 0.
 * zmi_bgzf_blocks_dev   the batch form, and a rank's building block.  Shard i = d_in[d_in_off[i] .. + d_in_len[i]), any layout, every
 *                       length <= max_len <= ZMI_BGZF_BLOCK_MAX (a larger max_len: ZMI_E_ARG; a larger d_in_len[i]: ZMI_E_ARG in
 *                       *d_status, the table lives on the device -- that shard becomes an empty block).  The blocks stand dense at
 *                       d_out + d_block_off[i]; d_block_off[n_blocks] = their total, exact whether or not they fitted;
 *                       d_block_len (NULL or n_blocks entries) = the block sizes as u32, the table zmi_exchange_sizes takes.  No
 *                       end-of-file block.  n_blocks 0: d_block_off[0] = 0, status 0.
 * zmi_bgzf_deflate_dev  a whole buffer: block i = [i * block_bytes, min(n, (i + 1) * block_bytes)), block_bytes 1 ..
 *                       ZMI_BGZF_BLOCK_MAX, n_blocks = ceil(n / block_bytes) (n 0: none, the file is the end-of-file block, as bgzip
 *                       writes), then the end-of-file block.  *d_out_len = the file's length (the size needed when it does not
 *                       fit); d_block_off (NULL or n_blocks + 1 entries): the offset of every block, then that of the end-of-file
 *                       block -- the virtual offset of raw byte u is d_block_off[u / block_bytes] << 16 | u % block_bytes.
 *   *d_status   0, or an encoder status, or Z_BUF_ERROR (-5) when the result exceeds out_cap: the blocks that end at or before
 *               out_cap are right then, a block that crosses it (and the end-of-file block, if it does) is not written, nothing at
 *               or behind d_out + out_cap is.
 *   Both calls are asynchronous on `stream` and do not synchronise with the host.  Launch groups as in zmi_deflate_stream_dev: a
 *   group's slots and match scratch stay within the scratch limit, the running offset stays in a device word; the bytes do not
 *   depend on the grouping.  Event timing: 0 = CRC-32, 1 / 5 / 2 = match search, parse, encode, 7 = sizes, scan, pack and close.
 *   Scratch of the context: at most 40 bytes per block, and one group's slots of zmi_deflate_bound(max_len, raw) bytes each. */
#define ZMI_BGZF_BLOCK_MAX 65280u   /* most input bytes per block: htslib's BGZF_BLOCK_SIZE, 0xff00 */
#define ZMI_BGZF_HEADER 18u
#define ZMI_BGZF_EOF 28u            /* the empty end-of-file block */
uint64_t zmi_bgzf_bound(uint64_t n, uint32_t block_bytes);
int zmi_bgzf_blocks_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_blocks,
                        uint32_t max_len, int level, int strategy, void* d_out, uint64_t out_cap, uint64_t* d_block_off,
                        uint32_t* d_block_len, int32_t* d_status, void* stream);
int zmi_bgzf_deflate_dev(zmi_ctx* ctx, const void* d_in, uint64_t n, uint32_t block_bytes, int level, int strategy, void* d_out,
                         uint64_t out_cap, uint64_t* d_out_len, uint64_t* d_block_off, int32_t* d_status, void* stream);

/* ---- reading ZIP archives (.zip, .npz, .whl / .jar / .docx / .xlsx): the directory, a batch inflate of entries, the CRC check --------
 * A ZIP is a batch of independent raw-deflate (method 8) or stored (method 0) streams; the size table and the CRC-32s stand in the
 * central directory at its end -- the input shape of zmi_inflate_batch_dev_ex, which checks nothing on a raw stream.  Two calls, both
 * asynchronous on `stream`, neither synchronises with the host, every result is a device word.  Positions are 64-bit, d_in may stand at
 * any alignment.  Not read: encrypted entries, methods other than 0 and 8, multi-disk archives, entries of 4 GiB or more (the batch
 * decoder's lengths are uint32_t) -- they are listed and flagged.  The archives themselves are made by zmi_zip_write_dev, below.
 *
 * zmi_zip_directory_dev   d_in[0 .. in_len) is the whole file.
 *   End record  the HIGHEST offset p in [max(0, in_len - 65557), in_len - 22] with in[p .. p + 4) = 50 4b 05 06 AND
 *               p + 22 + comment_len == in_len.  Stricter than Python's zipfile, which takes the last signature: an end record spelled
 *               inside the archive comment does not fool this one.  Bytes behind the archive are ZMI_ZA_NOEOCD, as is in_len < 22.
 *   ZIP64       where the 20-byte locator 50 4b 06 07 stands at p - 20, the 56-byte record 50 4b 06 06 at p - 76 gives count, size and
 *               offset (zipfile and Info-ZIP write the locator whenever a count field is 0xFFFF or the size or offset field
 *               0xFFFFFFFF; without a locator such fields are taken as they stand -- 65 535 entries is a valid plain archive).  A
 *               locator without that record in front of it, or a version-2 record with an extensible data sector (record size
 *               field != 44), is ZMI_ZA_ZIP64.
 *   Base        base = (start of the end structure: p, or p - 76) - cd_size - cd_off, the number of bytes that stand in front of the
 *               archive (a self-extractor, a concatenated prefix); it is added to every local-header offset.  A negative base is
 *               ZMI_ZA_BOUNDS; the directory ends exactly where the end structure begins by construction.
 *   Disks       a non-zero disk number anywhere (end record, ZIP64 record, locator, an entry's disk field; a locator that counts more
 *               than one disk) is ZMI_ZA_MULTIDISK.
 *   The chain   the bytes [base + cd_off, + cd_size): entry k starts where entry k - 1 ended, begins with 50 4b 01 02 and occupies
 *               46 + name + extra + comment bytes; the chain must end exactly at the directory's end, otherwise ZMI_ZA_CHAIN with the
 *               index of the first bad entry above the low 8 bits of detail.  n_entries = the entries walked (the good ones in front
 *               of a break); it must equal the end structure's count -- modulo 65 536 for the 16-bit field, exactly for the ZIP64
 *               record -- otherwise ZMI_ZA_COUNT.  n_listed = min(n_entries, cap): more entries than cap is no error, the first cap
 *               are listed and n_entries tells the rest (reading d_info is the caller's one synchronisation).
 *   Per entry   the fixed fields; the ZIP64 extra (id 0x0001), whose 8-byte values stand only for those of usize, csize and
 *               local-header offset -- in that order -- whose 32-bit field is 0xFFFFFFFF; then the local header at base + offset:
 *               data_off comes from the LOCAL name and extra lengths (they differ from the central ones: zipfile's force_zip64 writes
 *               a 20-byte local extra and no central one), sizes and CRC-32 always from the directory (general-purpose bit 3, the
 *               data descriptor, leaves zeros in the local header).  A flagged entry is still listed, with its name.
 *   d_info->status   0; Z_DATA_ERROR (-3) for NOEOCD / BOUNDS / CHAIN / COUNT / ZIP64; Z_VERSION_ERROR (-6) for MULTIDISK; detail = the
 *               ZMI_ZA_* case in its low 8 bits.  The 22-byte empty archive has status 0 and no entries.  With a status from the end
 *               record (all but CHAIN / COUNT and an entry's disk field) nothing is walked: n_entries = n_listed = 0.
 *   Scratch of the context: 8 bytes per entry of cap and 32 bytes per 16 KiB of in_len.  cap 0 (d_entries may be NULL) counts the entries.
 *
 * zmi_zip_inflate_dev     slot j reads entry d_sel[j] of the table d_entries[0 .. n_entries) (d_sel NULL: slot j = entry j); duplicates
 *               are allowed; an index >= n_entries -- the table lives on the device -- and an entry whose data leaves d_in or whose
 *               method and sizes no directory call would pass (a table not made from this buffer) get ZMI_E_ARG in the slot's status.
 *   Plan        d_out_off[j] = the sum of the usize of the readable slots in front, each rounded up to out_align (a power of two,
 *               1 .. 4096, otherwise ZMI_E_ARG); d_out_off[n_sel] = the room the selection needs, exact whether or not it fitted:
 *               the plan of zmi_inflate_batch_packed_dev fed from the directory instead of the size pass, and its rules for out_cap:
 *               slots that end at or before out_cap are decoded and right, the others report Z_BUF_ERROR / ZMI_ZE_OUT, nothing at or
 *               behind d_out + out_cap and nothing in the alignment gaps is written, a bitmap that cannot be reserved is ZMI_E_NOMEM.
 *   Reading     deflated slots go through the batch decoder with ZMI_WRAP_RAW and capacity usize, stored slots through the range
 *               copy; the CRC-32 kernel runs over every region; one verify kernel writes the slot's words:
 *   d_status / d_detail   0 / 0                       length and CRC-32 both match
 *               Z_DATA_ERROR / ZMI_ZE_DATA            a corrupt block
 *               Z_DATA_ERROR / ZMI_ZE_LENGTH          the decoded length is not usize, or the deflate stream does not end at byte csize
 *                                                     exactly (it wants more input, or ends early)
 *               Z_DATA_ERROR / ZMI_ZE_CHECK           CRC-32 mismatch
 *               Z_BUF_ERROR / ZMI_ZE_OUT              the region does not fit out_cap
 *               Z_VERSION_ERROR / the entry's ZMI_ZE_*    the directory flagged the entry: a region of 0 bytes
 *   d_out_len[j] = usize with status 0, 0 with every other status.  Never status 0 with wrong bytes; one bad entry does not touch its
 *   neighbours' status or bytes.  n_sel 0 writes d_out_off[0] = 0.  Bytes and words do not depend on the alignment of d_in, on the
 *   decode-kernel selection or on n_sel.  Scratch of the context: 32 bytes per slot, and the decoder's.
 *   Event timing: 5 = directory / tables and plan, 3 / 6 = decode, resolve, 0 = CRC-32, 4 = verify, 7 = stored copies. */
#define ZMI_ZA_NOEOCD 1     /* no end record that ends the file (Z_DATA_ERROR) */
#define ZMI_ZA_BOUNDS 2     /* directory size and offset do not fit in front of the end structure (Z_DATA_ERROR) */
#define ZMI_ZA_CHAIN 3      /* the directory chain breaks (Z_DATA_ERROR); index = the first bad entry */
#define ZMI_ZA_COUNT 4      /* the entries walked are not the count the end structure names (Z_DATA_ERROR) */
#define ZMI_ZA_ZIP64 5      /* a locator without a version-1 ZIP64 record of 56 bytes in front of it (Z_DATA_ERROR) */
#define ZMI_ZA_MULTIDISK 6  /* a non-zero disk number (Z_VERSION_ERROR) */
#define ZMI_ZE_LOCAL 1      /* local signature wrong; local header or data leave the file or reach into the directory; local method != central */
#define ZMI_ZE_METHOD 2     /* method not 0 / 8 */
#define ZMI_ZE_CRYPT 3      /* general-purpose bit 0 or bit 6 */
#define ZMI_ZE_BIG 4        /* a size of 4 GiB or more: the field reads 0xFFFFFFFF */
#define ZMI_ZE_EXTRA 5      /* a 32-bit field is 0xFFFFFFFF and the ZIP64 extra is missing, cut or too short */
#define ZMI_ZE_STORED 6     /* stored with csize != usize */
#define ZMI_ZE_DATA 7       /* slots only, from here on: a corrupt block */
#define ZMI_ZE_LENGTH 8
#define ZMI_ZE_CHECK 9
#define ZMI_ZE_OUT 10
typedef struct zmi_zip_entry {      /* 48 bytes */
    uint64_t data_off;   /* first data byte of the entry in d_in: behind ITS LOCAL header (30 + the local name / extra lengths); 0 where
                            the local header could not be read */
    uint64_t name_off;   /* first byte of its name in d_in (inside the central directory), name_len bytes */
    uint32_t csize, usize;            /* 0xFFFFFFFF together with ZMI_ZE_BIG when 4 GiB or more */
    uint32_t crc32, dos_time /* date << 16 | time */, ext_attr;
    uint16_t method, flags, name_len, reserved /* 0 */;
    int32_t  status;     /* 0: readable by zmi_zip_inflate_dev; otherwise the ZMI_ZE_* reason, known from the directory alone (the first
                            that holds of EXTRA, BIG, LOCAL, CRYPT, METHOD, STORED) */
} zmi_zip_entry;
typedef struct zmi_zip_info {       /* 48 bytes */
    uint64_t n_entries, n_listed, cd_off, cd_size, base;
    int32_t status, detail;
} zmi_zip_info;
uint32_t zmi_zip_walk_tile(void);   /* bytes of directory one window of the chain walk holds (for tests that place entries around it) */
int zmi_zip_directory_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, zmi_zip_entry* d_entries, uint32_t cap, zmi_zip_info* d_info,
                          void* stream);
int zmi_zip_inflate_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, const zmi_zip_entry* d_entries, uint32_t n_entries,
                        const uint32_t* d_sel, uint32_t n_sel, uint32_t out_align, void* d_out, uint64_t out_cap,
                        uint64_t* d_out_off /* n_sel + 1 */, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, void* stream);

/* ---- writing ZIP archives: entries from device memory into a .zip / .npz / .whl / .jar, directory and ZIP64 forms included -------------
 * Entry i = d_in[d_in_off[i] .. + d_in_len[i]), any layout; its name = d_names[d_name_off[i] .. d_name_off[i + 1]), bytes the caller promises
 * to be UTF-8 (nothing validates them).  d_out[0] stands at file position `base` -- the bytes already written in front, a self-extractor
 * stub -- and every position written INTO the archive is absolute, base + its place in d_out: local-header offsets, the directory offset,
 * the ZIP64 record's offset in the locator (the form zmi_zip_directory_dev computes a base of 0 for).  Every byte is fixed:
 *   local header    50 4b 03 04 | need u16 | flags u16 | method u16 | time u16 | date u16 | crc32 | csize u32 | usize u32 | name_len u16 |
 *                   00 00 | name           (30 + name bytes, never an extra field; sizes and CRC-32 stand here: no data descriptor, bit 3
 *                   clear).  method 8 / need 20 at levels 1 .. 9, method 0 / need 10 at level 0 for EVERY entry: the payload is then
 *                   the raw bytes (a stored entry, not deflate stored blocks; the encoder does not run).  flags = 0x0800 where the
 *                   name holds a byte >= 0x80, else 0.  No per-entry fallback to method 0 at levels 1 .. 9 (incompressible data has
 *                   csize > usize); an empty entry there is 03 00, csize 2 -- both as Python's zipfile does.
 *   payload         levels 1 .. 9: the entry is cut into pieces of piece_bytes (the last may be shorter), each compressed as an independent
 *                   piece of ONE raw stream, as zmi_deflate_pieces_dev(ZMI_STREAM_INDEPENDENT) does with max_len = piece_bytes: every
 *                   piece but the entry's last ends with the flush marker, the last ends the stream.  An entry's bytes are a function
 *                   of (its bytes, piece_bytes, level, strategy) alone -- not of n_entries, its index, the alignment, the scratch limit,
 *                   in_bytes or the launch grouping.  (Pieces are independent: smaller piece_bytes costs ratio, as documented for
 *                   zmi_deflate_stream_dev; and a piece_bytes shard is encoded in up to 16 regions, so entries far smaller than
 *                   piece_bytes pay for a large piece_bytes too -- choose it near the typical entry when the entries are small.)
 *   central record  50 4b 01 02 | made_by u16 = 0x0300 | need | need u16 | flags | method | time | date | crc32 | csize | usize | name_len |
 *                   extra_len u16 | comment_len 0 | disk 0 | int_attr 0 | ext_attr u32 | offset u32 | name [| 01 00 08 00 | offset u64]
 *                   (46 + name (+ 12) bytes).  Where the absolute local-header offset is >= 0xFFFFFFFF the field is all ones, the 12-byte
 *                   ZIP64 extra carries the offset and need is 45 (in this record; the local header keeps 20 / 10).  Sizes never need
 *                   the extra: see ZMI_ZIP_ENTRY_MAX.
 *   end             the ZIP64 form where n_entries >= 0xFFFF, or the directory's size >= 0xFFFFFFFF, or its absolute offset >= 0xFFFFFFFF:
 *                   50 4b 06 06 | 44 u64 | 0x032D u16 | 45 u16 | 0 u32 | 0 u32 | n u64 | n u64 | cd_size u64 | cd_off u64   (56 bytes), then
 *                   50 4b 06 07 | 0 u32 | that record's offset u64 | 1 u32                                                  (20 bytes);
 *                   then always 50 4b 05 06 | 0 u16 | 0 u16 | min(n, 0xFFFF) u16 x 2 | min(cd_size, 0xFFFFFFFF) u32 |
 *                   min(cd_off, 0xFFFFFFFF) u32 | 00 00 (22 bytes).  No comments anywhere.
 *   d_dos_time      one uint32_t per entry, date << 16 | time as in zmi_zip_entry; NULL: 0x00210000 (1980-01-01 00:00:00), which gives
 *                   reproducible archives.  d_ext_attr: one uint32_t per entry; NULL: 0x81A40000 (a regular file, 0644).
 *
 * zmi_zip_bound       room that always suffices for n_entries entries whose names are names_bytes and whose data is in_bytes in all
 *                     (not tight); piece_bytes 0: 0.
 * zmi_zip_write_dev   asynchronous on `stream`, never synchronises with the host, every result is a device word.
 *   Arguments   piece_bytes 1 .. 2^30, level -1 .. 9, strategy 0 .. 4, n_entries <= 2^31 - 1, otherwise ZMI_E_ARG as the return value.
 *               in_bytes is the caller's bound on the sum of d_in_len, normally the size of the buffer the entries lie in: it sizes the
 *               piece table, n_entries + in_bytes / piece_bytes places (more than 2^31 - 1: ZMI_E_ARG) -- the host cannot know the
 *               true count, the lengths live on the device.  A larger sum is ZMI_E_ARG in *d_status and no entry is written: the
 *               result is the 22-byte empty archive.
 *   Per entry   (the tables are device data) a length above ZMI_ZIP_ENTRY_MAX becomes an empty entry, a name longer than 65 535 bytes is
 *               cut to its first 65 535, either with ZMI_E_ARG in *d_status.  Every piece adds a flush marker and a block header to
 *               its entry, so hundreds of MB of incompressible bytes cut into pieces of a few bytes can pass 2^32 compressed bytes:
 *               such an entry is ZMI_E_ARG in *d_status too, its size fields are all ones and the archive is not a valid one.
 *               *d_status is otherwise 0, or the first encoder status.
 *   Capacity    an archive longer than out_cap: *d_status = Z_BUF_ERROR (-5; behind an earlier status that one stays).  *d_out_len is
 *               always the archive's length -- the room it needs when it does not fit.  Payloads and records (a local header with
 *               its name, a central record, each of the three end records) that end at or before out_cap are right, one that crosses
 *               it is not written, nothing at or behind d_out + out_cap is.
 *   d_entries   NULL, or n_entries rows: the table zmi_zip_directory_dev would list for the finished archive -- every field, name_off
 *               pointing into the written directory, status 0; positions are places in d_out.  d_info: NULL, or the matching
 *               zmi_zip_info, with cd_off the directory's place in d_out and base 0 (at base 0 exactly what the reader reports).
 *   n_entries 0 gives the 22-byte empty archive.
 *   Launch groups as in zmi_deflate_stream_dev: a group's slots and match scratch stay within the scratch limit, the running offset
 *   stays in a device word, an entry may lie across groups; the bytes do not depend on the grouping.  A slot holds one piece of
 *   min(piece_bytes, in_bytes) bytes, so one large entry beside many small ones costs slots of piece_bytes, not of the entry.
 *   Event timing: 0 = CRC-32 (pieces, then the fold per entry), 1 / 5 / 2 = match search, parse, encode, 7 = layout, sizes, scans,
 *   pack, headers, directory and close.
 *   Scratch of the context: 36 bytes per entry, 40 bytes and 1 bit per place of the piece table, and one group's slots of
 *   zmi_deflate_pieces_stride(min(piece_bytes, in_bytes)) bytes each (pieces below ~17 KiB under a piece_bytes above 64 KiB: up to
 *   2.2 KiB more, the room of that geometry's regions). */
#define ZMI_ZIP_ENTRY_MAX 0xF0000000u   /* most bytes per entry: the encoder's worst case of it (stored blocks) still fits 32 bits */
uint64_t zmi_zip_bound(uint32_t n_entries, uint64_t names_bytes, uint64_t in_bytes, uint32_t piece_bytes, int level);
int zmi_zip_write_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_entries,
                      uint64_t in_bytes, const void* d_names, const uint64_t* d_name_off /* n_entries + 1 */,
                      const uint32_t* d_dos_time /* NULL */, const uint32_t* d_ext_attr /* NULL */, uint32_t piece_bytes, int level,
                      int strategy, uint64_t base, void* d_out, uint64_t out_cap, uint64_t* d_out_len,
                      zmi_zip_entry* d_entries /* NULL or n_entries */, zmi_zip_info* d_info /* NULL */, int32_t* d_status, void* stream);

/* ---- reading PNG images: the chunk chain, a batch inflate of the IDAT streams, the scanline unfilter ------------------------------------
 * A PNG is a chain of chunks (length u32 BE | type | data | CRC-32 of type + data, W3C PNG third edition section 5.3; RFC 2083
 * section 3.2) behind an eight-byte signature (5.2); the image is one zlib stream cut into consecutive IDAT chunks (10.1, 11.2.4) that
 * inflates to `height` scanlines of 1 filter byte + row_bytes bytes (7.2, 9.2).  Two calls, both asynchronous on `stream`, neither
 * synchronises with the host, every per-image failure is a status word.  Image i is the file d_in[d_in_off[i] .. + d_in_len[i]), at
 * any alignment.  PNG is not part of the reference project: the contract is the specification.  Not read: Adam7 (8.2), images whose
 * scanlines reach 4 GiB (the batch decoder's lengths are uint32_t); APNG frames, gamma and ICC are not looked at.  Writing: further down.
 *
 * zmi_png_headers_dev   one zmi_png_image per file.  The first rule that holds, in this order, is the record's status:
 *   ZMI_PE_SIGNATURE    the eight bytes 89 50 4e 47 0d 0a 1a 0a are wrong (5.2)
 *   ZMI_PE_IHDR         the first chunk is not a 13-byte IHDR; a dimension of 0 or above 2^31 - 1; a depth / colour type pair outside
 *                       table 11.1 (11.2.2); compression or filter method not 0; interlace method above 1
 *   ZMI_PE_INTERLACE    interlace method 1: listed with its dimensions, flagged, not decoded (the chain is then not walked)
 *   ZMI_PE_TRUNC        a chunk length above 2^31 - 1 (5.3), a chunk that leaves the file, no IEND before the file ends
 *   ZMI_PE_CRITICAL     an unknown chunk whose first letter is upper case (5.4)
 *   ZMI_PE_ORDER        no IDAT; IDAT chunks that are not consecutive; PLTE missing for colour type 3, PLTE behind IDAT, a PLTE length
 *                       not a multiple of 3 or above 768 (5.6, 11.2.3); a second IHDR
 *   ZMI_PE_BIG          (1 + row_bytes) * height does not fit 32 bits
 *   Ancillary chunks are skipped unread -- acTL, fcTL and fdAT too, so the default image of an APNG decodes; tRNS (11.3.2.1) is only
 *   located.  Bytes behind IEND are ignored.
 *
 * zmi_png_decode_dev    slot j decodes image d_sel[j] of the table d_images[0 .. n_images) (d_sel NULL: slot j = image j); duplicates
 *               are allowed; an index >= n_images, and a record no headers call would write for this file (the IDAT run it names --
 *               idat_pos + 12 * n_idat + idat_bytes -- and the IEND behind it leave the file, a size of 0), get ZMI_E_ARG in the
 *               slot's status and nothing of them is read.
 *   Region      height * row_bytes bytes: the unfiltered scanlines, no filter bytes, no row padding.  Depth 8 is an [H, W, C] byte
 *               tensor as it stands; samples below 8 bits stay packed (7.2); 16-bit samples stay big-endian unless
 *               flags & ZMI_PNG_NATIVE16, with which the unfilter's own store writes them little-endian.
 *   Plan        d_out_off, out_align, out_cap as zmi_inflate_batch_packed_dev: d_out_off[j] = the sum of the region sizes of the
 *               readable slots in front, each rounded up to out_align (a power of two, 1 .. 4096, otherwise ZMI_E_ARG);
 *               d_out_off[n_sel] = the room the selection needs whether or not it fitted; a slot that ends behind out_cap reports
 *               Z_BUF_ERROR / ZMI_PE_OUT; nothing at or behind d_out + out_cap and nothing in the gaps is written.  A flagged or failed
 *               slot takes no room (a failed one: the room the plan gave it), has length 0, and raises nothing.
 *   Reading     one workgroup walk per slot checks the CRC-32 of IHDR, PLTE, every IDAT and IEND (never an ancillary chunk's;
 *               flags & ZMI_PNG_NO_CRC skips it) and gathers the payloads of several IDAT chunks into one stream in context scratch
 *               (a single IDAT is read in place); the batch decoder runs with ZMI_WRAP_ZLIB and capacity (1 + row_bytes) * height
 *               into scratch, which checks the Adler-32; the unfilter kernel (9.2: None, Sub, Up, Average on a 9-bit sum, Paeth with
 *               ties in the order a, b, c; every neighbour outside the image is 0) writes the region; one kernel writes the slot's
 *               words, the first of these that holds:
 *   d_status / d_detail   Z_DATA_ERROR / the record's ZMI_PE_*     flagged by the headers call (Z_VERSION_ERROR for INTERLACE and BIG)
 *               Z_BUF_ERROR / ZMI_PE_OUT        the region does not fit out_cap
 *               Z_MEM_ERROR / ZMI_PE_SCRATCH    the gathered streams of the call exceed its scratch, see below
 *               Z_DATA_ERROR / ZMI_PE_CRC       a wrong CRC-32 in a critical chunk
 *               Z_DATA_ERROR / ZMI_PE_DATA      a corrupt zlib stream, a wrong Adler-32, FDICT set
 *               Z_DATA_ERROR / ZMI_PE_LENGTH    the stream ends before or behind exactly (1 + row_bytes) * height bytes.  libpng only
 *                                               warns about surplus image data ("Too much image data"); this call refuses it
 *               Z_DATA_ERROR / ZMI_PE_FILTER    a filter byte above 4 (9.2); the region's bytes are then unspecified
 *   Bytes behind the end of the zlib stream but inside the IDAT payload are no error (libpng and PIL accept them).
 *   d_out_len[j] = height * row_bytes with status 0, otherwise 0.  Never status 0 with wrong bytes; one bad image does not touch its
 *   neighbours.  n_sel 0 writes d_out_off[0] = 0.  Bytes and words do not depend on the alignment of d_in, on n_images, on the slot
 *   index or on the decode-kernel selection.
 *   Scratch of the context, sized from out_cap and n_sel because no size of the input is known to the host: 88 bytes per slot; the
 *   filtered scanlines, 2 * out_cap + 16 bytes per slot (1 + row_bytes <= 2 * row_bytes) -- so out_cap should be the room the batch
 *   needs, not a large buffer kept for reuse; the gathered streams of the images with more than one IDAT, min(2.125 * out_cap + 1 KiB
 *   per slot + 64 KiB, the context's scratch limit) -- the streams are planned in slot order, and every slot whose stream does not end
 *   inside that room (a call whose multi-IDAT payloads EXPAND their scanlines by more than 6 % in total, by junk behind the streams for
 *   instance) reports ZMI_PE_SCRATCH, keeps its room and has length 0; and the decoder's, sized by this call from out_cap whatever the
 *   context's limits are.  Scratch that cannot be reserved is ZMI_E_NOMEM.
 *   Event timing: 5 = slot tables and plans, 0 = the walk (chunk CRC-32 and gather), 7 = unused (the gather is fused into the
 *   walk), 3 / 6 = decode, resolve (the decoder's own Adler-32 pass adds to 0, its verify to 4), 2 = the unfilter (the encoder's slot is
 *   idle on every read path), 4 = the slot words. */
#define ZMI_PE_SIGNATURE 1   /* Z_DATA_ERROR */
#define ZMI_PE_IHDR 2        /* Z_DATA_ERROR */
#define ZMI_PE_INTERLACE 3   /* Z_VERSION_ERROR */
#define ZMI_PE_TRUNC 4       /* Z_DATA_ERROR */
#define ZMI_PE_CRITICAL 5    /* Z_DATA_ERROR */
#define ZMI_PE_ORDER 6       /* Z_DATA_ERROR */
#define ZMI_PE_BIG 7         /* Z_VERSION_ERROR */
#define ZMI_PE_CRC 8         /* slots only, from here on: Z_DATA_ERROR */
#define ZMI_PE_DATA 9
#define ZMI_PE_LENGTH 10
#define ZMI_PE_FILTER 11
#define ZMI_PE_OUT 12        /* Z_BUF_ERROR */
#define ZMI_PE_SCRATCH 13    /* Z_MEM_ERROR */
#define ZMI_PNG_NATIVE16 1u  /* flags: 16-bit samples leave little-endian */
#define ZMI_PNG_NO_CRC 2u    /* flags: no chunk CRC-32 is checked */
typedef struct zmi_png_image {      /* 48 bytes */
    uint32_t width, height;           /* IHDR (11.2.2); 0 where the record's status is SIGNATURE or IHDR */
    uint8_t  depth, colour, channels; /* bit depth 1 / 2 / 4 / 8 / 16, colour type 0 / 2 / 3 / 4 / 6, samples per pixel 1 .. 4 */
    uint8_t  bpp;                     /* the filters' pixel distance: max(1, channels * depth / 8) (9.2) */
    uint32_t row_bytes;               /* ceil(width * channels * depth / 8); 0xFFFFFFFF together with ZMI_PE_BIG where that is 4 GiB or more */
    uint32_t idat_pos;                /* position in the file of the first IDAT chunk (of its length field) */
    uint32_t n_idat, idat_bytes;      /* the consecutive IDAT chunks from there, and the sum of their payload lengths */
    uint32_t plte_pos, plte_len;      /* position of the PLTE chunk's DATA in the file and its length; 0, 0 if absent */
    uint32_t trns_pos, trns_len;      /* the same for tRNS */
    int32_t  status;                  /* 0: readable by zmi_png_decode_dev; otherwise the ZMI_PE_* reason */
} zmi_png_image;
uint32_t zmi_png_strip(void);       /* bytes of a scanline one LDS strip of the unfilter kernel holds (for tests that place row_bytes around it) */
int zmi_png_headers_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_images,
                        zmi_png_image* d_images, void* stream);
int zmi_png_decode_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                       const zmi_png_image* d_images, uint32_t n_images, const uint32_t* d_sel, uint32_t n_sel, uint32_t flags,
                       uint32_t out_align, void* d_out, uint64_t out_cap, uint64_t* d_out_off /* n_sel + 1 */, uint32_t* d_out_len,
                       int32_t* d_status, int32_t* d_detail, void* stream);

/* ---- writing PNG images: the scanline filter with a choice per row, deflate in pieces, the chunks ------------------------------------------
 * The inverse of the two calls above: a batch of images in device memory becomes a batch of complete PNG files in device memory, one
 * asynchronous call on `stream` that never synchronises with the host; every per-image failure is a status word.  Not written: colour
 * type 3 (PLTE / tRNS), Adam7, ancillary chunks, APNG, several IDAT chunks per image; one level, strategy and filter mode per call.
 *
 *   Input       image i is the pixels d_in[d_in_off[i] .. + d_in_len[i]) at any alignment -- exactly the region zmi_png_decode_dev writes:
 *               height * row_bytes bytes, no filter bytes, no row padding.  Samples below 8 bits are packed, padding bits are taken as
 *               they stand.  16-bit samples are big-endian, or little-endian under flags & ZMI_PNG_NATIVE16 (the filter kernel's own
 *               load swaps them; there is no extra pass).  Any other flag: ZMI_E_ARG.
 *   d_images    of d_images[i] only width, height, depth and colour are read; channels, bpp and row_bytes are recomputed, so a table
 *               from zmi_png_headers_dev can be encoded again as it stands and a caller may fill just four fields.  The table is device
 *               data: every violation is ZMI_E_ARG in d_status[i] -- length 0, no room taken, neighbours untouched, nothing of the image
 *               read --, the first of these that holds: a dimension of 0 or above 2^31 - 1; a depth / colour pair outside table 11.1;
 *               colour type 3; (1 + row_bytes) * height above ZMI_PNG_SCAN_MAX; d_in_len[i] != height * row_bytes.
 *   scan_bytes  the caller's bound on the sum of (1 + row_bytes) * height over the valid images (the lengths live on the device: what
 *               in_bytes is to zmi_zip_write_dev).  It sizes the piece table, n_images + scan_bytes / piece_bytes places (more than
 *               2^31 - 1: ZMI_E_ARG as the return value), and the scanline scratch.  A larger true sum is ZMI_E_ARG in every slot:
 *               nothing is written, every d_out_off word is 0.
 *   File        every byte is fixed, one IDAT per image:
 *                 89 50 4e 47 0d 0a 1a 0a | 00 00 00 0d "IHDR" width height depth colour 00 00 00 crc |
 *                 len "IDAT" zlib-stream crc | 00 00 00 00 "IEND" ae 42 60 82
 *               The zlib stream: the two header bytes zmi_deflate_stream_dev writes for ZMI_WRAP_ZLIB at that level and strategy; the
 *               filtered scanlines cut into pieces of piece_bytes, each compressed as an independent piece of ONE raw stream exactly
 *               as zmi_deflate_pieces_dev(ZMI_STREAM_INDEPENDENT) does with max_len = piece_bytes -- every piece but the last ends with
 *               the flush marker, the last ends the stream --; the big-endian Adler-32 of the filtered scanlines.  Level 0 is deflate
 *               stored blocks through the same path (PNG has no "stored" method).  A file's bytes are a function of (its pixels and
 *               four fields, flags, filter, piece_bytes, level, strategy) alone -- not of n_images, its index, the alignment of d_in,
 *               out_align, the scratch limit or the launch grouping.  An image whose IDAT data (the stream with its 6 bytes of frame)
 *               passes 2^31 - 1 bytes is ZMI_E_ARG too (its length is computed in 64 bits; the room the plan gave it stays taken).
 *               Otherwise d_status[i] is 0, Z_BUF_ERROR, or the first encoder status of its pieces.
 *   Filter      filter 0 .. 4: that type (9.2: None, Sub, Up, Average on a 9-bit sum, Paeth with ties in the order a, b, c) on every
 *               row.  ZMI_PNG_FILTER_ADAPTIVE: per row the type whose filtered bytes v have the least sum of (v < 128 ? v : 256 - v)
 *               over the row's row_bytes bytes (the minimum sum of absolute differences of 12.7, exact, 64-bit), the SMALLEST type
 *               among those of least cost -- on row 0 None therefore beats Up and Sub beats Paeth, which always tie there.  The
 *               neighbours are raw bytes, every one outside the image is 0.  filter above 5: ZMI_E_ARG as the return value.
 *   Plan        d_out_off[i] = the sum of the file lengths of the valid images in front, each rounded up to out_align (a power of two,
 *               1 .. 4096, otherwise ZMI_E_ARG); d_out_off[n_images] = the room the batch needs whether or not it fitted.  A file that
 *               ends at or before out_cap is complete with status 0; one that crosses it has Z_BUF_ERROR and length 0 (pieces of it
 *               that end in front of out_cap may have been written).  Nothing at or behind d_out + out_cap and nothing in the alignment
 *               gaps is written.  d_out_len[i] = the file's length with status 0, otherwise 0.  n_images 0 writes d_out_off[0] = 0.
 *   d_written   NULL, or n_images rows: the table zmi_png_headers_dev would list for the written files -- every field, status 0 --;
 *               the row of an image whose status is not 0 is all zeros with that status.
 *   zmi_png_bound   room that always suffices (not tight); piece_bytes 0: 0.
 *   Arguments   piece_bytes 1 .. 2^30, level -1 .. 9, strategy 0 .. 4, n_images <= 2^31 - 1, otherwise ZMI_E_ARG as the return value.
 *   Launch groups as in zmi_zip_write_dev: a group's slots and match scratch stay within the scratch limit, the running offset stays in
 *   a device word, an image may lie across groups; the bytes do not depend on the grouping.
 *   Scratch of the context: the filtered scanlines, scan_bytes + 128 bytes, NOT capped by the scratch limit (all images are filtered
 *   before the first group is encoded); 48 bytes per image, 40 bytes and 1 bit per place of the piece table, 12 bytes per slot of a
 *   group; one group's slots as in zmi_zip_write_dev.  Scratch that cannot be reserved is ZMI_E_NOMEM.
 *   Event timing: 3 = the filter kernel (the decoder's slot is idle on every write path, as the encoder's is where the reader put its
 *   unfilter), 0 = Adler-32 of the scanline pieces, CRC-32 of the compressed pieces, the folds per image, 1 / 5 / 2 = match search, parse,
 *   encode, 7 = layout, scans, the piece table, places and pack, 4 = the files' fixed bytes and the images' words. */
#define ZMI_PNG_FILTER_ADAPTIVE 5u      /* filter: 0 .. 4 = that type on every row (9.2), 5 = per row, see above */
#define ZMI_PNG_SCAN_MAX 0x7F000000u    /* most filtered bytes per image: 16 MiB below 2^31, which holds the encoder's worst case (stored
                                           blocks, a marker per piece) for pieces of 64 KiB and more; smaller pieces: see File */
uint32_t zmi_png_filter_tile(void);     /* bytes of a scanline one trip of the filter kernel covers per wave (for tests that place row_bytes around it) */
uint64_t zmi_png_bound(uint32_t n_images, uint64_t scan_bytes, uint32_t piece_bytes, uint32_t out_align, int level);
int zmi_png_encode_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                       const zmi_png_image* d_images, uint32_t n_images, uint64_t scan_bytes, uint32_t flags, uint32_t filter,
                       uint32_t piece_bytes, int level, int strategy, uint32_t out_align, void* d_out, uint64_t out_cap,
                       uint64_t* d_out_off /* n_images + 1 */, uint32_t* d_out_len, zmi_png_image* d_written /* NULL or n_images */,
                       int32_t* d_status, void* stream);

/* ---- reading TIFF files with Deflate compression: the IFD chain, a batch inflate of strips or tiles, the predictor undo ----------------
 * A TIFF is a header (TIFF 6.0 section 2: II or MM, magic 42, the offset of the first image file directory) and a chain of IFDs, one a
 * page: a count, entries of tag | type | count | value-or-offset, the offset of the next IFD, 0 at the end.  BigTIFF, as libtiff reads
 * it: magic 43, offset size 8, a reserved 0, 64-bit offsets and counts, entries of 20 bytes, an 8-byte entry count.  A page is cut
 * into strips (section 3) or tiles (section 15), every segment compressed on its own -- Deflate is compression 8 of the Adobe Photoshop
 * TIFF Technical Notes, 32946 the older code for the same zlib stream -- and the file holds the table of the segments' offsets and byte
 * counts.  Behind the decoder stands the predictor: horizontal differencing (section 14) or the floating-point predictor of Adobe
 * Technical Note 3.  Two calls, both asynchronous on `stream`, neither synchronises with the host, every per-file and per-segment
 * failure is a device word; positions are 64-bit and d_in may stand at any alignment.  TIFF is not part of the reference project: the
 * contract is these documents.  Not read: LZW, JPEG, ZSTD, LERC, PackBits; PlanarConfiguration 2; depths below 8; SubIFDs (tag 330 is
 * not followed); YCbCr subsampling and colour maps (the photometric value is listed, nothing more); segments of 4 GiB or more.
 *
 * zmi_tiff_directory_dev   takes the whole file d_in[0 .. in_len).  *d_info: status 0, or Z_DATA_ERROR with detail
 *   ZMI_TA_HEADER       not II / MM with magic 42, or magic 43 with offset size 8 and a reserved word of 0
 *   ZMI_TA_CHAIN | index << 8    IFD number `index` leaves the file, has 0 entries, or stands behind ZMI_TIFF_PAGES_MAX IFDs already
 *                       walked (the guard against a chain that loops); a first-IFD offset of 0 is index 0.  The IFDs in front of it
 *                       are counted and listed all the same.
 *   n_pages = the IFDs walked, n_listed = min(n_pages, cap): more pages than cap is no error, and cap 0 counts.  One lane follows the
 *   chain; the tags of the listed pages are read by a thread per page, in whatever order they stand (real writers do not keep them
 *   ascending; of a tag that stands twice the first counts): 256 ImageWidth, 257 ImageLength, 258 BitsPerSample, 259 Compression, 262
 *   PhotometricInterpretation, 273 StripOffsets, 277 SamplesPerPixel, 278 RowsPerStrip, 279 StripByteCounts, 284 PlanarConfiguration,
 *   317 Predictor, 322 TileWidth, 323 TileLength, 324 TileOffsets, 325 TileByteCounts, 338 ExtraSamples (its count only), 339
 *   SampleFormat (its first value).  Defaults (section 8): BitsPerSample 1, SamplesPerPixel 1, Compression 1, RowsPerStrip 2^32 - 1,
 *   PlanarConfiguration 1, Predictor 1, SampleFormat 1.  Scalars may be BYTE, SHORT, LONG or LONG8, the two arrays SHORT, LONG or LONG8;
 *   a value that fits the entry's value field (4 bytes, BigTIFF 8) stands there, and the record keeps the file position of the value
 *   bytes either way.  The record's status is the first of these that holds:
 *   ZMI_TP_TAGS         width, height or one of the segment tags is missing; both or neither of the strip tags (273, 279) and the tile
 *                       tags (322 .. 325) are present; an array's count is not n_segs; an array or a read value leaves the file or has
 *                       another type; a dimension, a tile size or RowsPerStrip is 0                                   (Z_DATA_ERROR)
 *   ZMI_TP_FORMAT       BitsPerSample differs between samples; a depth that is not 8 / 16 / 32 / 64; predictor 3 with a SampleFormat
 *                       other than 3 or a depth below 16; predictor 0 or above 3; samples 0 or above 8             (Z_DATA_ERROR)
 *   ZMI_TP_COMPRESSION  anything but 1, 8 and 32946                                                                (Z_VERSION_ERROR)
 *   ZMI_TP_PLANAR       PlanarConfiguration 2                                                                      (Z_VERSION_ERROR)
 *   ZMI_TP_BIG          seg_bytes does not fit 32 bits: the field reads 0xFFFFFFFF                                 (Z_VERSION_ERROR)
 *   A flagged page is listed with what was read of it; the geometry fields of a ZMI_TP_TAGS page are 0.
 *
 * zmi_tiff_read_dev     slot j reads segment d_sel[j] of page `page` of the table d_pages[0 .. n_pages) (d_sel NULL: slot j = segment
 *               j); segments are numbered row by row, duplicates are allowed.  An index >= the page's n_segs, a page index >= n_pages
 *               and a record no directory call would write for a file of in_len bytes (arrays that leave it, sizes that do not follow
 *               from the fields) get ZMI_E_ARG in the slot's status, and nothing of them is read.
 *   Region      default (dense): rows * seg_w * samples * sample_bytes bytes, rows = seg_h but for the last strip of a page, which has
 *               the rows left, height - k * seg_h: the decoded segment with the predictor undone and every sample in the machine's
 *               little-endian order whatever the file's, a [rows, seg_w, C] tensor as it stands; edge tiles keep their padding columns
 *               and rows.  d_out_off, out_align, out_cap as zmi_png_decode_dev: d_out_off[j] = the sum of the region sizes of the
 *               slots in front that read a segment, each rounded up to out_align (a power of two, 1 .. 4096, otherwise ZMI_E_ARG);
 *               d_out_off[n_sel] = the room the selection needs whether or not it fitted; a slot that ends behind out_cap reports
 *               Z_BUF_ERROR / ZMI_TE_OUT; nothing at or behind d_out + out_cap and nothing in the gaps is written.  A flagged page
 *               and a bad index take no room, a failed segment keeps the room the plan gave it.
 *   flags & ZMI_TIFF_ASSEMBLE   the output is the page as ONE [height, width, C] image of height * width * samples * sample_bytes
 *               bytes at d_out: every selected segment is written at its place, cropped at the right and the bottom edge; what no
 *               selected segment covers is left untouched.  d_out_off[j] = the byte offset of the segment's first pixel,
 *               d_out_off[n_sel] = the image's size (0 where the page is not readable); an image that does not fit out_cap is
 *               Z_BUF_ERROR / ZMI_TE_OUT in every slot; out_align is ignored.  d_out_len[j] = the bytes of the cropped segment.
 *   decoded_bytes   the caller's bound on the sum of the decoded sizes (the dense region sizes, in either mode) of the slots that
 *               read a segment -- what scan_bytes is to zmi_png_encode_dev: it sizes the scratch that holds the still-predicted
 *               bytes.  A larger true sum is ZMI_E_ARG in every slot, and nothing is written.
 *   Reading     one kernel reads offset and byte count of every slot from the file's two arrays, in the file's byte order and the
 *               array's value type.  Compression 8 / 32946 goes through the batch decoder with ZMI_WRAP_ZLIB and capacity = the decoded
 *               size into scratch, which checks the Adler-32; compression 1 goes through the range copy.  A segment with byte count 0
 *               is sparse (GDAL writes missing tiles so): its region is zero bytes, its status 0, its detail ZMI_TE_SPARSE.  The
 *               unpredict kernel writes the regions: predictor 1 copies (MM files: the bytes of every sample swapped); predictor 2
 *               (section 14) is x[i] = d[i] + x[i - samples] mod 2^(8 * sample_bytes) along a row, d read in the file's byte order,
 *               integer arithmetic on the bits whatever SampleFormat says; predictor 3 (Technical Note 3) is p[i] = q[i] +
 *               p[i - samples] mod 256 over the row's bytes, after which byte b of sample k is p[b * seg_w * samples + k], b = 0 the
 *               most significant in II and MM files alike.  One kernel writes the slot's words, the first of these that holds:
 *   d_status / d_detail   Z_DATA_ERROR or Z_VERSION_ERROR / the record's ZMI_TP_*   the page is flagged (see above)
 *               Z_BUF_ERROR / ZMI_TE_OUT        the region (assemble: the image) does not fit out_cap
 *               Z_DATA_ERROR / ZMI_TE_BOUNDS    offset + byte count leaves the file, or the byte count is 4 GiB or more
 *               0 / ZMI_TE_SPARSE               byte count 0
 *               Z_DATA_ERROR / ZMI_TE_DATA      a corrupt zlib stream, a wrong Adler-32, FDICT set
 *               Z_DATA_ERROR / ZMI_TE_LENGTH    the stream -- compression 1: the byte count -- ends before or behind exactly the decoded
 *                                               size.  Bytes behind the end of the zlib stream but inside the byte count are no error
 *                                               (libtiff accepts them).
 *   d_out_len[j] = the region's size with status 0, otherwise 0.  Never status 0 with wrong bytes; one bad segment does not touch its
 *   neighbours.  n_sel 0 writes d_out_off[0] = 0 and nothing else.  Bytes and words do not depend on the alignment of d_in, on n_sel,
 *   on the slot index or on the decode-kernel selection.
 *   Scratch of the context: 8 bytes per page of cap (the directory call); 96 bytes per slot; the still-predicted bytes, decoded_bytes
 *   + 16 bytes per slot + 96; and the decoder's, sized by this call from decoded_bytes.  Scratch that cannot be reserved is ZMI_E_NOMEM.
 *   Event timing: 5 = directory; slot tables and plans, 3 / 6 = decode, resolve (the decoder's own Adler-32 pass adds to 0, its verify
 *   to 4), 7 = the copies of compression 1, 2 = the unpredict (the encoder's slot is idle on every read path: where the PNG reader put
 *   its unfilter), 4 = the slot words. */
#define ZMI_TA_HEADER 1      /* zmi_tiff_info.detail & 0xFF, status Z_DATA_ERROR */
#define ZMI_TA_CHAIN 2       /* ... the index of the first bad IFD above the low 8 bits */
#define ZMI_TP_TAGS 1        /* zmi_tiff_page.status and the slot's detail: Z_DATA_ERROR */
#define ZMI_TP_FORMAT 2      /* Z_DATA_ERROR */
#define ZMI_TP_COMPRESSION 3 /* Z_VERSION_ERROR */
#define ZMI_TP_PLANAR 4      /* Z_VERSION_ERROR */
#define ZMI_TP_BIG 5         /* Z_VERSION_ERROR */
#define ZMI_TE_OUT 6         /* slots only, from here on: Z_BUF_ERROR */
#define ZMI_TE_BOUNDS 7      /* Z_DATA_ERROR */
#define ZMI_TE_DATA 8
#define ZMI_TE_LENGTH 9
#define ZMI_TE_SPARSE 10     /* status 0 */
#define ZMI_TIFF_ASSEMBLE 1u /* flags: the page as one image */
#define ZMI_TIFF_PAGES_MAX 65535u
typedef struct zmi_tiff_page {      /* 72 bytes */
    uint64_t offsets_pos, counts_pos; /* file positions of the values of StripOffsets / TileOffsets and of the byte counts */
    uint32_t width, height;
    uint32_t seg_w, seg_h;            /* tile size; strips: seg_w = width, seg_h = min(RowsPerStrip, height) */
    uint32_t segs_across, segs_down, n_segs;
    uint32_t seg_bytes;               /* decoded bytes of a full segment: seg_w * seg_h * samples * sample_bytes */
    uint16_t bits, samples, sample_format, predictor, compression, photometric, extra_samples;
    uint8_t  sample_bytes;            /* bits / 8; 0 where the depth is not 8 / 16 / 32 / 64 */
    uint8_t  big_endian, bigtiff, tiled;
    uint8_t  offsets_type, counts_type;   /* 3 SHORT, 4 LONG, 16 LONG8 */
    int32_t  status;                  /* 0: readable by zmi_tiff_read_dev; otherwise the ZMI_TP_* reason */
} zmi_tiff_page;
typedef struct zmi_tiff_info {      /* 40 bytes */
    uint64_t n_pages, n_listed, first_ifd;
    uint32_t big_endian, bigtiff;
    int32_t status, detail;
} zmi_tiff_info;
uint32_t zmi_tiff_row_tile(void);   /* bytes of a row one trip of the unpredict kernel covers per wave (for tests that place row lengths
                                       around it): pixel sizes that do not divide 16 make the trip a little shorter, see tiff_kernels.h */
int zmi_tiff_directory_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, zmi_tiff_page* d_pages, uint32_t cap, zmi_tiff_info* d_info,
                           void* stream);
int zmi_tiff_read_dev(zmi_ctx* ctx, const void* d_in, uint64_t in_len, const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page,
                      const uint32_t* d_sel, uint32_t n_sel, uint64_t decoded_bytes, uint32_t flags, uint32_t out_align, void* d_out,
                      uint64_t out_cap, uint64_t* d_out_off /* n_sel + 1 */, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail,
                      void* stream);

/* ---- writing TIFF files with Deflate compression: the forward predictor, deflate in pieces, the IFD -------------------------------------
 * The inverse of the two calls above: one page in device memory becomes one complete little-endian (II) TIFF file in device memory,
 * one asynchronous call on `stream` that never synchronises with the host.  The geometry is the caller's (*w is host memory, read during
 * the call), so n_segs, the decoded size of every segment and the length of the metadata follow on the host and every table is sized
 * exactly; the geometry words are the reader's: seg_w, seg_h, segs_across, segs_down, n_segs, seg_bytes.  Not written: big-endian files,
 * several pages, compression 1 and LZW, PlanarConfiguration 2, depths below 8, sparse segments, ancillary tags, SubIFDs.
 *
 *   Arguments   ZMI_E_ARG as the return value, with a zmi_last_error text and nothing launched: a dimension of 0; bits not 8 / 16 / 32 / 64;
 *               samples 0 or above 8; extra_samples >= samples; predictor outside 1 .. 3; sample_format outside 1 .. 3; predictor 3
 *               without sample_format 3 or with bits < 16; exactly one of tile_w / tile_h being 0; a tile size that is not a multiple
 *               of 16 (TIFF 6.0 section 15); a segment whose decoded size passes ZMI_PNG_SCAN_MAX; piece_bytes outside 1 .. 2^30; level
 *               outside -1 .. 9; strategy outside 0 .. 4; out_align not a power of two in 1 .. 4096; an unknown flag; more than
 *               2^31 - 1 pieces (n_segs + the page's decoded bytes / piece_bytes).
 *   Input       default (dense): segment k is the bytes d_in[d_in_off[k] ..) -- exactly the region zmi_tiff_read_dev writes in dense
 *               mode: [rows, seg_w, C] little-endian samples, the last strip only the rows left, edge tiles with their padding as
 *               given.  flags & ZMI_TIFF_ASSEMBLE: d_in is the [height, width, C] image, d_in_off is not read; the predict kernel cuts
 *               the segments itself and the padding samples of edge tiles are 0.  d_in may stand at any alignment.
 *   File        every byte is fixed:
 *                 classic   49 49 2A 00 08 00 00 00 | the IFD at 8: u16 count, entries of 12 bytes, u32 0
 *                 BigTIFF   49 49 2B 00 08 00 00 00 | u64 16 | the IFD at 16: u64 count, entries of 20 bytes, u64 0
 *               The entries stand ascending by tag ("seg" = LONG, in BigTIFF LONG8): 256 LONG width; 257 LONG height; 258 SHORT x
 *               samples; 259 SHORT 8; 262 SHORT photometric; strips: 273 seg x n_segs; 277 SHORT samples; strips: 278 LONG seg_h,
 *               279 seg x n_segs; 284 SHORT 1; 317 SHORT predictor (always); tiles: 322 LONG seg_w, 323 LONG seg_h, 324 and 325 seg x
 *               n_segs; 338 SHORT x extra_samples, each extra_kind, only where extra_samples > 0; 339 SHORT x samples.  Values that fit
 *               the 4-byte value field (BigTIFF: 8) stand in it, left-justified and zero-filled -- the two arrays of a one-segment
 *               page too --, the others follow the IFD in tag order, each at the next even position.  Segment 0 starts at the next
 *               multiple of out_align, every further segment at the next multiple behind its predecessor; every gap byte is 0; the
 *               file ends with the last byte of the last segment.
 *   Segment     one zlib stream: the two header bytes zmi_deflate_stream_dev writes for ZMI_WRAP_ZLIB at that level and strategy; the
 *               predicted bytes cut into pieces of piece_bytes, each compressed exactly as zmi_deflate_pieces_dev(
 *               ZMI_STREAM_INDEPENDENT) does with max_len = piece_bytes -- every piece but the last ends with the flush marker, the
 *               last ends the stream --; the big-endian Adler-32 of the predicted bytes: the IDAT payload of zmi_png_encode_dev.
 *               Level 0 is stored blocks through the same path.  A file's bytes are a function of the pixels and *w alone -- not of
 *               the alignment of d_in, the scratch limit, the launch grouping or the wave schedule.
 *   Predictor   the inverse of what the reader undoes.  1 copies; 2: d[i] = x[i] - x[i - samples] mod 2^bits along a row, the first
 *               pixel as it is, integer arithmetic on the bits whatever sample_format says; 3 (Technical Note 3): byte b of sample k,
 *               b = 0 the most significant, goes to p[b * N + k] with N = seg_w * samples, then q[j] = p[j] - p[j - samples] mod 256 over
 *               the row's bytes.
 *   Words       *d_file_len = the length the file needs, whether or not it fitted; d_seg_len[k] (the table may be NULL) = the byte count
 *               of segment k; d_status[k] = the first encoder status of its pieces, or 0; *d_file_status = the first of these that holds:
 *               ZMI_E_ARG where a classic file would pass 2^32 - 1 bytes, Z_BUF_ERROR where the file does not fit out_cap, the first
 *               segment status that is not 0, 0.  Nothing at or behind d_out + out_cap is written; with Z_BUF_ERROR nothing is promised
 *               about the bytes in front of it.  d_written (NULL or one record) = what zmi_tiff_directory_dev would list for page 0 of
 *               the written file, every field; all zeros with the file status where that is not 0.
 *   zmi_tiff_bound   room that always suffices (not tight); 0 where *w is not valid.
 *   Plan        zmi_png_encode_dev's with segments in place of images: one piece table of exactly the page's pieces (at most n_segs +
 *               decoded bytes / piece_bytes), launch groups within the scratch limit, the running offset kept in a device word; the hole
 *               in front of a segment's first piece is the 2 header bytes (and the pad in front of them), the one behind its last the
 *               4 of the Adler-32, the metadata is the hole in front of segment 0.  A piece's slot and match scratch are sized for
 *               min(seg_bytes, piece_bytes), the longest piece the page has; the bytes are those of pieces of piece_bytes all the same.
 *   Scratch of the context: the predicted segments, every one at a multiple of 16, NOT capped by the scratch limit (the whole page is
 *   predicted before the first group is encoded); 8 bytes per segment, 40 bytes and 1 bit per piece, 12 bytes per slot of a group; one
 *   group's slots as in zmi_zip_write_dev.  Scratch that cannot be reserved is ZMI_E_NOMEM.
 *   Event timing, as zmi_png_encode_dev: 3 = the predict kernel (the decoder's slot is idle on every write path), 0 = Adler-32 of the
 *   pieces and the fold per segment, 1 / 5 / 2 = match search, parse, encode, 7 = the piece table, places and pack, 4 = the file's fixed
 *   bytes, the segments' frames and array entries, the words. */
#define ZMI_TIFF_BIGTIFF 2u          /* flags; ZMI_TIFF_ASSEMBLE (1u) keeps its meaning: the input is the page as one image */
typedef struct zmi_tiff_write {     /* host memory, read during the call */
    uint32_t width, height;
    uint32_t tile_w, tile_h;          /* both 0: strips */
    uint32_t rows_per_strip;          /* strips only; 0 or >= height: one strip */
    uint16_t bits, samples, sample_format, predictor, photometric, extra_samples, extra_kind;
    uint32_t flags, piece_bytes, out_align;
    int32_t  level, strategy;
} zmi_tiff_write;
uint32_t zmi_tiff_predict_tile(void);   /* bytes of a row one trip of the predict kernel covers per wave (for tests that place row lengths around it) */
uint64_t zmi_tiff_bound(const zmi_tiff_write* w);      /* room that always suffices; 0 where w is not valid */
int zmi_tiff_write_dev(zmi_ctx* ctx, const zmi_tiff_write* w, const void* d_in, const uint64_t* d_in_off /* n_segs, NULL with ASSEMBLE */,
                       void* d_out, uint64_t out_cap, uint64_t* d_file_len, uint32_t* d_seg_len /* NULL or n_segs */,
                       int32_t* d_status /* n_segs */, int32_t* d_file_status, zmi_tiff_page* d_written /* NULL or 1 */, void* stream);

/* ---- reading OpenEXR images (ZIP / ZIPS / PXR24 / NONE): the attribute list, a batch inflate of the chunks, the unzip ------------------
 * Two calls, both asynchronous on `stream`, neither synchronises with the host, every per-file failure is a device word.  File i is
 * d_in[d_in_off[i] .. + d_in_len[i]), at any alignment.  OpenEXR is not part of the reference project: the contract is the format, as
 * stated here.  Not built, each a change of its own: RLE, PIZ, B44, DWA; subsampled channels, mip / rip levels,
 * multi-part and deep files; a selection of rows or tiles inside a file; conversion of HALF to float.
 *
 * The format.  All integers and floats are little-endian.
 *   File        the magic 76 2f 31 01; a version word u32 -- the low byte is the version number (2), the upper bits are flags: 0x200
 *               single-part tiled, 0x400 long names (up to 255 bytes instead of 31), 0x800 deep data, 0x1000 multi-part --; the header:
 *               a list of attributes ended by one 00 byte (an empty name); directly behind it the offset table, one u64 file position
 *               per chunk; the chunks.  An attribute is name\0 | type\0 | i32 size | size bytes of value.
 *   Attributes  the reader uses these and skips all others by their size, whatever their type:
 *               channels (chlist)         entries ended by a 00 byte, each name\0 | i32 pixelType (0 UINT 4 bytes, 1 HALF 2 bytes, 2 FLOAT
 *                                         4 bytes) | u8 pLinear | 3 reserved bytes | i32 xSampling | i32 ySampling.  The order of the
 *                                         list is the storage order; writers keep it sorted by name, the reader takes it as it stands.
 *               compression (1 byte)      0 NONE, 1 RLE, 2 ZIPS: 1 scanline per chunk; 3 ZIP: 16; 4 PIZ: 32; 5 PXR24: 16; 6 B44, 7 B44A,
 *                                         8 DWAA: 32; 9 DWAB: 256
 *               dataWindow (box2i)        i32 xMin, yMin, xMax, yMax, inclusive, may be negative; W = xMax - xMin + 1, H = yMax - yMin + 1
 *               displayWindow (box2i)     recorded, not used
 *               lineOrder (1 byte)        0 increasing y, 1 decreasing y, 2 random y (tiled files only): the PHYSICAL order of the chunks;
 *                                         the offset table is always in increasing y, or in tile order
 *               tiles (tiledesc, 9 bytes; required with flag 0x200)   u32 xSize, u32 ySize, u8 mode: level mode = mode & 15 (0 one level,
 *                                         1 mipmap, 2 ripmap), rounding = mode >> 4
 *   Chunks      scanline files: ceil(H / lines per chunk) chunks, chunk k = i32 y | i32 dataSize | data with y = yMin + k * lines
 *               (absolute); the last chunk holds the scanlines that remain.  Tiled files with one level: ceil(W / xSize) x ceil(H / ySize)
 *               chunks, table index = tileY * tilesX + tileX, each i32 tileX | i32 tileY | i32 levelX | i32 levelY | i32 dataSize | data;
 *               edge tiles hold only the pixels inside the data window (cropped, not padded).  The UNCOMPRESSED bytes of a chunk
 *               ("raw"): for every scanline of the chunk (of the tile) in increasing y, for every channel in list order, that
 *               scanline's pixels of that channel, left to right -- a row is C planar runs of width * size bytes, and the expected raw
 *               size is n = rows * sum_c width * size_c.  dataSize == n: the raw bytes as they stand (writers store a chunk raw when
 *               compression does not shrink it, compression NONE always does); dataSize < n: a compressed chunk; dataSize > n: an error.
 *   ZIP / ZIPS  the data is one zlib stream (RFC 1950) that inflates to exactly n bytes d[0 .. n).  Predictor undo: t[0] = d[0], t[i] =
 *               (t[i - 1] + d[i] - 128) mod 256 -- equivalently t[i] = (sum_{k <= i} d[k] - 128 i) mod 256: an inclusive byte sum with 128
 *               subtracted at odd i.  Interleave: with h = (n + 1) / 2, raw[2 i] = t[i] and raw[2 i + 1] = t[h + i].
 *               Example: d = 00 80 80 80 e6 19 bd 84 82 82 6a gives raw = 00 3c 00 40 00 42 00 44 66 2e ff.
 *   PXR24       compression 5: 16 scanlines per chunk, or one tile; chunk headers, the table, the line orders and the raw rule
 *               (dataSize == n: the n raw bytes, floats at their full 32 bits) exactly as for ZIP.  dataSize < n: one zlib stream that
 *               inflates to exactly m = rows * sum_c width * p_c bytes with p = 4 / 2 / 3 for UINT / HALF / FLOAT (m <= n, and m < n as
 *               soon as there is a FLOAT channel).  The inflated bytes: for every scanline of the chunk in increasing y, for every
 *               channel in list order, a run of p * w bytes (w = the pixels of that row in the chunk): p planes of w bytes, most
 *               significant byte first, that hold diff[x] = v[x] - v[x - 1] mod 2^(8p) with v[-1] = 0 at the start of every run -- byte
 *               k of plane j is (diff[k] >> 8 (p - 1 - j)) & 255.  v is the UINT value, the HALF's 16 bits, and f24(bits) of a FLOAT.
 *               Reading accumulates v[x] = (v[x - 1] + diff[x]) mod 2^(8p) and writes v, for FLOAT v << 8: the low byte of every float
 *               read from a compressed chunk is 0.  f24 of the 32 float bits u, with s = u & 0x80000000, e = u & 0x7f800000, m = u &
 *               0x007fffff: if e == 0x7f800000 and m != 0, m >>= 8 and i = (e >> 8) | m | (m == 0 ? 1 : 0) -- a NaN stays a NaN --; if
 *               e == 0x7f800000 and m == 0, i = e >> 8; otherwise i = ((e | m) + (m & 0x80)) >> 8, and if i >= 0x7f8000 then i = (e |
 *               m) >> 8 -- rounding never produces an infinity.  f24 = (s >> 8) | i.  Pinned: 3f000000 -> 3f0000, 3f8000ff -> 3f8001,
 *               3f80007f -> 3f8000, 3f800080 -> 3f8001, 7f7fffff -> 7f7fff, 7f800000 -> 7f8000, 7f800001 -> 7f8001, ffc12345 ->
 *               ffc123, 80000000 -> 800000, 000000ff -> 000001, bfc00000 -> bfc000.
 *               Example: one row of width 3, channels G HALF = 1, 2, 3; Z FLOAT = 0.5, -1.5, 2.5; id UINT = 7, 5, 0x01020304.  Raw, 30
 *               bytes: 003c 0040 0042 0000003f 0000c0bf 00002040 07000000 05000000 04030201.  Inflated, 27 bytes: 3c 04 02 00 00 00 |
 *               3f 80 80 00 c0 60 00 00 00 | 00 ff 01 00 ff 02 00 ff 02 07 fe ff.  (zlib level 6 makes 33 bytes of them, so a writer
 *               stores this chunk raw; a crafted file may still carry the stream.)
 *
 * zmi_exr_headers_dev   one lane per file walks the attributes (the chain is serial; the batch is the parallelism) and writes one
 *               zmi_exr_image per file and the first chan_cap channels of file i to d_channels[i * chan_cap ..) (the records behind the
 *               file's last channel are zeros).  The first rule that holds, in this order, is the record's status:
 *   ZMI_XE_MAGIC        the four magic bytes are wrong, or the file is shorter than 8 bytes
 *   ZMI_XE_HEADER       a version number other than 2; an attribute or a name that leaves the file; a name (of an attribute, a type or a
 *                       channel) that is too long, a type name that is empty; a negative size; a missing channels, compression,
 *                       dataWindow or lineOrder; missing tiles in a tiled file; a wrong value size for a used attribute (a channel list
 *                       that does not end with its attribute); an inverted window; a pixel type above 2; zero channels; a sampling below
 *                       1; a compression above 9; a line order above 2; a tile size of 0, a level mode above 2 or a rounding above 1; an
 *                       offset table that leaves the file; more than ZMI_EXR_ATTRS_MAX attributes (the walk is one lane's: it ends
 *                       there, as the TIFF chain ends at 65 535 IFDs).  Only version, the tiled flag and the status are set.
 *   ZMI_XE_KIND         deep or multi-part flags
 *   ZMI_XE_COMPRESSION  anything but 0, 2, 3, 5: the file is listed with its dimensions and channels, and flagged
 *   ZMI_XE_SAMPLING     a sampling other than 1
 *   ZMI_XE_LEVELS       mipmap or ripmap (n_chunks: those of level 0)
 *   ZMI_XE_CHANNELS     more than chan_cap channels; n_channels still holds the true count, row_bytes and region_bytes are 0
 *   ZMI_XE_BIG          W, H, W * H, a chunk's raw size or the region's size does not fit 32 bits
 *   An attribute that stands twice: the first counts.
 *
 * zmi_exr_read_dev      slot j reads file d_sel[j] of the table (d_sel NULL: slot j = file j); duplicates are allowed; an index >= n_files,
 *               and a record no headers call would write for that file (every size and position is derived again from the windows, the
 *               compression, the tile description and the channel types and compared; the offset table must stand inside the file),
 *               get ZMI_E_ARG in the slot's status and nothing of them is read.  chunk_cap and decoded_bytes are the host's bounds on
 *               the chunks and on the raw bytes (height * row_bytes) of the readable files of the selection, summed in slot order; they
 *               size the tables and the scratch, and every slot from the first whose running sum passes either bound on gets ZMI_E_ARG.
 *   Region      the channels' planes in list order; plane c is [H, W] of its type, little-endian, at zmi_exr_channel.plane_off, the
 *               next multiple of 4 bytes (the at most 2 bytes of padding in front of a plane are not written).  With one pixel type
 *               throughout the region is a [C, H, W] tensor with a plane stride of W * H * size rounded up to 4 bytes: dense, except
 *               for several HALF channels of an odd W * H, where one unwritten pixel lies between two planes.
 *   Plan        d_out_off, out_align, out_cap exactly as zmi_png_decode_dev: d_out_off[j] = the region sizes of the readable slots in
 *               front, each rounded up to out_align; d_out_off[n_sel] = the room the selection needs; a flagged or failed slot has
 *               length 0; nothing at or behind d_out + out_cap and nothing in the gaps is written.
 *   Reading     one kernel reads every chunk's table entry and header; compressed chunks go through the batch decoder with
 *               ZMI_WRAP_ZLIB and capacity n (PXR24: m, in a place of n bytes) into scratch, every chunk at a multiple of 16, and
 *               the decoder checks the Adler-32; raw chunks go through the range copy into the same scratch; the unzip kernel
 *               (exr_kernels.h) undoes the predictor and the interleave and writes every run at its place in its plane -- the streams
 *               of PXR24 files go through zmi_exr_pxr24_undo_kernel instead: one wave per (chunk, row, channel) run, a prefix sum of
 *               16-, 24- or 32-bit words --; one kernel writes the slot's words.  One call may mix NONE, ZIPS, ZIP and PXR24 files in
 *               any slot order.  flags must be 0.
 *   d_status / d_detail   after the record's own flag (Z_DATA_ERROR for MAGIC and HEADER, Z_BUF_ERROR for CHANNELS, else
 *               Z_VERSION_ERROR; detail = the ZMI_XE_* code) the first of these that holds for any chunk of the file; d_detail = the
 *               code, with the index of the first chunk that has it above the low 8 bits:
 *               Z_BUF_ERROR / ZMI_XE_OUT        the region does not fit out_cap (no chunk index)
 *               Z_MEM_ERROR / ZMI_XE_SCRATCH    the decoder could not reserve what the chunk needs
 *               Z_DATA_ERROR / ZMI_XE_CHUNK     a table entry that leaves the file; a chunk header whose y or tile coordinates are not
 *                                               the expected ones; a nonzero level; a dataSize that is negative, above n, or leaves the
 *                                               file; compression NONE with dataSize != n
 *               Z_DATA_ERROR / ZMI_XE_MISSING   a table entry of 0, the mark of an unfinished file
 *               Z_DATA_ERROR / ZMI_XE_DATA      a corrupt stream, a wrong Adler-32, FDICT
 *               Z_DATA_ERROR / ZMI_XE_LENGTH    the stream does not end at exactly n bytes (PXR24: m bytes)
 *   d_out_len[j] = the region's size with status 0, otherwise 0.  Never status 0 with wrong bytes; one bad file does not touch its
 *   neighbours.  n_sel 0 writes d_out_off[0] = 0 and nothing else.  Bytes and words do not depend on the alignment of d_in, on the
 *   slot index, on n_files or on the decode-kernel selection.
 *   Scratch of the context: 40 bytes per slot, 100 per chunk of chunk_cap, 8 per 1024 bytes of decoded_bytes; the inflated chunks,
 *   decoded_bytes + 16 bytes per chunk + 96; and the decoder's, sized by this call.  Scratch that cannot be reserved is ZMI_E_NOMEM.
 *   Event timing: 5 = headers; slot and chunk tables, plans, 3 / 6 = decode, resolve, 7 = the copies of raw chunks, 2 = block sums, their
 *   scans, the unzip and the PXR24 undo, 4 = the slot words. */
#define ZMI_XE_MAGIC 1        /* zmi_exr_image.status and the slot's detail: Z_DATA_ERROR */
#define ZMI_XE_HEADER 2       /* Z_DATA_ERROR */
#define ZMI_XE_KIND 3         /* Z_VERSION_ERROR */
#define ZMI_XE_COMPRESSION 4  /* Z_VERSION_ERROR */
#define ZMI_XE_SAMPLING 5     /* Z_VERSION_ERROR */
#define ZMI_XE_LEVELS 6       /* Z_VERSION_ERROR */
#define ZMI_XE_CHANNELS 7     /* Z_BUF_ERROR */
#define ZMI_XE_BIG 8          /* Z_VERSION_ERROR */
#define ZMI_XE_OUT 9          /* slots only, from here on: Z_BUF_ERROR */
#define ZMI_XE_SCRATCH 10     /* Z_MEM_ERROR */
#define ZMI_XE_CHUNK 11       /* Z_DATA_ERROR */
#define ZMI_XE_MISSING 12
#define ZMI_XE_DATA 13
#define ZMI_XE_LENGTH 14
#define ZMI_EXR_ATTRS_MAX 65535u
typedef struct zmi_exr_channel {    /* 24 bytes */
    uint32_t name_pos, name_len;      /* the name's position in the file and its bytes (no 0) */
    int32_t  pixel_type;              /* 0 UINT, 1 HALF, 2 FLOAT */
    int32_t  x_sampling, y_sampling;
    uint32_t plane_off;               /* byte offset of the channel's [H, W] plane inside the file's region */
} zmi_exr_channel;
typedef struct zmi_exr_image {      /* 88 bytes */
    uint32_t version;                 /* the version word: number and flags */
    uint8_t  compression, line_order, tile_mode, tiled;
    int32_t  data_window[4], display_window[4];   /* xMin, yMin, xMax, yMax */
    uint32_t width, height, lines_per_chunk;
    uint32_t tile_w, tile_h;          /* 0 in scanline files */
    uint32_t n_channels, n_chunks;
    uint32_t row_bytes;               /* sum over the channels of width * size */
    uint32_t region_bytes;            /* the file's region: the planes, each at the next multiple of 4 */
    int32_t  status;                  /* 0: readable by zmi_exr_read_dev; otherwise the ZMI_XE_* reason */
    uint64_t table_pos;               /* file position of the offset table */
} zmi_exr_image;
uint32_t zmi_exr_trip(void);    /* output bytes one trip of the unzip kernel covers per wave (for tests that place run lengths around it) */
uint32_t zmi_exr_piece(void);   /* the longest piece of a run one work item of the unzip kernel writes: a whole number of trips */
uint32_t zmi_exr_pxr24_trip(void);   /* pixels one trip of the PXR24 undo kernel (and of the forward kernel) covers per wave */
int zmi_exr_headers_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_files,
                        zmi_exr_image* d_images, zmi_exr_channel* d_channels /* n_files * chan_cap */, uint32_t chan_cap, void* stream);
int zmi_exr_read_dev(zmi_ctx* ctx, const void* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_exr_image* d_images,
                     const zmi_exr_channel* d_channels, uint32_t chan_cap, uint32_t n_files, const uint32_t* d_sel, uint32_t n_sel,
                     uint32_t chunk_cap, uint64_t decoded_bytes, uint32_t flags, uint32_t out_align, void* d_out, uint64_t out_cap,
                     uint64_t* d_out_off /* n_sel + 1 */, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, void* stream);

/* ---- writing OpenEXR images (ZIP / ZIPS / PXR24 / NONE): the forward transform, deflate in pieces, chunks and offset table -----------------
 * The inverse of the two calls above: a batch of images of ONE layout (a frame sequence) in device memory becomes a batch of complete
 * single-part .exr files in one device buffer, one asynchronous call on `stream` that never synchronises with the host; every per-image
 * failure is a device word.  The layout is the caller's (*w and the channel list are host memory, read during the call), so the chunk
 * count, every chunk's raw size n and the header's bytes follow on the host and every table is sized exactly.  Not written: the other
 * compressions, subsampled channels, mip / rip levels, multi-part and deep files, line orders other than increasing y, further attributes.
 *
 *   Arguments   ZMI_E_ARG as the return value, with a zmi_last_error text and nothing launched: an inverted window; a width, height,
 *               pixel count, row, region or chunk that does not fit 32 bits (what the reader flags ZMI_XE_BIG); zero channels; a pixel
 *               type above 2; a name that is NULL, empty or longer than 255 bytes; names that are not strictly ascending bytewise (the
 *               order every other writer keeps, so the file reads elsewhere); a compression other than 0, 2, 3, 5; exactly one of tile_w /
 *               tile_h being 0; piece_bytes outside 1 .. 2^30; level outside -1 .. 9; strategy outside 0 .. 4; out_align not a power of
 *               two in 1 .. 4096; flags other than 0; a file bound above 2^32 - 1; more than 2^31 - 1 pieces or chunks in the call;
 *               a NULL table that is not optional.
 *   Input       image i is exactly the region zmi_exr_read_dev writes, at d_in + d_in_off[i], at any alignment: the channels' [H, W]
 *               planes in list order, little-endian, each at the next multiple of 4 bytes; the pad bytes are not read.
 *   File        every byte is fixed:
 *                 76 2f 31 01 | u32 version = 2, | 0x200 where tiled, | 0x400 where a channel name is longer than 31 bytes
 *                 the attributes, each name\0 type\0 i32 size value, in this order:
 *                   channels chlist            per channel name\0 | i32 pixelType | u8 pLinear 0 | 00 00 00 | i32 1 | i32 1; then 00
 *                   compression compression    1 byte
 *                   dataWindow box2i           4 x i32
 *                   displayWindow box2i        4 x i32
 *                   lineOrder lineOrder        1 byte, 0
 *                   pixelAspectRatio float     1.0
 *                   screenWindowCenter v2f     0.0, 0.0
 *                   screenWindowWidth float    1.0
 *                   tiles tiledesc             tiled files only: u32 tile_w | u32 tile_h | u8 mode 0
 *                 00 | the offset table, one u64 per chunk | the chunks in table order, dense: no gap and no padding inside a file,
 *                 which ends with its last chunk.
 *               Chunk k of a scanline file is i32 y = yMin + k * lines | i32 dataSize | data, of a tiled file i32 tileX | i32 tileY |
 *               i32 0 | i32 0 | i32 dataSize | data with k = tileY * tilesX + tileX; edge tiles are cropped.  With compression NONE,
 *               windows (-1, 5, 1, 6) / (0, 0, 2, 1), channels G HALF = 1 .. 6 and Z FLOAT = 0.5 .. 5.5 the file is these 363 bytes:
 *                 762f3101 02000000 "channels\0chlist\0" 25000000 "G\0" 01000000 00000000 01000000 01000000 "Z\0" 02000000 00000000
 *                 01000000 01000000 00 "compression\0compression\0" 01000000 00 "dataWindow\0box2i\0" 10000000 ffffffff 05000000
 *                 01000000 06000000 "displayWindow\0box2i\0" 10000000 00000000 00000000 02000000 01000000 "lineOrder\0lineOrder\0"
 *                 01000000 00 "pixelAspectRatio\0float\0" 04000000 0000803f "screenWindowCenter\0v2f\0" 08000000 00000000 00000000
 *                 "screenWindowWidth\0float\0" 04000000 0000803f 00 | 3701000000000000 5101000000000000 | 05000000 12000000
 *                 003c 0040 0042 0000003f 0000c03f 00002040 | 06000000 12000000 0044 0045 0046 00006040 00009040 0000b040
 *   Chunk data  the raw bytes are the chunk's rows, every row the planar runs of its channels (the reader's comment above).  The zip
 *               forward transform with h = (n + 1) / 2: t[i] = raw[2 i], t[h + i] = raw[2 i + 1]; d[0] = t[0], d[i] = (t[i] - t[i - 1]
 *               + 128) mod 256.  The candidate stream is the IDAT payload zmi_png_encode_dev would write for d: the two zlib header bytes
 *               zmi_deflate_stream_dev writes for that level and strategy; d in pieces of piece_bytes, each compressed exactly as
 *               zmi_deflate_pieces_dev(ZMI_STREAM_INDEPENDENT) does with max_len = piece_bytes; the big-endian Adler-32 of d.
 *   PXR24       compression 5 (16 scanlines a chunk, or one tile): d is the chunk's m bytes of byte planes stated with the reader --
 *               zmi_exr_pxr24_forward_kernel: a work item is one trip of a run, f24 on FLOAT, the predecessor from the lane below,
 *               no scan -- and everything behind it is the ZIP path with length m: pieces, Adler-32, candidate.  The raw rule compares
 *               the candidate with n, and a chunk stored raw holds the n raw bytes with full 32-bit floats.  Writing is therefore
 *               lossy for FLOAT channels only, and only in the chunks that are stored compressed: such a float reads back as
 *               f24(bits) << 8.  UINT and HALF are exact.  zmi_exr_bound is unchanged.
 *   Raw rule    the reader takes dataSize == n to mean raw bytes, so: where the candidate's length is >= n the chunk's data is the n
 *               RAW bytes (not d) and dataSize = n; otherwise the data is the candidate and dataSize < n.  Level 0 therefore stores
 *               every chunk raw (under PXR24: every chunk without a FLOAT channel; m + the stored blocks' bytes may stay below n), and
 *               so does a chunk of 2 bytes; compression NONE skips the encoder altogether.  A file's bytes are a
 *               function of its pixels and *w alone -- not of n_images, the image's index, the alignment of d_in, the scratch limit,
 *               the launch grouping or the wave schedule.
 *   Words       as zmi_png_encode_dev: d_out_off[i] = the lengths in front, each rounded up to out_align; d_out_off[n_images] = the room
 *               the batch needs, whether or not it fitted; a file that crosses out_cap has Z_BUF_ERROR and length 0 (nothing is promised
 *               about its bytes in front of out_cap); nothing at or behind d_out + out_cap and nothing in the alignment gaps is written.
 *               d_status[i] = 0, Z_BUF_ERROR, or the first encoder status among the image's pieces (such a chunk is stored raw, the
 *               length is 0).  d_chunk_len (NULL or n_images * n_chunks) = every chunk's dataSize.  d_written / d_written_channels
 *               (NULL or n_images / n_images * n_channels records) = exactly what zmi_exr_headers_dev lists for the written file with
 *               chan_cap = n_channels, name_pos included; zeros and the status for an image whose status is not 0.  n_images 0 writes
 *               d_out_off[0] = 0 and nothing else.
 *   zmi_exr_bound   header + table + every chunk's header + n, rounded up to out_align, times n_images: with the raw rule no file is
 *               longer.  0 where *w is not valid.
 *   Plan        one piece table of exactly the call's pieces; launch groups of whole chunks -- the raw decision needs a chunk's whole
 *               candidate length before its first byte is placed -- of floor(pieces the scratch limit allows / pieces of the largest
 *               chunk) chunks (ZMI_STREAM_GROUP is rounded down the same way, to at least one chunk; a limit too small for one chunk is
 *               ZMI_E_NOMEM); the place kernel decides per chunk, the running offset stays in a device word.  Chunk sizes, piece counts
 *               and item counts are device scans over the chunks of the call.  Raw chunks are gathered from the planes straight into
 *               the file; no copy of the image stands in scratch.
 *   Scratch of the context: d of every chunk of the call, each at a multiple of 16, NOT capped by the scratch limit (nothing under
 *   NONE; m of them under PXR24); 72 bytes per chunk, 36 bytes and 1 bit per piece, 4 per image, 8 per launch group, 24 per channel and the header's bytes; one
 *   group's slots as in zmi_zip_write_dev.  Scratch that cannot be reserved is ZMI_E_NOMEM.
 *   Event timing, as zmi_tiff_write_dev: 3 = the forward zip kernel (PXR24: the forward kernel), 0 = Adler-32 of the pieces and the fold per chunk, 1 / 5 / 2 =
 *   match search, parse, encode, 7 = the chunk and piece tables, places, pack and the raw gather, 4 = the fixed bytes and the words. */
typedef struct zmi_exr_write_channel { const char* name; int32_t pixel_type; } zmi_exr_write_channel;   /* 0 UINT, 1 HALF, 2 FLOAT */
typedef struct zmi_exr_write {      /* host memory, read during the call */
    int32_t  data_window[4], display_window[4];   /* xMin, yMin, xMax, yMax */
    uint32_t n_channels;
    const zmi_exr_write_channel* channels;        /* sorted by name */
    uint32_t compression;             /* 0 NONE, 2 ZIPS, 3 ZIP, 5 PXR24 */
    uint32_t tile_w, tile_h;          /* both 0: scanlines */
    uint32_t flags, piece_bytes, out_align;
    int32_t  level, strategy;
} zmi_exr_write;
uint32_t zmi_exr_zip_trip(void);    /* raw bytes one trip of the forward zip kernel covers per wave (for tests that place run lengths around it) */
uint64_t zmi_exr_bound(const zmi_exr_write* w, uint32_t n_images);   /* the room the batch needs at most; 0 where w is not valid */
int zmi_exr_write_dev(zmi_ctx* ctx, const zmi_exr_write* w, const void* d_in, const uint64_t* d_in_off, uint32_t n_images, void* d_out,
                      uint64_t out_cap, uint64_t* d_out_off /* n_images + 1 */, uint32_t* d_out_len, uint32_t* d_chunk_len /* NULL or n_images * n_chunks */,
                      zmi_exr_image* d_written /* NULL or n_images */, zmi_exr_channel* d_written_channels /* NULL or n_images * n_channels */,
                      int32_t* d_status, void* stream);

/* ---- host-buffer convenience wrappers: copy in, run the batch on the GPU, copy back ---- */
int zmi_deflate_batch(zmi_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n_shards,
                      int level, int strategy, int wrap, uint8_t* out, uint64_t out_stride, uint32_t* out_len,
                      int32_t* status);
int zmi_inflate_batch(zmi_ctx* ctx, const uint8_t* in, const uint64_t* in_off, const uint32_t* in_len, uint32_t n_streams,
                      int wrap, uint8_t* out, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len,
                      int32_t* status);
/* One host stream through zmi_inflate_resume_dev (staging buffers are kept in the context): `in` starts at bit in_bit of
 * its first byte, `hist` is the up to 32 KiB of output in front of it, resume[4] as above; out receives
 * min(*out_len, out_cap) bytes.  This is what the stream ABI's inflate() / inflateBack() run on. */
int zmi_inflate_resume(zmi_ctx* ctx, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist,
                       uint32_t hist_len, uint8_t* out, uint32_t out_cap, uint32_t* out_len, int32_t* status,
                       int32_t* detail, uint32_t* in_used, uint32_t* resume);
/* The same call for a stream with flush points (Z_SYNC_FLUSH / Z_FULL_FLUSH markers 00 00 FF FF: pigz, this library's own
 * deflate()): seg_start[0..nseg) are byte offsets into `in` proposed as restart points (seg_start[0] = 0, ascending; normally
 * the byte behind every marker found).  The pieces are decoded side by side on the whole GPU and stitched; every cut is
 * verified (the decode in front of it must end exactly there, on a block boundary), anything else falls back to the
 * serial decode from that point -- results are those of zmi_inflate_resume on the same arguments, whatever seg_start
 * holds.  *segments_used (may be NULL): how many pieces were decoded in parallel (0 = the serial path ran).
 * Reference path it accelerates: zlib-rs/src/inflate.rs:1276 ff. (the Mode::Type block loop), restarted where
 * zlib-rs/src/deflate.rs:2733-2744 (the empty stored block of a flush) made the stream restartable. */
int zmi_inflate_split(zmi_ctx* ctx, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist,
                      uint32_t hist_len, uint8_t* out, uint32_t out_cap, const uint32_t* seg_start, uint32_t nseg,
                      uint32_t* out_len, int32_t* status, int32_t* detail, uint32_t* in_used, uint32_t* resume,
                      uint32_t* segments_used);

/* The same call for a stream WITHOUT flush points -- what every ordinary compressor writes: nothing in it is byte aligned, but
 * its dynamic blocks announce themselves.  The device tries every bit position of the stream for a block header (BTYPE 10, a
 * complete code-length code, code lengths that decode exactly into two complete codes: csrc/blockscan.hip), the stretches
 * between the boundaries found are decoded side by side and stitched as above; a cut counts only if the decode in front of
 * it ended exactly there, at that bit.  Results are those of zmi_inflate_resume on the same arguments; *segments_used (may be
 * NULL) = pieces decoded in parallel, 0 = the serial path ran (stream below 256 KiB, fewer than three boundaries found).
 * Reference path it accelerates: the block loop of zlib-rs/src/inflate.rs:1276 ff. over blocks of 16 383 symbols
 * (zlib-rs/src/deflate.rs:321), driven by test-libz-rs-sys/examples/blogpost-uncompress.rs:6-44. */
int zmi_inflate_blocks(zmi_ctx* ctx, const uint8_t* in, uint32_t in_len, uint32_t in_bit, const uint8_t* hist,
                       uint32_t hist_len, uint8_t* out, uint32_t out_cap, uint32_t* out_len, int32_t* status, int32_t* detail,
                       uint32_t* in_used, uint32_t* resume, uint32_t* segments_used);

#ifdef __cplusplus
}
#endif
#endif
