// zmi_kernels.h -- launch entry points and parameter blocks shared by the kernels and the host API.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifdef ZMI_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#endif

// match-finder effort (the GPU analogue of CONFIGURATION_TABLE, deflate/algorithm/mod.rs:69-82)
struct zmi_lz_params {
    uint32_t max_chain;  // hash-chain links followed per position
    uint32_t nice_len;   // stop searching once a match this long is found
    uint32_t good_len;   // halve the remaining chain budget above this length
    uint32_t max_dist;   // farthest back-reference (<= 32768 - 5*1024 - 16 = 27632, ring-buffer constraint: LZ_MAX_DIST in lz77.hip)
    uint32_t claim;      // positions a searcher wave claims at once (64, 128, 192 or 256)
    uint32_t hash6;      // 1: chain keyed by a 6-byte hash + one most-recent 4-byte probe; 0: 4-byte hash chain
    uint32_t producers;  // 1..4 hash-building waves per workgroup (tile k is built by wave k mod producers)
    uint32_t dbg;        // measurement aids, 0 in the product (1: producers' pace alone, see lz77.hip)
    uint32_t carry;      // 1: the shards are consecutive segments of one stream; a segment may match into the up to 27 KiB
                         // in front of it (window carry-over, what a preset dictionary is in deflate.rs:499-564)
    uint32_t dict_len;   // carry only: bytes in front of shard 0 that are history too (preset dictionary / earlier input)
    uint32_t barren_chain; // chain links walked in a claim whose 64 probes all missed (an incompressible stretch: whatever the 6-byte
                           // chain holds there is mostly a hash collision).  1: with 0 the benchmark mix keeps its ratio but paper-100k.pdf loses 0.2 %
                           // for 0.5 % of the kernel's time (round 4)
    uint32_t far4, far5; // a 4- (5-) byte match further back than this costs more bits than its literals: dropped
                         // (classic zlib's TOO_FAR idea; the reference itself only drops matches <= 5 under
                         // Z_FILTERED, zlib-rs/src/deflate/algorithm/slow.rs:69-74)
};

struct zmi_enc_params {
    uint32_t max_lazy;    // defer a match shorter than this if the next position has a longer one (0 = greedy)
    uint32_t lazy2, lazy3; // ... or if the position after that (the one after) has one longer by more than this (>= 258: off)
    uint32_t wrap;        // 0 raw deflate, 1 zlib (RFC 1950), 2 gzip (RFC 1952)
    uint32_t level;       // only used for the header's level hint bits
    uint32_t block_span;  // input bytes per deflate block (multiple of 64) ...
    uint32_t block_tokens; // tokens per sub-block: after each one the encoder decides whether it joins the open block or starts
                           // a new one (the reference cuts at 16383 symbols, deflate.rs:321)
    uint32_t split_hdr_bits; // what a block of its own must save: the cost of another dynamic header
    uint32_t min_sub_span;   // input bytes a sub-block covers at least (unless it holds 2 * block_tokens tokens already)
    uint32_t strategy;    // 0 default, 4 = Z_FIXED (static trees only)
    uint32_t far4, far5;  // first block of a piece: a 4- (5-) byte match further back than this is dropped; later blocks derive
                          // their limits from the codes of the block before (enc_far_limits)
    uint32_t chain_mode;  // 0: every shard is its own stream; 1: the shards of the batch are consecutive
                          // segments of ONE raw deflate stream, only shard `last_shard` ends it (BFINAL);
                          // 2: as 1 but nothing ends the stream (Z_SYNC_FLUSH / Z_FULL_FLUSH output) -- or, with `ends`,
                          // the shards named there do
    uint32_t last_shard;
    const uint32_t* ends; // chain mode 2 only, null = none: device bitmap, bit s set = shard s of the call (first_shard included)
                          // ends a stream; the next shard starts another one
    uint32_t cost_parse;  // 1: tokens are chosen by a backward cost parse over the matches (levels 3-9, csrc/parse.hip);
                          // 0: by the lazy rule (levels 1, 2 -- greedy -- and Z_HUFFMAN_ONLY / level 0, which have no matches)
    const uint32_t* dictid; // wrap 1 only, null = none: device word holding the Adler-32 of a preset dictionary; the zlib header
                          // then carries FDICT and this DICTID (zmi_deflate_batch_shared_dict_dev)
};

// per-shard result codes written by the kernels (zlib numbering, zlib-rs/src/c_api.rs:140-148)
#define ZMI_OK 0
#define ZMI_STREAM_END 1
#define ZMI_DATA_ERROR (-3)
#define ZMI_BUF_ERROR (-5)

struct zmi_zip_entry;   // include/zmi355.h
struct zmi_zip_info;
struct zmi_png_image;
struct zmi_tiff_page;
struct zmi_tiff_info;
struct zmi_exr_image;
struct zmi_exr_channel;

// zmi_tiff_write_dev: what the host works out of *w (the geometry is the caller's, so nothing of it is a device value); the kernels of
// tiff_write_kernels.h take it by value
struct zmi_tw_plan {
    uint32_t width, height, seg_w, seg_h, across, n_segs;
    uint32_t sb, spp, pb, rb;          // bytes of a sample, samples of a pixel, bytes of a pixel, bytes of a segment's row
    uint32_t pred, assemble, big;
    uint32_t seg_bytes, last_bytes;    // decoded bytes of a full segment and of the last one (the last strip holds the rows left)
    uint32_t ss;                       // the segments stand in the scratch at multiples of this: seg_bytes rounded up to 16
    uint32_t piece_bytes, ppf, ppl, np;   // pieces of a full segment, of the last one, of the page
    uint32_t band_rows, bands;         // rows of a work item of the predict kernel, items per segment
    uint64_t off_pos, cnt_pos;         // file positions of the values of the two arrays (inside the entry where n_segs is 1)
    uint64_t meta_end, seg0;           // where the metadata ends and where segment 0 starts: the next multiple of out_align
};
// ... and the file's bytes that follow from *w alone: b[0 .. a_len) stands at 0 (header, IFD, the values of tag 258), b[a_len .. a_len +
// b_len) at b_pos (the values of tags 338 and 339, behind the two arrays); rec = the zmi_tiff_page of the written file
struct zmi_tw_meta {
    uint8_t b[400];
    uint8_t rec[72];
    uint32_t a_len, b_len;
    uint64_t b_pos;
};

// zmi_exr_write_dev: what the host works out of *w; the kernels of exr_write_kernels.h take it by value.  A chunk is a box of the data
// window -- box_w = the tile's width (scanline files: the image's), box_h = the tile's height (scanline files: the lines of a chunk) --,
// chunk k of an image the box (k % across, k / across), cropped at the right and the bottom edge: up to four sizes.
struct zmi_xw_plan {
    uint32_t W, H, box_w, box_h, across, down, nc;   // nc = across * down: the chunks of one image
    uint32_t n_ch, per_px;             // channels; the bytes of a pixel over all of them
    uint32_t tiled, comp, chdr;        // chdr: the bytes of a chunk's header, 8 or 20
    int32_t ymin;
    uint32_t hdr_len;                  // magic, version word, attributes and the 00 behind them: the offset table starts here
    uint32_t n_images, ncc;            // ncc = n_images * nc: the chunks of the call
    uint32_t piece_bytes, out_align;
    uint32_t per_p;                    // the bytes of a pixel inside a PXR24 stream: a FLOAT keeps 3
    uint8_t rec[88];                   // the zmi_exr_image of a written file
};
// a slice of the host's bytes on its way into the context's scratch (kernel arguments are the one copy that needs no staging)
struct zmi_xw_slice {
    uint8_t b[2048];
    uint32_t len;
    uint64_t at;
};

extern "C" {
int zmi_launch_gen(uint8_t* d_out, uint64_t seed, uint32_t first_shard, uint32_t n_shards, uint32_t shard_bytes,
                   hipStream_t stream);
int zmi_launch_gen_strided(uint8_t* d_out, uint64_t seed, uint32_t first_shard, uint32_t shard_step, uint32_t n_shards,
                           uint32_t shard_bytes, hipStream_t stream);
int zmi_launch_scan_sizes(const uint32_t* d_len, uint32_t n, uint64_t* d_off, hipStream_t stream);
// the same scan, offsets starting at *d_base (a device word; may be d_off[0] itself)
int zmi_launch_scan_sizes_base(const uint32_t* d_len, uint32_t n, uint64_t* d_off, const uint64_t* d_base, hipStream_t stream);
// single-stream deflate (pack.hip, checksum.hip): the pieces of a buffer, the wrapper around their packed deflate bytes, and the
// check value of the concatenation from the pieces' (check, raw length) pairs
int zmi_launch_piece_layout(uint64_t n, uint32_t piece_bytes, uint32_t count, uint64_t* d_off, uint32_t* d_len, hipStream_t stream);
uint32_t zmi_stream_header_len(int wrap);
int zmi_launch_frame(uint8_t* d_out, uint64_t out_cap, uint32_t wrap, uint32_t level, uint32_t strategy, const uint64_t* d_payload,
                     const uint32_t* d_check, const uint64_t* d_raw_len, uint64_t* d_out_len, int32_t* d_status, const int32_t* d_piece_st,
                     uint32_t n_st, uint64_t* d_index, uint32_t n_index, hipStream_t stream);
uint32_t zmi_combine_partials(uint32_t n);
int zmi_launch_checksum_combine(const uint32_t* d_check, const uint32_t* d_len, uint32_t n, uint32_t world, uint32_t n_local,
                                uint32_t adler, uint32_t* d_pc, uint64_t* d_pl, uint32_t* d_out_check, uint64_t* d_out_len,
                                hipStream_t stream);
int zmi_launch_copy_ranges(const uint8_t* d_src, const uint64_t* d_src_off, uint64_t src_stride, const uint32_t* d_len,
                           uint32_t n, uint8_t* d_dst, const uint64_t* d_dst_off, uint64_t dst_cap, uint32_t max_len,
                           hipStream_t stream);
int zmi_launch_clamp_lens(const uint32_t* d_len, const uint32_t* d_cap, uint32_t n, uint32_t* d_out, hipStream_t stream);
int zmi_launch_copy_ranges_few(const uint8_t* d_src, const uint64_t* d_src_off, uint64_t src_stride, const uint32_t* d_len,
                               uint32_t n, uint8_t* d_dst, const uint64_t* d_dst_off, uint64_t dst_cap, uint32_t max_len,
                               uint32_t groups, hipStream_t stream);
int zmi_launch_checksum(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, uint32_t n_shards,
                        uint32_t kind, uint32_t* d_adler, uint32_t* d_crc, hipStream_t stream);
int zmi_launch_lz77(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, uint32_t first_shard,
                    uint32_t n_shards, uint32_t* d_match, uint64_t match_stride, zmi_lz_params prm, hipStream_t stream);
// the match search with one preset dictionary in front of every shard (lz77.hip): d_img = zmi_launch_dict_image's image of
// zmi_lz77_dict_image_len(dict_len) bytes (lead 0).  zmi_launch_dict_image: d_img[0, lead) = 0, then the last `take` bytes of the
// dictionary, then `pad` zero bytes; d_lay_off / d_lay_len (may be null) receive the one-entry layout (0, dict_len)
int zmi_launch_dict_image(const uint8_t* d_dict, uint32_t dict_len, uint8_t* d_img, uint32_t lead, uint32_t take, uint32_t pad,
                          uint64_t* d_lay_off, uint32_t* d_lay_len, hipStream_t stream);
uint32_t zmi_lz77_dict_image_len(uint32_t dict_len);
int zmi_launch_lz77_dict(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, uint32_t first_shard,
                         uint32_t n_shards, uint32_t* d_match, uint64_t match_stride, zmi_lz_params prm, const uint8_t* d_img,
                         uint32_t img_len, hipStream_t stream);
int zmi_launch_encode(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len, uint32_t first_shard,
                      uint32_t n_shards, uint32_t* d_match, uint64_t match_stride, const uint32_t* d_adler,
                      const uint32_t* d_crc, uint8_t* d_out, uint64_t out_stride, uint32_t out_cap, uint32_t* d_out_len,
                      int32_t* d_status, uint32_t pieces, uint32_t* d_piece_len, const uint32_t* d_dec, uint64_t dec_stride,
                      zmi_enc_params prm, hipStream_t stream);
// the cost parse (levels 3-9, csrc/parse.hip): d_dec receives two bits per position of every shard of the group (dec_stride
// dwords per shard, 16 bytes per segment of 64 positions): 0 literal, 1 the match, 2 the match one byte shorter
int zmi_launch_parse(const uint32_t* d_len, uint32_t first_shard, uint32_t n_shards, uint32_t max_len, const uint32_t* d_match,
                     uint64_t match_stride, uint32_t* d_dec, uint64_t dec_stride, uint32_t pieces, uint32_t strategy, uint32_t span_chunks,
                     hipStream_t stream);
int zmi_launch_inflate(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_streams,
                       uint32_t wrap, uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                       uint32_t* d_out_len, uint32_t* d_in_used, uint32_t* d_check, int32_t* d_status,
                       uint64_t* d_bitmap, uint64_t bitmap_words, uint64_t* d_bm_off, const uint32_t* d_out_hist,
                       const uint32_t* d_in_bit, uint32_t* d_resume, uint32_t* d_order, uint32_t mw_max, hipStream_t stream);
// the size pass (the decode kernel counting instead of storing) and the packed call's plan / mark kernels
int zmi_launch_inflate_sizes(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_streams,
                             uint32_t wrap, uint32_t hist, uint32_t size_limit, uint32_t* d_size, int32_t* d_status,
                             uint32_t* d_in_used, int32_t* d_detail, uint32_t* d_order, uint32_t mw_max, hipStream_t stream);
int zmi_launch_inflate_pack_plan(const uint32_t* d_size, uint32_t n_streams, uint32_t align, uint64_t out_cap, uint64_t* d_out_off,
                                 uint32_t* d_cap, hipStream_t stream);
int zmi_launch_inflate_pack_mark(const uint32_t* d_size, const uint64_t* d_out_off, uint32_t n_streams, uint64_t out_cap,
                                 uint32_t* d_out_len, int32_t* d_status, uint32_t* d_in_used, int32_t* d_detail, hipStream_t stream);
int zmi_launch_resolve_jump(uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_len, uint32_t n_streams,
                            const uint64_t* d_bitmap, const uint64_t* d_bm_off, int32_t* d_ptr, uint64_t n_idx, uint32_t rounds,
                            uint32_t* d_flags, hipStream_t stream);
int zmi_launch_resolve_jump_segments(uint8_t* d_fin, const uint64_t* d_soff, uint32_t nseg, const uint64_t* d_bitmap,
                                     const uint64_t* d_bm_off, int32_t* d_ptr, uint64_t total, uint32_t hist_len, uint32_t rounds,
                                     uint32_t* d_flags, uint32_t* d_err, const uint64_t* d_one_off, const uint32_t* d_one_len,
                                     hipStream_t stream);
int zmi_launch_inflate_resolve(uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_len, uint32_t n_streams,
                               const uint64_t* d_bitmap, const uint64_t* d_bm_off, const uint32_t* d_out_hist,
                               const uint32_t* d_order, hipStream_t stream);
// the batch with one shared preset dictionary (inflate.hip): every stream's `hist`, the resolve pass that reads the dictionary's image,
// the DICTID check; and the check of every stream's trailer against the sums of the produced bytes
int zmi_launch_inflate_shared_hist(uint32_t* d_hist, uint32_t n_streams, uint32_t hist, hipStream_t stream);
int zmi_launch_inflate_resolve_shared(uint8_t* d_out, const uint64_t* d_out_off, const uint32_t* d_out_len, uint32_t n_streams,
                                      const uint64_t* d_bitmap, const uint64_t* d_bm_off, const uint32_t* d_order,
                                      const uint8_t* d_img, uint32_t hist, hipStream_t stream);
int zmi_launch_inflate_dictid(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n_streams,
                              const uint32_t* d_dictid, int32_t* d_status, int32_t* d_detail, uint32_t* d_out_len,
                              hipStream_t stream);
int zmi_launch_inflate_verify(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len,
                              uint32_t n_streams, uint32_t wrap, const uint32_t* d_check, const uint32_t* d_adler,
                              const uint32_t* d_crc, int32_t* d_status, int32_t* d_detail, hipStream_t stream);
// single-stream inflate (inflate.hip): header, piece layout from the cuts, cut verification, symbolic resolve, window scan,
// substitute, trailer; proposals of cuts
int zmi_launch_si_header(const uint8_t* d_in, uint64_t n, uint32_t wrap, uint32_t* d_hdr, hipStream_t stream);
int zmi_launch_si_setup(const uint64_t* d_cuts, uint32_t n_cuts, uint64_t in_len, uint32_t first, uint32_t cnt, uint64_t stride,
                        uint32_t cap, uint64_t* d_in_off, uint32_t* d_in_n, uint64_t* d_out_off, uint32_t* d_ocap, uint32_t* d_hist,
                        hipStream_t stream);
int zmi_launch_si_verify(const uint64_t* d_cuts, uint32_t n_cuts, uint32_t first, uint32_t cnt, const uint32_t* d_in_n,
                         const uint32_t* d_olen, const int32_t* d_st, const int32_t* d_det, const uint32_t* d_res, uint32_t cap,
                         uint32_t* d_len, uint64_t* d_bad, uint64_t* d_tail, hipStream_t stream);
int zmi_launch_si_resolve(const uint8_t* d_dec, uint64_t stride, const uint32_t* d_out_len, uint32_t cap, uint32_t n,
                          const uint64_t* d_bitmap, const uint64_t* d_bm_off, uint16_t* d_sym, hipStream_t stream);
uint32_t zmi_si_scan_blocks(uint32_t n, uint32_t B);
int zmi_launch_si_window_scan(const uint16_t* d_sym, uint64_t stride, const uint32_t* d_len, uint32_t n, uint32_t B, uint16_t* d_agg,
                              uint8_t* d_carry, uint8_t* d_wstart, uint8_t* d_win, hipStream_t stream);
int zmi_launch_si_subst(const uint16_t* d_sym, uint64_t stride, const uint32_t* d_len, const uint64_t* d_off, const uint8_t* d_win,
                        uint32_t n, uint32_t piece_cap, uint32_t first, uint8_t* d_out, uint64_t out_cap, uint64_t* d_bad,
                        hipStream_t stream);
// cut_shift: 0 for cuts in bytes, 3 for cuts in bits (*d_cut0 must be the end of the header in that unit)
int zmi_launch_si_final(const uint8_t* d_in, uint64_t in_len, const uint32_t* d_hdr, const uint64_t* d_cut0, uint32_t cut_shift,
                        const uint64_t* d_bad, const uint64_t* d_tail, const uint64_t* d_total, const uint32_t* d_adler, const uint32_t* d_crc,
                        uint64_t out_cap, int32_t* d_status, int32_t* d_detail, uint64_t* d_out_len, uint64_t* d_in_used, hipStream_t stream);
// the same two steps for cuts at BIT positions (zmi_inflate_stream_bits_dev): d_in_bit[i] = the bit of its first byte piece i starts at
int zmi_launch_si_setup_bits(const uint64_t* d_cuts, uint32_t n_cuts, uint64_t in_len, uint32_t first, uint32_t cnt, uint64_t stride,
                             uint32_t cap, uint64_t* d_in_off, uint32_t* d_in_n, uint64_t* d_out_off, uint32_t* d_ocap, uint32_t* d_hist,
                             uint32_t* d_in_bit, hipStream_t stream);
int zmi_launch_si_verify_bits(const uint64_t* d_cuts, uint32_t n_cuts, uint32_t first, uint32_t cnt, const uint32_t* d_in_n,
                              const uint32_t* d_olen, const int32_t* d_st, const int32_t* d_det, const uint32_t* d_res, uint32_t cap,
                              uint32_t* d_len, uint64_t* d_bad, uint64_t* d_tail, hipStream_t stream);
int zmi_launch_si_clamp(const uint32_t* d_len, const uint64_t* d_off, uint32_t n, uint64_t out_cap, uint32_t* d_clen, hipStream_t stream);
int zmi_launch_si_find_cuts(const uint8_t* d_in, uint64_t n, const uint32_t* d_hdr, uint32_t* d_seg, uint64_t min_gap, uint64_t* d_cuts,
                            uint32_t cap, uint32_t* d_n_cuts, hipStream_t stream);
// random access into one stream (inflate.hip): the index kept by zmi_inflate_stream_index_dev -- the greedy selection of one launch
// group's piece starts (its state is *d_n_points, d_ix_out[count - 1], *d_max_gap), the windows of the selected pieces, the closing
// step -- and the plan / history / finish steps of zmi_inflate_ranges_dev.  d_u32: eight u32[g] tables, d_ioff / d_ooff: u64[g]
int zmi_launch_ix_select(const uint64_t* d_cuts, const uint64_t* d_off, uint32_t first, uint32_t cnt, uint64_t span, uint64_t* d_ix_bit,
                         uint64_t* d_ix_out, uint32_t ix_cap, uint32_t* d_n_points, uint64_t* d_max_gap, hipStream_t stream);
int zmi_launch_ix_gather(const uint64_t* d_cuts, const uint64_t* d_off, uint32_t first, uint32_t cnt, const uint64_t* d_ix_bit,
                         const uint64_t* d_ix_out, const uint32_t* d_n_points, const uint8_t* d_win, uint8_t* d_ix_win, hipStream_t stream);
int zmi_launch_ix_final(const int32_t* d_status, const uint64_t* d_total, uint64_t* d_ix_out, uint32_t* d_n_points, uint64_t* d_max_gap,
                        hipStream_t stream);
int zmi_launch_rg_plan(const uint64_t* d_ix_bit, const uint64_t* d_ix_out, uint32_t n_points, uint32_t has_win, uint64_t in_len,
                       uint64_t max_gap, const uint64_t* d_lo, const uint32_t* d_len, uint32_t first, uint32_t cnt, uint32_t max_len,
                       uint64_t rstride, uint64_t* d_ioff, uint64_t* d_ooff, uint32_t* d_u32, uint32_t g, hipStream_t stream);
int zmi_launch_rg_hist(const uint8_t* d_ix_win, const uint32_t* d_u32, uint32_t g, uint32_t cnt, uint64_t rstride, uint8_t* d_work,
                       hipStream_t stream);
int zmi_launch_rg_finish(uint64_t* d_ioff, uint64_t* d_ooff, uint32_t* d_u32, uint32_t g, const uint32_t* d_olen, const int32_t* d_st,
                         const int32_t* d_det, uint32_t first, uint32_t cnt, const uint64_t* d_out_off, uint64_t out_stride, uint32_t* d_got,
                         int32_t* d_status, uint64_t* d_c_src, uint32_t* d_c_len, uint64_t* d_c_dst, hipStream_t stream);
// the block scan (blockscan.hip): the host-buffer form of zmi_inflate_blocks, and one window of the ordered form of
// zmi_stream_find_blocks_dev
int zmi_launch_block_scan(const uint8_t* d_in, uint32_t n, uint64_t first_bit, uint32_t* d_pre, uint32_t pre_cap, uint32_t* d_list,
                          uint32_t cap, uint32_t* d_count, hipStream_t stream);
uint32_t zmi_block_scan_groups(uint32_t own_bits);
uint32_t zmi_block_scan_slot(void);
uint32_t zmi_block_scan_look(void);
int zmi_launch_block_scan_window(const uint8_t* d_win, uint32_t n_vis, uint64_t base_bit, uint32_t own_bits, const uint32_t* d_hdr,
                                 uint32_t* d_slots, uint32_t* d_cnt, uint32_t* d_vcnt, uint64_t* d_voff, uint32_t* d_vlist, uint32_t vcap,
                                 uint64_t gap_bits, uint32_t first, uint64_t* d_cuts, uint32_t cap, uint32_t* d_n_cuts, hipStream_t stream);
// BGZF (pack.hip): the batch call's length check, the framed sizes with the choice between the encoder's slot and a stored block,
// the members written in one pass (n blocks of one launch group: slot i at d_slots + i * slot_stride), the closing step (total,
// Z_BUF_ERROR, the end-of-file block)
int zmi_launch_bgzf_lens(const uint32_t* d_len, uint32_t n, uint32_t max_len, uint32_t* d_clen, int32_t* d_status, hipStream_t stream);
int zmi_launch_bgzf_sizes(const uint32_t* d_len, const uint32_t* d_olen, const int32_t* d_st, uint32_t n, uint32_t* d_framed,
                          uint32_t* d_stored, int32_t* d_status, hipStream_t stream);
int zmi_launch_bgzf_pack(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_len, const uint8_t* d_slots,
                         uint64_t slot_stride, const uint32_t* d_olen, const uint32_t* d_stored, const uint32_t* d_crc, uint32_t n,
                         uint32_t max_len, uint8_t* d_out, const uint64_t* d_boff, uint64_t out_cap, hipStream_t stream);
int zmi_launch_bgzf_close(uint8_t* d_out, uint64_t out_cap, const uint64_t* d_blocks_end, uint32_t eof, uint64_t* d_out_len,
                          int32_t* d_status, hipStream_t stream);
// writing ZIP archives (pack.hip, checksum.hip): the entries' checked lengths and piece counts; the piece table (d_first: the scan of
// the counts, *d_sum: the sum of the lengths, d_ends: the bitmap of chain mode 2, wpg words per launch group of `group` pieces);
// one group's places and payload copies; the CRC-32 of every entry from its pieces'; the local headers and the sizes of the central
// records (pass 0), the central records and d_entries (pass 1); the end structure, *d_out_len, d_info and Z_BUF_ERROR
int zmi_launch_zip_layout(const uint32_t* d_in_len, const uint64_t* d_name_off, uint32_t n, uint32_t piece_bytes, uint32_t* d_elen,
                          uint32_t* d_nlen, uint32_t* d_npc, uint64_t* d_sum, int32_t* d_status, hipStream_t stream);
int zmi_launch_zip_pieces(const uint64_t* d_in_off, const uint32_t* d_elen, const uint32_t* d_nlen, const uint64_t* d_first,
                          const uint64_t* d_sum, uint32_t n, uint64_t in_bytes, uint32_t piece_bytes, uint32_t cap, uint32_t group,
                          uint32_t wpg, uint64_t* d_p_off, uint32_t* d_p_len, uint32_t* d_head, uint32_t* d_ends, uint32_t* d_n_eff,
                          int32_t* d_status, hipStream_t stream);
int zmi_launch_zip_sizes(const uint32_t* d_head, const uint32_t* d_olen, const int32_t* d_st, uint32_t n, uint32_t* d_size, int32_t* d_status,
                         hipStream_t stream);
int zmi_launch_zip_pack(const uint8_t* d_in, const uint64_t* d_p_off, const uint32_t* d_head, const uint8_t* d_slots, uint64_t slot_stride,
                        const uint32_t* d_olen, uint32_t n, uint32_t max_len, uint8_t* d_out, const uint64_t* d_pos, uint64_t out_cap,
                        hipStream_t stream);
int zmi_launch_combine_segments(const uint32_t* d_check, const uint32_t* d_len, const uint64_t* d_first, uint32_t n, const uint32_t* d_n_live,
                                uint32_t* d_out, hipStream_t stream);
int zmi_launch_zip_headers(const uint32_t* d_elen, const uint32_t* d_nlen, const uint64_t* d_first, const uint64_t* d_pos, const uint32_t* d_crc,
                           const uint8_t* d_names, const uint64_t* d_name_off, const uint32_t* d_dos_time, const uint32_t* d_ext_attr, uint32_t n,
                           const uint32_t* d_n_eff, uint32_t method, uint64_t base, uint8_t* d_out, uint64_t out_cap, uint32_t* d_cen_size,
                           const uint64_t* d_cen_off, zmi_zip_entry* d_entries, uint32_t pass, int32_t* d_status, hipStream_t stream);
int zmi_launch_zip_close(uint8_t* d_out, uint64_t out_cap, const uint64_t* d_pay_end, const uint64_t* d_cd_end, const uint32_t* d_n_eff,
                         uint64_t base, uint64_t* d_out_len, zmi_zip_info* d_info, int32_t* d_status, hipStream_t stream);
// multi-member gzip files: proposals of member starts (pack.hip: count, scan, gather) and the plan / verify / repair steps of
// zmi_inflate_members_dev (inflate.hip).  d_tab: eight u32[n] tables, d_off: u64[n + 1], d_w: sixteen words
uint32_t zmi_mm_scan_segments(uint64_t in_len, uint32_t head);
int zmi_launch_mm_find(const uint8_t* d_in, uint64_t in_len, uint32_t* d_cnt, uint64_t* d_off, uint64_t* d_starts, uint32_t cap,
                       uint32_t* d_n_starts, hipStream_t stream);
int zmi_launch_mm_init(const uint64_t* d_starts, uint32_t n, uint64_t in_len, uint32_t* d_tab, uint64_t* d_off, uint32_t* d_w, hipStream_t stream);
int zmi_launch_mm_plan(const uint64_t* d_starts, uint32_t n, uint32_t* d_tab, uint64_t* d_off, uint32_t* d_w, const uint8_t* d_in,
                       uint64_t in_len, uint32_t pass, hipStream_t stream);
int zmi_launch_mm_setup(const uint64_t* d_starts, uint32_t n, uint32_t* d_tab, uint64_t* d_off, uint32_t* d_w, uint64_t out_cap, uint64_t half,
                        uint32_t grp, uint64_t* g_ioff, uint32_t* g_in, uint64_t* g_ooff, uint32_t* g_cap, hipStream_t stream);
int zmi_launch_mm_collect(const uint64_t* d_starts, uint32_t n, uint32_t* d_tab, uint64_t* d_off, uint32_t* d_w, uint64_t out_cap, uint64_t half,
                          uint32_t grp, const uint32_t* g_olen, const int32_t* g_st, const uint32_t* g_used, const int32_t* g_det,
                          hipStream_t stream);
int zmi_launch_mm_verify(const uint64_t* d_starts, uint32_t n, uint32_t* d_tab, uint64_t* d_off, uint32_t* d_w, uint64_t out_cap, uint32_t pass,
                         int repair, hipStream_t stream);
int zmi_launch_mm_lr_setup(const uint64_t* d_starts, uint32_t n, uint32_t* d_tab, uint64_t* d_off, uint32_t* d_w, uint64_t in_len,
                           uint64_t out_cap, uint64_t room_max, uint64_t* l_ioff, uint32_t* l_in, uint64_t* l_ooff, uint32_t* l_cap,
                           hipStream_t stream);
int zmi_launch_mm_final(const uint64_t* d_starts, uint32_t n, uint32_t* d_tab, uint64_t* d_off, uint32_t* d_w, const uint8_t* d_in,
                        uint64_t in_len, uint64_t out_cap, const uint64_t* d_rank, const uint32_t* lr_olen, const int32_t* lr_st,
                        const uint32_t* lr_used, const int32_t* lr_det, const uint32_t* chk_trailer, const uint32_t* chk_crc,
                        uint64_t* d_out_len, uint64_t* d_in_used, uint32_t* d_members, uint64_t* d_member_off, int32_t* d_status,
                        int32_t* d_detail, hipStream_t stream);
// ZIP archives (pack.hip): the directory -- locate, the chain (segments followed side by side, the stitching walk), parse; d_w four
// words, d_chain u64[cap], d_seg four words per segment of zmi_zip_segments(in_len), stages 1 .. 3 = how many of the three run -- and
// the two kernels around the batch decoder: the tables of the selected slots, and the slots' final words
uint32_t zmi_zip_walk_tile(void);
uint64_t zmi_zip_segments(uint64_t in_len);
int zmi_launch_zip_directory(const uint8_t* d_in, uint64_t in_len, zmi_zip_entry* d_entries, uint32_t cap, zmi_zip_info* d_info, uint64_t* d_w,
                             uint64_t* d_chain, uint64_t* d_seg, uint32_t stages, hipStream_t stream);
int zmi_launch_zip_prep(const zmi_zip_entry* d_entries, uint32_t n_entries, const uint32_t* d_sel, uint32_t n_sel, uint64_t in_len,
                        uint64_t* d_in_off, uint32_t* d_in_n, uint32_t* d_size, uint32_t* d_slen, hipStream_t stream);
int zmi_launch_zip_verify(const zmi_zip_entry* d_entries, uint32_t n_entries, const uint32_t* d_sel, uint32_t n_sel, uint64_t in_len,
                          const uint64_t* d_out_off, uint64_t out_cap, const uint32_t* d_used, const uint32_t* d_crc, uint32_t* d_out_len,
                          int32_t* d_status, int32_t* d_detail, hipStream_t stream);
// PNG images (png_kernels.h, compiled into pack.hip): the records; the slots' sizes (pass 0: d_pix, for the plan of the regions; pass 1,
// behind it: scanline sizes, gather sizes, bands of 64 rows, cleared flag words); the walk (chunk CRC-32, the gather of several IDAT
// chunks, where the decoder reads each slot's stream); the unfilter over the items -- d_item_off the scan of the bands, bound what it
// can sum to; the slots' final words
uint32_t zmi_png_strip(void);
int zmi_launch_png_headers(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, zmi_png_image* d_images,
                           hipStream_t stream);
int zmi_launch_png_prep(const zmi_png_image* d_images, uint32_t n_images, const uint32_t* d_sel, uint32_t n_sel, const uint32_t* d_in_len,
                        uint32_t pass, uint32_t* d_pix, const uint32_t* d_pcap, uint32_t* d_ssz, uint32_t* d_gsz, uint32_t* d_items, uint32_t* d_fl,
                        hipStream_t stream);
int zmi_launch_png_walk(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_png_image* d_images,
                        const uint32_t* d_sel, uint32_t n_sel, const uint32_t* d_ssz, const uint32_t* d_gsz, const uint64_t* d_goff,
                        const uint32_t* d_gcap, uint8_t* d_gbuf, uint32_t check_crc, uint64_t* d_zin_off, uint32_t* d_zin_len, uint32_t* d_fl,
                        hipStream_t stream);
int zmi_launch_png_unfilter(const zmi_png_image* d_images, const uint32_t* d_sel, uint32_t n_sel, const uint64_t* d_item_off, uint64_t bound,
                            const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_ssz, const uint32_t* d_slen, const int32_t* d_sst,
                            uint8_t* d_out, const uint64_t* d_out_off, uint32_t native16, uint32_t split, uint32_t* d_fl, hipStream_t stream);
int zmi_launch_png_finish(const zmi_png_image* d_images, uint32_t n_images, const uint32_t* d_sel, uint32_t n_sel, const uint32_t* d_in_len,
                          const uint64_t* d_out_off, uint64_t out_cap, const uint32_t* d_ssz, const uint32_t* d_slen, const int32_t* d_sst,
                          const uint32_t* d_fl, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, hipStream_t stream);
// writing PNG images (png_kernels.h; the piece table and the payload copies are zmi_launch_zip_pieces / zmi_launch_zip_pack): the images'
// scanline sizes, piece counts and bands of rows (*d_sum: the sum of the sizes); the forward filter over the items -- d_item_off the scan
// of the bands -- into the scanline scratch at d_soff; one launch group's places (d_pos[0]: where it starts,
// d_ends: the group's bitmap); the Adler-32 of every image from its pieces' (checksum.hip); the files' fixed bytes and the images' words
uint32_t zmi_png_filter_tile(void);
int zmi_launch_png_wlayout(const zmi_png_image* d_images, const uint32_t* d_in_len, uint32_t n, uint32_t piece_bytes, uint32_t* d_ssz,
                           uint32_t* d_nlen, uint32_t* d_npc, uint32_t* d_bands, uint64_t* d_sum, hipStream_t stream);
int zmi_launch_png_filter(const zmi_png_image* d_images, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                          const uint64_t* d_item_off, const uint64_t* d_sum, uint64_t scan_bytes, uint8_t* d_scan,
                          const uint64_t* d_soff, uint32_t filter, uint32_t native16, hipStream_t stream);
int zmi_launch_png_place(const uint32_t* d_head, const uint32_t* d_olen, const uint32_t* d_ends, uint32_t n, uint32_t align, uint64_t* d_pos,
                         hipStream_t stream);
int zmi_launch_combine_segments_adler(const uint32_t* d_check, const uint32_t* d_len, const uint64_t* d_first, uint32_t n,
                                      const uint32_t* d_n_live, uint32_t* d_out, hipStream_t stream);
int zmi_launch_png_wfinish(const zmi_png_image* d_images, const uint32_t* d_in_len, uint32_t n, const uint32_t* d_n_eff, const uint64_t* d_first,
                           const uint64_t* d_pos, const uint32_t* d_olen, const int32_t* d_st, const uint32_t* d_adler, const uint32_t* d_crc,
                           uint32_t level, uint32_t strategy, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len,
                           int32_t* d_status, zmi_png_image* d_written, hipStream_t stream);
// TIFF files (tiff_kernels.h, compiled into pack.hip): the IFD chain and the pages' records (d_ifd_pos: cap words of scratch); the slots'
// tables (pass 0 in front of the plan, pass 1 behind it and behind the scan d_pix_off of the decoded sizes); the unpredict over the row
// groups -- d_item_off the scan of d_items -- from the scratch at d_soff to the regions; the slots' final words
uint32_t zmi_tiff_row_tile(void);
int zmi_launch_tiff_directory(const uint8_t* d_in, uint64_t in_len, zmi_tiff_page* d_pages, uint32_t cap, zmi_tiff_info* d_info,
                              uint64_t* d_ifd_pos, hipStream_t stream);
int zmi_launch_tiff_slots(const uint8_t* d_in, uint64_t in_len, const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page,
                          const uint32_t* d_sel, uint32_t n_sel, uint32_t assemble, uint32_t pass, uint64_t out_cap, uint64_t decoded_bytes,
                          const uint64_t* d_pix_off, uint32_t* d_pix, uint32_t* d_pcap, uint64_t* d_zin_off, uint32_t* d_zin_len,
                          uint32_t* d_ssz, uint32_t* d_rawlen, uint32_t* d_items, uint32_t* d_fl, uint64_t* d_out_off, hipStream_t stream);
int zmi_launch_tiff_unpredict(const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page, const uint32_t* d_sel, uint32_t n_sel,
                              uint64_t in_len, uint32_t assemble, const uint64_t* d_item_off, uint64_t bound, uint8_t* d_sbuf,
                              const uint64_t* d_soff, const uint32_t* d_ssz, const uint32_t* d_slen, const int32_t* d_sst,
                              const uint32_t* d_rawlen, const uint32_t* d_fl, uint8_t* d_out, const uint64_t* d_out_off, hipStream_t stream);
int zmi_launch_tiff_finish(const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page, const uint32_t* d_sel, uint32_t n_sel,
                           uint64_t in_len, uint32_t assemble, uint64_t out_cap, uint64_t decoded_bytes, const uint64_t* d_pix_off,
                           const uint64_t* d_out_off, const uint32_t* d_ssz, const uint32_t* d_slen, const int32_t* d_sst,
                           const uint32_t* d_fl, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, hipStream_t stream);
// writing TIFF files (tiff_write_kernels.h, compiled into pack.hip; the payload copies are zmi_launch_zip_pack, the fold per segment
// zmi_launch_combine_segments_adler): the piece table, which follows from the plan alone (d_first: n_segs + 1 words, *d_n_eff = n_segs,
// d_pos[0] = where segment 0 starts); the forward predictor into the scratch, segment k at k * plan.ss; one launch group's places
// (zmi_launch_png_place with a tail of 4 bytes in place of 20); the fixed bytes that follow from *w alone; per segment the zlib frame,
// the gap in front, its two array entries and its words (*d_bad, set to all ones by the caller: the first segment whose status is not
// 0); the file's words
uint32_t zmi_tiff_predict_tile(void);
int zmi_launch_tiff_wpieces(zmi_tw_plan plan, uint32_t group, uint32_t wpg, uint64_t* d_p_off, uint32_t* d_p_len, uint32_t* d_head,
                            uint32_t* d_ends, uint64_t* d_first, uint32_t* d_n_eff, uint64_t* d_pos, hipStream_t stream);
int zmi_launch_tiff_predict(zmi_tw_plan plan, const uint8_t* d_in, const uint64_t* d_in_off, uint8_t* d_scan, hipStream_t stream);
int zmi_launch_tiff_place(const uint32_t* d_head, const uint32_t* d_olen, const uint32_t* d_ends, uint32_t n, uint32_t align, uint64_t* d_pos,
                          hipStream_t stream);
int zmi_launch_tiff_wmeta(zmi_tw_meta meta, uint8_t* d_out, uint64_t out_cap, hipStream_t stream);
int zmi_launch_tiff_wsegs(zmi_tw_plan plan, const uint64_t* d_pos, const uint32_t* d_olen, const int32_t* d_st, const uint32_t* d_adler,
                          uint32_t level, uint32_t strategy, uint8_t* d_out, uint64_t out_cap, uint32_t* d_seg_len, int32_t* d_status,
                          uint32_t* d_bad, hipStream_t stream);
int zmi_launch_tiff_wclose(zmi_tw_plan plan, zmi_tw_meta meta, const uint64_t* d_pos, const uint32_t* d_olen, const int32_t* d_status,
                           const uint32_t* d_bad, uint64_t out_cap, uint64_t* d_file_len, int32_t* d_file_status, void* d_written,
                           hipStream_t stream);
// OpenEXR images (exr_kernels.h, compiled into pack.hip): the records; the slots' sizes (pass 0, in front of the plan and the scans of the
// chunk counts and raw bytes) and which of them are read (pass 1); the chunks' tables over chunk_cap entries; one byte sum per block of
// every inflated chunk and their scan per chunk (bound: the words of d_bsum and of d_bpre); the unzip over the items -- d_item_off the
// scan of d_items -- from the scratch at d_soff to the planes; the slots' final words
uint32_t zmi_exr_trip(void);
uint32_t zmi_exr_piece(void);
int zmi_launch_exr_headers(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, zmi_exr_image* d_images,
                           zmi_exr_channel* d_chans, uint32_t chan_cap, hipStream_t stream);
int zmi_launch_exr_slots(const uint32_t* d_in_len, const zmi_exr_image* d_images, const zmi_exr_channel* d_chans, uint32_t chan_cap,
                         uint32_t n_files, const uint32_t* d_sel, uint32_t n_sel, uint32_t pass, uint64_t chunk_cap, uint64_t decoded_bytes,
                         const uint32_t* d_pcap, const uint64_t* d_ch_off, const uint64_t* d_raw_off, uint32_t* d_size, uint32_t* d_nch,
                         uint32_t* d_rawb, uint32_t* d_kind, uint32_t* d_live, hipStream_t stream);
int zmi_launch_exr_chunks(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_exr_image* d_images,
                          const zmi_exr_channel* d_chans, uint32_t chan_cap, const uint32_t* d_sel, uint32_t n_sel, const uint64_t* d_ch_off,
                          const uint32_t* d_live, uint32_t chunk_cap, uint64_t* d_zin_off, uint32_t* d_zin_len, uint32_t* d_csz,
                          uint32_t* d_rawlen, uint32_t* d_fl, uint32_t* d_items, uint32_t* d_nblk, uint32_t* d_cslot, uint32_t* d_cm, uint32_t* d_pitems,
                          hipStream_t stream);
// PXR24 (compression 5): the decoder's capacities from the lengths the streams must inflate to; the undo over the items of its own scan
uint32_t zmi_exr_pxr24_trip(void);
int zmi_launch_exr_deccap(const uint32_t* d_csz, const uint32_t* d_scap, const uint32_t* d_cm, uint32_t chunk_cap, uint32_t* d_dcap,
                          hipStream_t stream);
int zmi_launch_exr_pxr24_undo(const zmi_exr_image* d_images, const zmi_exr_channel* d_chans, uint32_t chan_cap, const uint32_t* d_sel,
                              const uint64_t* d_ch_off, const uint32_t* d_cslot, uint32_t chunk_cap, const uint64_t* d_pitem_off, uint64_t bound,
                              const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_csz, const uint32_t* d_scap, const uint32_t* d_cm,
                              const uint32_t* d_slen, const int32_t* d_sst, uint8_t* d_out, const uint64_t* d_out_off, hipStream_t stream);
int zmi_launch_exr_blocksum(const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_csz, const uint32_t* d_scap,
                            const uint64_t* d_blk_off, uint32_t chunk_cap, uint64_t bound, uint32_t* d_bsum, uint32_t* d_bpre, hipStream_t stream);
int zmi_launch_exr_unzip(const zmi_exr_image* d_images, const zmi_exr_channel* d_chans, uint32_t chan_cap, const uint32_t* d_sel,
                         const uint64_t* d_ch_off, const uint32_t* d_cslot, uint32_t chunk_cap, const uint64_t* d_item_off, uint64_t bound,
                         const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_csz, const uint32_t* d_scap, const uint32_t* d_slen,
                         const int32_t* d_sst, const uint32_t* d_rawlen, const uint64_t* d_blk_off, const uint32_t* d_bpre, uint8_t* d_out,
                         const uint64_t* d_out_off, hipStream_t stream);
int zmi_launch_exr_finish(const zmi_exr_image* d_images, const uint32_t* d_sel, uint32_t n_sel, const uint32_t* d_kind, const uint32_t* d_size,
                          const uint32_t* d_pcap, const uint64_t* d_ch_off, const uint64_t* d_raw_off, uint64_t chunk_cap, uint64_t decoded_bytes,
                          const uint32_t* d_csz, const uint32_t* d_scap, const uint32_t* d_rawlen, const uint32_t* d_fl, const uint32_t* d_cm,
                          const uint32_t* d_slen, const int32_t* d_sst, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail,
                          hipStream_t stream);
// writing OpenEXR images (exr_write_kernels.h, compiled into pack.hip; the payload copies are zmi_launch_zip_pack, the fold per chunk
// zmi_launch_combine_segments_adler): a slice of the host's bytes into the scratch; per chunk of the call its raw size, pieces, room in
// the scratch and work items (and the words the later kernels start from); the piece table over the scans of those; the forward zip
// over the items into the scratch; one launch group's places -- chunks first .. first + count, the raw decision, d_run[0] -> d_run[1];
// the raw chunks' gather from the planes; the fixed bytes; the images' words
uint32_t zmi_exr_zip_trip(void);
int zmi_launch_exr_wslice(zmi_xw_slice slice, uint8_t* d_blob, hipStream_t stream);
int zmi_launch_exr_wchunks(zmi_xw_plan plan, const zmi_exr_channel* d_chs, uint32_t* d_csz, uint32_t* d_npc, uint32_t* d_ssz, uint32_t* d_items,
                           uint32_t* d_cds, uint32_t* d_neff, uint32_t* d_bad, uint64_t* d_run, uint32_t* d_cm, uint32_t* d_fitems,
                           hipStream_t stream);
int zmi_launch_exr_pxr24_forward(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint8_t* d_in, const uint64_t* d_in_off,
                                 const uint64_t* d_fitem_off, uint64_t bound, const uint64_t* d_soff, uint8_t* d_scan, hipStream_t stream);
int zmi_launch_exr_wpieces(zmi_xw_plan plan, const uint64_t* d_cfirst, const uint64_t* d_soff, const uint32_t* d_csz, uint32_t group_chunks,
                           uint32_t wpg, uint32_t np, uint64_t* d_poff, uint32_t* d_plen, uint32_t* d_ends, hipStream_t stream);
int zmi_launch_exr_zip(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_item_off,
                       uint64_t bound, const uint64_t* d_soff, uint8_t* d_scan, hipStream_t stream);
int zmi_launch_exr_wplace(zmi_xw_plan plan, uint32_t first, uint32_t count, const uint64_t* d_cfirst, const uint32_t* d_csz,
                          const uint32_t* d_olen, const int32_t* d_st, uint64_t* d_run, uint32_t* d_cds, uint64_t* d_cpos, uint64_t* d_ppos,
                          uint32_t* d_phead, uint64_t* d_out_off, uint32_t* d_bad, hipStream_t stream);
int zmi_launch_exr_gather(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint8_t* d_in, const uint64_t* d_in_off,
                          const uint64_t* d_item_off, uint64_t bound, const uint32_t* d_csz, const uint32_t* d_cds, const uint64_t* d_cpos,
                          uint8_t* d_out, uint64_t out_cap, hipStream_t stream);
int zmi_launch_exr_wframe(zmi_xw_plan plan, const uint8_t* d_hdr, const uint32_t* d_csz, const uint32_t* d_cds, const uint64_t* d_cpos,
                          const uint32_t* d_cadler, const uint64_t* d_out_off, uint32_t level, uint32_t strategy, uint8_t* d_out, uint64_t out_cap,
                          hipStream_t stream);
int zmi_launch_exr_wwords(zmi_xw_plan plan, const zmi_exr_channel* d_chs, const uint32_t* d_cds, const uint64_t* d_cpos,
                          const uint64_t* d_out_off, const uint32_t* d_bad, const int32_t* d_st, uint64_t out_cap, uint32_t* d_out_len,
                          int32_t* d_status, zmi_exr_image* d_written, zmi_exr_channel* d_written_channels, hipStream_t stream);
}
