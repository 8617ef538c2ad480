// pack.hip -- turning the batch's strided output slots into dense, ordered byte ranges (the "stitch").
//
// What the reference does here: its parallel-deflate recipe compresses pieces independently and then simply appends
// the finished byte strings in order (zlib-rs/src/deflate.rs:4145-4221 `split_deflate`; multi-member gzip is read
// back the same way, libz-rs-sys/src/gz.rs:1464-1506).  On the device the compressed shards sit in compress_bound-
// strided slots (72 GiB of slots for ~29 GiB of data at the headline size), so the stitch is two small kernels:
//   zmi_scan_sizes_kernel   exclusive prefix sum of the u32 sizes -> u64 byte offsets (n + 1 entries)
//   zmi_copy_ranges_kernel  range i: len[i] bytes from src + src_off[i] to dst + dst_off[i], any alignment
// One call packs a rank's slots into its slab (src_off = i * stride, dst_off = scan); after the slab exchange the
// same kernel scatters a peer's slab into the globally ordered output (src_off = the peer's scan, dst_off = the
// global offsets of its shards).  HBM-bound: one read + one write of the compressed bytes; 4 KiB tiles are loaded
// with aligned 16-byte reads into LDS and stored as aligned dwords (source and destination are misaligned against
// each other in general), 256-thread workgroups, several workgroups per range so that a few large ranges still fill
// the chip.
#include "zmi_device.h"
#include "zmi_kernels.h"
#include "../../include/zmi355.h"   // zmi_zip_entry, zmi_zip_info, ZMI_ZA_* / ZMI_ZE_*

#define PK_T 256u
#define PK_TILE 4096u

// base (may be NULL): a device word the offsets start from -- the end of the previous launch group of a single stream
// (zmi_deflate_stream_dev), read before anything is written, so it may be off[0] itself
__global__ void __launch_bounds__(1024) zmi_scan_sizes_kernel(const uint32_t* __restrict__ len, uint32_t n,
                                                               uint64_t* off, const uint64_t* base) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t b = base ? *base : 0ull;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += len[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t o = b + part[t] - sum;
    for (uint32_t i = lo; i < hi; ++i) { off[i] = o; o += len[i]; }
    if (t == 1023u) off[n] = b + part[1023];
}

// Tiles part, part + split, ... of the l bytes at s go to dst + d0, either at any alignment, through the workgroup's stage of
// PK_TILE + 32 bytes; every thread of the workgroup calls it with the same arguments.  Nothing outside [s, s + l) is read, nothing
// outside [dst + d0, dst + d0 + l) written.
static __device__ __forceinline__ void pk_copy_tiles(uint8_t* stage, const uint8_t* s, uint32_t l, uint8_t* dst, uint64_t d0, uint32_t part,
                                                     uint32_t split, uint32_t t) {
    const uint32_t mis = (uint32_t)((uintptr_t)s & 15u);   // the tile loads start at the 16-byte line at or below s
    for (uint32_t base = part * PK_TILE; base < l; base += split * PK_TILE) {
        const uint32_t nb = l - base < PK_TILE ? l - base : PK_TILE;
        // stage[mis + k] = s[base + k]; 16-byte aligned loads, the first / last line of a range byte-wise
        const uint8_t* line0 = s + base - mis;
        const uint32_t span = mis + nb;
        for (uint32_t c = t * 16u; c < span; c += PK_T * 16u) {
            if (base + c >= mis && c + 16u <= span && (base != 0 || c >= 16u || mis == 0u)) {
                *(uint4*)(stage + c) = *(const uint4*)(line0 + c);
            } else {
                for (uint32_t j = 0; j < 16u; ++j)
                    if (c + j >= mis && c + j < span) stage[c + j] = line0[c + j];
            }
        }
        __syncthreads();
        uint8_t* A = dst + d0 + base;
        uint32_t head = (4u - (uint32_t)((uintptr_t)A & 3u)) & 3u;
        if (head > nb) head = nb;
        const uint32_t ndw = (nb - head) >> 2;
        uint32_t* A4 = (uint32_t*)(A + head);
        for (uint32_t k = t; k < ndw; k += PK_T) {
            const uint32_t o = mis + head + 4u * k;
            const uint32_t* w = (const uint32_t*)(stage + (o & ~3u));
            A4[k] = __builtin_amdgcn_alignbyte(w[1], w[0], o & 3u);
        }
        if (t == 0) {
            for (uint32_t j = 0; j < head; ++j) A[j] = stage[mis + j];
            for (uint32_t j = head + 4u * ndw; j < nb; ++j) A[j] = stage[mis + j];
        }
        __syncthreads();
    }
}

// n * split jobs: job b handles tiles b % split, b % split + split, ... of range b / split; the grid is the number of jobs, or
// fewer workgroups that take the jobs in turn (a destination in host memory: see zmi_launch_copy_ranges_few)
__global__ void __launch_bounds__(PK_T) zmi_copy_ranges_kernel(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_off,
                                                              uint64_t src_stride, const uint32_t* __restrict__ len,
                                                              uint8_t* __restrict__ dst, const uint64_t* __restrict__ dst_off,
                                                              uint64_t dst_cap, uint32_t split, uint32_t jobs) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[PK_TILE + 32];
    const uint32_t t = threadIdx.x;
  for (uint32_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const uint32_t r = job / split, part = job % split;
    const uint32_t l = len[r];
    const uint64_t so = src_off ? src_off[r] : (uint64_t)r * src_stride;
    const uint64_t d0 = dst_off[r];
    if (d0 + l > dst_cap) continue;   // does not fit: the caller sees that from the offsets
    pk_copy_tiles(stage, src + so, l, dst, d0, part, split, t);
  }
}

// out[i] = min(len[i], cap[i]): what a stream's output region really holds (inflate counts past a full region)
__global__ void __launch_bounds__(256) zmi_clamp_lens_kernel(const uint32_t* __restrict__ len, const uint32_t* __restrict__ cap, uint32_t n,
                                                             uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = len[i] < cap[i] ? len[i] : cap[i];
}
extern "C" int zmi_launch_clamp_lens(const uint32_t* d_len, const uint32_t* d_cap, uint32_t n, uint32_t* d_out, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_clamp_lens_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_len, d_cap, n, d_out);
    return 0;
}

extern "C" int zmi_launch_scan_sizes(const uint32_t* d_len, uint32_t n, uint64_t* d_off, hipStream_t stream) {
    ZMI_LAUNCH(zmi_scan_sizes_kernel, dim3(1), dim3(1024), 0, stream, d_len, n, d_off, (const uint64_t*)nullptr);
    return 0;
}
extern "C" int zmi_launch_scan_sizes_base(const uint32_t* d_len, uint32_t n, uint64_t* d_off, const uint64_t* d_base, hipStream_t stream) {
    ZMI_LAUNCH(zmi_scan_sizes_kernel, dim3(1), dim3(1024), 0, stream, d_len, n, d_off, d_base);
    return 0;
}

extern "C" int zmi_launch_copy_ranges(const uint8_t* d_src, const uint64_t* d_src_off, uint64_t src_stride, const uint32_t* d_len,
                                      uint32_t n, uint8_t* d_dst, const uint64_t* d_dst_off, uint64_t dst_cap, uint32_t max_len,
                                      hipStream_t stream) {
    if (n == 0) return 0;
    // a few thousand workgroups fill the chip; small batches of large ranges are split across workgroups
    uint32_t split = 1;
    const uint32_t tiles = (max_len + PK_TILE - 1u) / PK_TILE;
    while ((uint64_t)n * split < 4096u && split < tiles) split <<= 1;
    ZMI_LAUNCH(zmi_copy_ranges_kernel, dim3(n * split), dim3(PK_T), 0, stream, d_src, d_src_off, src_stride, d_len, d_dst, d_dst_off,
               dst_cap, split, n * split);
    return 0;
}

// The same copy with `groups` workgroups only, for a destination in pinned HOST memory (the host-buffer pipeline's slab): the
// stores leave over PCIe at ~50 GB/s whatever the launch looks like, and a launch of thousands of workgroups sits on every CU
// for the 5 ms that takes -- the next chunk's match search (one 1024-thread workgroup per CU, 152 KiB of LDS) could not
// start beside it.  A few dozen workgroups keep the link busy and leave the CUs to the kernels.
extern "C" int zmi_launch_copy_ranges_few(const uint8_t* d_src, const uint64_t* d_src_off, uint64_t src_stride, const uint32_t* d_len,
                                          uint32_t n, uint8_t* d_dst, const uint64_t* d_dst_off, uint64_t dst_cap, uint32_t max_len,
                                          uint32_t groups, hipStream_t stream) {
    if (n == 0) return 0;
    uint32_t split = 1;
    const uint32_t tiles = (max_len + PK_TILE - 1u) / PK_TILE;
    while ((uint64_t)n * split < 4096u && split < tiles) split <<= 1;
    // the `groups` workgroups that run at a time should work on ONE range, tile beside tile (job = range * split + part, the
    // workgroups take consecutive jobs): sixteen workgroups writing sixteen different megabytes of host memory ran at a
    // quarter of the link's rate (the inflate pipeline's per-stream ranges: 19 -> 5 GiB/s until this was fixed)
    while (split < groups && split < tiles) split <<= 1;
    const uint64_t jobs64 = (uint64_t)n * split;
    const uint32_t jobs = jobs64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)jobs64;
    ZMI_LAUNCH(zmi_copy_ranges_kernel, dim3(jobs < groups ? jobs : groups), dim3(PK_T), 0, stream, d_src, d_src_off, src_stride, d_len, d_dst,
               d_dst_off, dst_cap, split, jobs);
    return 0;
}

// ---- the single stream (zmi_deflate_stream_dev, zmi_stream_frame_dev) -------------------------------------------------------
// The reference's split_deflate (zlib-rs/src/deflate.rs:4145-4221) writes the wrapper once, every piece but the last behind a
// flush marker, and one trailer with the combined check value.  The pieces' deflate bytes are packed by the copy kernel above at
// d_out + h; these kernels lay the pieces out and write what surrounds them.

// piece i of an n-byte buffer: [i * piece_bytes, + min(piece_bytes, n - i * piece_bytes)); n = 0 is one empty piece
__global__ void __launch_bounds__(256) zmi_piece_layout_kernel(uint64_t n, uint32_t piece_bytes, uint32_t count, uint64_t* __restrict__ off,
                                                               uint32_t* __restrict__ len) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint64_t o = (uint64_t)i * piece_bytes;
    off[i] = o;
    len[i] = n - o < piece_bytes ? (uint32_t)(n - o) : piece_bytes;
}
extern "C" int zmi_launch_piece_layout(uint64_t n, uint32_t piece_bytes, uint32_t count, uint64_t* d_off, uint32_t* d_len, hipStream_t stream) {
    if (count == 0) return 0;
    ZMI_LAUNCH(zmi_piece_layout_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, n, piece_bytes, count, d_off, d_len);
    return 0;
}

// header bytes of deflateInit2_(level, Z_DEFLATED, 15 / 31, 8, strategy) + deflate() without deflateSetHeader (zlib_abi.hip
// put_header; deflate.rs:1572-1601, 2574-2700): zlib CMF 0x78, FLEVEL from level and strategy, FCHECK; gzip magic, CM 8, no flags,
// MTIME 0, XFL, OS 3.  Returns h.
static __device__ __forceinline__ uint32_t zmi_stream_header(uint32_t wrap, uint32_t level, uint32_t strategy, uint8_t* hb) {
    if (wrap == 1u) {
        const uint32_t lf = (strategy >= 2u || level < 2u) ? 0u : (level < 6u ? 1u : (level == 6u ? 2u : 3u));
        uint32_t h = (0x78u << 8) | (lf << 6);
        h += 31u - (h % 31u);
        hb[0] = (uint8_t)(h >> 8);
        hb[1] = (uint8_t)h;
        return 2u;
    }
    if (wrap == 2u) {
        const uint8_t g[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, (uint8_t)(level == 9u ? 2u : ((strategy >= 2u || level < 2u) ? 4u : 0u)), 3};
        for (int i = 0; i < 10; ++i) hb[i] = g[i];
        return 10u;
    }
    return 0u;
}

// Block 0, thread 0: header at out[0..h), trailer behind out[h + *payload] (Adler-32 big-endian / CRC-32 and ISIZE little-endian),
// *out_len = h + payload + trailer.  A stream that does not fit out_cap gets no trailer and status Z_BUF_ERROR (*out_len still
// tells the size it needs).  Every thread of the grid: index[i] += h (piece offsets relative to the payload -> offsets in out) and
// the first non-zero piece status lands in *status (which the caller zeroed).  The last index entry, the end of the deflate data,
// is written by thread 0 alone: it may be the payload word itself (zmi_deflate_stream_dev scans into the caller's index), and a
// workgroup that shifted it before thread 0 read it would move the trailer.
__global__ void __launch_bounds__(256) zmi_frame_kernel(uint8_t* __restrict__ out, uint64_t out_cap, uint32_t wrap, uint32_t level,
                                                        uint32_t strategy, const uint64_t* payload,
                                                        const uint32_t* __restrict__ check, const uint64_t* __restrict__ raw_len,
                                                        uint64_t* __restrict__ out_len, int32_t* status, const int32_t* __restrict__ piece_st,
                                                        uint32_t n_st, uint64_t* index, uint32_t n_index) {
    uint8_t hb[10];
    const uint32_t h = zmi_stream_header(wrap, level, strategy, hb);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = g0; i + 1u < n_index; i += stride) index[i] += h;
    if (status)
        for (uint64_t i = g0; i < n_st; i += stride)
            if (piece_st[i] != 0) atomicCAS(status, 0, piece_st[i]);
    if (g0 != 0) return;
    const uint64_t pl = *payload;
    if (n_index) index[n_index - 1u] = h + pl;
    const uint32_t tl = wrap == 1u ? 4u : (wrap == 2u ? 8u : 0u);
    const uint64_t total = h + pl + tl;
    *out_len = total;
    if (total > out_cap) {
        if (status) atomicCAS(status, 0, ZMI_BUF_ERROR);
        return;
    }
    for (uint32_t i = 0; i < h; ++i) out[i] = hb[i];
    uint8_t* tr = out + h + pl;
    const uint32_t c = check ? *check : 0u;
    if (wrap == 1u) {
        for (int i = 0; i < 4; ++i) tr[i] = (uint8_t)(c >> (24 - 8 * i));
    } else if (wrap == 2u) {
        const uint32_t isz = (uint32_t)*raw_len;
        for (int i = 0; i < 4; ++i) { tr[i] = (uint8_t)(c >> (8 * i)); tr[4 + i] = (uint8_t)(isz >> (8 * i)); }
    }
}
extern "C" uint32_t zmi_stream_header_len(int wrap) { return wrap == 1 ? 2u : (wrap == 2 ? 10u : 0u); }
extern "C" int zmi_launch_frame(uint8_t* d_out, uint64_t out_cap, uint32_t wrap, uint32_t level, uint32_t strategy, const uint64_t* d_payload,
                                const uint32_t* d_check, const uint64_t* d_raw_len, uint64_t* d_out_len, int32_t* d_status,
                                const int32_t* d_piece_st, uint32_t n_st, uint64_t* d_index, uint32_t n_index, hipStream_t stream) {
    const uint32_t work = n_st > n_index ? n_st : n_index;
    uint32_t blocks = (work + 255u) / 256u;
    if (blocks < 1u) blocks = 1u;
    if (blocks > 1024u) blocks = 1024u;
    ZMI_LAUNCH(zmi_frame_kernel, dim3(blocks), dim3(256), 0, stream, d_out, out_cap, wrap, level, strategy, d_payload, d_check, d_raw_len,
               d_out_len, d_status, d_piece_st, n_st, d_index, n_index);
    return 0;
}

// ---- proposals of gzip member starts (zmi_gzip_find_members_dev) -----------------------------------------------------------------
// A member announces itself: 1f 8b 08 and a FLG byte whose reserved bits are clear (RFC 1952; the reader of multi-member files,
// libz-rs-sys/src/gz.rs:1464-1506, looks for the same bytes behind every trailer).  Position p is an entry if p == 0, or if those
// four bytes stand at p and at least 18 bytes remain (10 of header, 8 of trailer).  One pass, 16-byte loads: the buffer is taken
// as 16-byte lines of the ADDRESS space (line 0 holds the first input byte at offset `head`), a lane owns the 16 start positions
// of its line and sees three bytes of the next line -- its neighbour's first dword, moved over by one DPP shift; lane 63 loads it.
// A hit belongs to the line its first byte lies in, so a pattern across a lane, wave or workgroup boundary is found exactly once.
// A workgroup takes MM_LINES lines per thread (16 KiB); pass 1 counts, the scan of pack.hip turns the counts into offsets, pass 2
// reads again only the segments that hold a hit (a real file: one segment in a few dozen) and writes every hit at its rank.
#define MM_T 256u
#define MM_LINES 4u
#define MM_SEG (MM_T * MM_LINES * 16u)

// the 16 bytes of line `li` (bytes outside the input read as zero)
static __device__ __forceinline__ zmi_b16 mm_line(const uint8_t* line0, uint64_t li, uint32_t head, uint64_t n) {
    const uint64_t q = li * 16u;               // offset of the line from line0; input byte p stands at q = p + head
    const uint64_t end = n + head;             // first offset behind the input
    zmi_b16 r;
    if (q >= head && q + 16u <= end) {
        const uint4 v = *(const uint4*)(line0 + q);
        r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w;
    } else {
        uint64_t lo = 0, hi = 0;
        for (uint32_t i = 0; i < 16u; ++i) {
            const uint64_t x = q + i;
            const uint64_t b = (x >= head && x < end) ? (uint64_t)line0[x] << (8u * (i & 7u)) : 0ull;
            if (i < 8u) lo |= b; else hi |= b;
        }
        r.w[0] = (uint32_t)lo; r.w[1] = (uint32_t)(lo >> 32); r.w[2] = (uint32_t)hi; r.w[3] = (uint32_t)(hi >> 32);
    }
    return r;
}

// bit i set: input position 16 * li - head + i is an entry
static __device__ __forceinline__ uint32_t mm_hits(const uint8_t* line0, uint64_t li, uint32_t head, uint64_t n) {
    const zmi_b16 c = mm_line(line0, li, head, n);
    uint32_t fill = 0;
    if (zmi_lane() == 63u) fill = mm_line(line0, li + 1u, head, n).w[0];
    const uint32_t nx = zmi_lane_down1(c.w[0], fill);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i) {
        const uint32_t lo = c.w[i >> 2], hi = (i >> 2) == 3u ? nx : c.w[(i >> 2) + 1u];
        const uint32_t v = (i & 3u) ? (lo >> (8u * (i & 3u))) | (hi << (32u - 8u * (i & 3u))) : lo;
        if ((v & 0xE0FFFFFFu) == 0x00088B1Fu) m |= 1u << i;
    }
    // positions in front of the input, position 0 (always an entry) and the last 17 positions
    const uint64_t q = li * 16u;
    if (q <= head || q + 33u > n + head) {   // (only the first line and the last three)
        for (uint32_t i = 0; i < 16u; ++i) {
            const uint64_t x = q + i;
            if (x < head || x - head + 18u > n) m &= ~(1u << i);
            if (x == head && n != 0u) m |= 1u << i;
        }
    }
    return m;
}

__global__ void __launch_bounds__(MM_T) zmi_mm_count_kernel(const uint8_t* __restrict__ line0, uint32_t head, uint64_t n,
                                                            uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wsum[MM_T / 64u];
    const uint32_t t = threadIdx.x;
    uint32_t c = 0;
    for (uint32_t r = 0; r < MM_LINES; ++r)
        c += (uint32_t)__popc(mm_hits(line0, ((uint64_t)blockIdx.x * MM_LINES + r) * MM_T + t, head, n));
    c = zmi_wave_sum(c);
    if (zmi_lane() == 0u) wsum[zmi_wave()] = c;
    __syncthreads();
    if (t == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void __launch_bounds__(MM_T) zmi_mm_gather_kernel(const uint8_t* __restrict__ line0, uint32_t head, uint64_t n,
                                                             const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ off, uint32_t nseg,
                                                             uint64_t* __restrict__ starts, uint32_t cap, uint32_t* __restrict__ n_starts) {
    __shared__ uint32_t wsum[MM_T / 64u];
    const uint32_t t = threadIdx.x;
    if (blockIdx.x == 0 && t == 0) { const uint64_t all = off[nseg]; *n_starts = all < cap ? (uint32_t)all : cap; }
    if (cnt[blockIdx.x] == 0u) return;   // (the whole workgroup)
    uint64_t at = off[blockIdx.x];
    for (uint32_t r = 0; r < MM_LINES; ++r) {
        const uint64_t li = ((uint64_t)blockIdx.x * MM_LINES + r) * MM_T + t;
        uint32_t m = mm_hits(line0, li, head, n);
        const uint32_t c = (uint32_t)__popc(m);
        const uint32_t incl = zmi_wave_incl_scan(c);
        __syncthreads();   // (wsum of the round before has been read)
        if (zmi_lane() == 63u) wsum[zmi_wave()] = incl;
        __syncthreads();
        uint32_t before = incl - c, total = 0;
        for (uint32_t w = 0; w < MM_T / 64u; ++w) { if (w < zmi_wave()) before += wsum[w]; total += wsum[w]; }
        uint64_t k = at + before;
        while (m) {
            const uint32_t i = (uint32_t)__ffs(m) - 1u;
            m &= m - 1u;
            if (k < cap) starts[k] = li * 16u + i - head;
            ++k;
        }
        at += total;
    }
}

extern "C" uint32_t zmi_mm_scan_segments(uint64_t in_len, uint32_t head) { return (uint32_t)((in_len + head + MM_SEG - 1u) / MM_SEG); }
// d_cnt u32[nseg], d_off u64[nseg + 1]; in_len > 0
extern "C" int zmi_launch_mm_find(const uint8_t* d_in, uint64_t in_len, uint32_t* d_cnt, uint64_t* d_off, uint64_t* d_starts, uint32_t cap,
                                  uint32_t* d_n_starts, hipStream_t stream) {
    const uint32_t head = (uint32_t)((uintptr_t)d_in & 15u);
    const uint8_t* line0 = d_in - head;
    const uint32_t nseg = zmi_mm_scan_segments(in_len, head);
    ZMI_LAUNCH(zmi_mm_count_kernel, dim3(nseg), dim3(MM_T), 0, stream, line0, head, in_len, d_cnt);
    ZMI_LAUNCH(zmi_scan_sizes_kernel, dim3(1), dim3(1024), 0, stream, (const uint32_t*)d_cnt, nseg, d_off, (const uint64_t*)nullptr);
    ZMI_LAUNCH(zmi_mm_gather_kernel, dim3(nseg), dim3(MM_T), 0, stream, line0, head, in_len, (const uint32_t*)d_cnt, (const uint64_t*)d_off, nseg,
               d_starts, cap, d_n_starts);
    return 0;
}

// ---- BGZF: blocked gzip (zmi_bgzf_blocks_dev, zmi_bgzf_deflate_dev) ---------------------------------------------------------------
// A block is a gzip member of 18 header bytes (FEXTRA with the one subfield BC, which holds BSIZE = the member's size - 1), a
// complete raw deflate stream and CRC-32 | ISIZE: the bytes htslib's bgzf.c writes.  The deflate stream is the encoder's slot, or,
// where that is longer than a stored block of the raw bytes (5 + len), that stored block -- so a member of len <= 65280 raw bytes
// is at most len + 31 bytes whatever the encoder did, and BSIZE fits its 16 bits.  The sizes kernel chooses, the scan above turns
// the sizes into offsets, the pack kernel writes every member in one pass: one read and one write of the compressed bytes.
#define BGZF_HEAD 18u
#define BGZF_TAIL 8u
#define BGZF_EOF 28u
#define BGZF_E_ARG (-103)   // ZMI_E_ARG (include/zmi355.h), in the call's status word

// header byte k < 16: 1f 8b 08 04 | MTIME 0 | XFL 0 | OS ff | XLEN 6 | 'B' 'C' 2 0
static __device__ __forceinline__ uint8_t bgzf_fixed(uint32_t k) {
    const uint64_t w = k < 8u ? 0x0000000004088B1Full : 0x000243420006FF00ull;
    return (uint8_t)(w >> (8u * (k & 7u)));
}

// the batch call's length table lives on the device: a shard above max_len becomes an empty one (the scratch is sized by max_len)
// and the call's status ZMI_E_ARG
__global__ void __launch_bounds__(256) zmi_bgzf_lens_kernel(const uint32_t* __restrict__ len, uint32_t n, uint32_t max_len,
                                                            uint32_t* __restrict__ clen, int32_t* status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = len[i];
    clen[i] = l > max_len ? 0u : l;
    if (l > max_len) atomicCAS(status, 0, BGZF_E_ARG);
}

// framed[i] = min(olen[i], len[i] + 5) + 26, stored[i] = the stored block was chosen (also behind an encoder status, which lands
// in *status: whatever the slot holds then is not read)
__global__ void __launch_bounds__(256) zmi_bgzf_sizes_kernel(const uint32_t* __restrict__ len, const uint32_t* __restrict__ olen,
                                                             const int32_t* __restrict__ st, uint32_t n, uint32_t* __restrict__ framed,
                                                             uint32_t* __restrict__ stored, int32_t* status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = len[i], e = olen[i];
    const int32_t s = st[i];
    const bool sb = s != 0 || e > l + 5u;
    framed[i] = (sb ? l + 5u : e) + BGZF_HEAD + BGZF_TAIL;
    stored[i] = sb ? 1u : 0u;
    if (s != 0) atomicCAS(status, 0, s);
}

// n * split jobs as in zmi_copy_ranges_kernel: job b copies tiles b % split, ... of block b / split's payload -- from its slot, or
// from the raw input behind the five bytes of a stored block -- and part 0 also writes the 18 + 8 (+ 5) bytes around it, one byte
// per thread.  A block that crosses out_cap is not written at all.
__global__ void __launch_bounds__(PK_T) zmi_bgzf_pack_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                             const uint32_t* __restrict__ len, const uint8_t* __restrict__ slots,
                                                             uint64_t slot_stride, const uint32_t* __restrict__ olen,
                                                             const uint32_t* __restrict__ stored, const uint32_t* __restrict__ crc,
                                                             uint8_t* __restrict__ out, const uint64_t* __restrict__ boff, uint64_t out_cap,
                                                             uint32_t split, uint32_t jobs) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[PK_TILE + 32];
    const uint32_t t = threadIdx.x;
  for (uint32_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const uint32_t r = job / split, part = job % split;
    const uint32_t l = len[r];
    const bool sb = stored[r] != 0u;
    const uint32_t pl = sb ? l + 5u : olen[r];
    const uint32_t total = BGZF_HEAD + pl + BGZF_TAIL;
    const uint64_t d0 = boff[r];
    if (d0 + total > out_cap) continue;   // does not fit: the call's status says so
    uint8_t* B = out + d0;
    if (part == 0u) {
        if (t < 16u) B[t] = bgzf_fixed(t);
        else if (t < BGZF_HEAD) B[t] = (uint8_t)((total - 1u) >> (8u * (t - 16u)));
        else if (t < BGZF_HEAD + BGZF_TAIL) {
            const uint32_t k = t - BGZF_HEAD;
            B[BGZF_HEAD + pl + k] = (uint8_t)((k < 4u ? crc[r] : l) >> (8u * (k & 3u)));
        } else if (sb && t < BGZF_HEAD + BGZF_TAIL + 5u) {
            const uint32_t k = t - (BGZF_HEAD + BGZF_TAIL);   // 01 | LEN | ~LEN
            B[BGZF_HEAD + k] = k == 0u ? (uint8_t)1u : (uint8_t)((k < 3u ? l : ~l) >> (8u * ((k - 1u) & 1u)));
        }
    }
    if (sb) pk_copy_tiles(stage, in + in_off[r], l, out, d0 + BGZF_HEAD + 5u, part, split, t);
    else pk_copy_tiles(stage, slots + (uint64_t)r * slot_stride, pl, out, d0 + BGZF_HEAD, part, split, t);
  }
}

// one thread: the total behind the last block (+ the end-of-file block), the status of a result that does not fit, and the
// end-of-file block itself: an empty member, 1f 8b 08 04 ... 42 43 02 00 | 1b 00 | 03 00 | CRC 0 | ISIZE 0
__global__ void zmi_bgzf_close_kernel(uint8_t* __restrict__ out, uint64_t out_cap, const uint64_t* __restrict__ blocks_end, uint32_t eof,
                                      uint64_t* __restrict__ out_len, int32_t* status) {
    const uint64_t at = *blocks_end;
    const uint64_t total = at + (eof ? BGZF_EOF : 0u);
    if (out_len) *out_len = total;
    if (total > out_cap) { atomicCAS(status, 0, ZMI_BUF_ERROR); return; }
    if (!eof) return;
    uint8_t* B = out + at;
    for (uint32_t k = 0; k < 16u; ++k) B[k] = bgzf_fixed(k);
    B[16] = (uint8_t)(BGZF_EOF - 1u);
    B[17] = 0;
    B[18] = 3;
    for (uint32_t k = 19u; k < BGZF_EOF; ++k) B[k] = 0;
}

extern "C" int zmi_launch_bgzf_lens(const uint32_t* d_len, uint32_t n, uint32_t max_len, uint32_t* d_clen, int32_t* d_status, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_bgzf_lens_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_len, n, max_len, d_clen, d_status);
    return 0;
}
extern "C" int zmi_launch_bgzf_sizes(const uint32_t* d_len, const uint32_t* d_olen, const int32_t* d_st, uint32_t n, uint32_t* d_framed,
                                     uint32_t* d_stored, int32_t* d_status, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_bgzf_sizes_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_len, d_olen, d_st, n, d_framed, d_stored, d_status);
    return 0;
}
extern "C" int zmi_launch_bgzf_pack(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_len, const uint8_t* d_slots,
                                    uint64_t slot_stride, const uint32_t* d_olen, const uint32_t* d_stored, const uint32_t* d_crc, uint32_t n,
                                    uint32_t max_len, uint8_t* d_out, const uint64_t* d_boff, uint64_t out_cap, hipStream_t stream) {
    if (n == 0) return 0;
    uint32_t split = 1;
    const uint32_t tiles = (max_len + 5u + PK_TILE - 1u) / PK_TILE;
    while ((uint64_t)n * split < 4096u && split < tiles) split <<= 1;
    ZMI_LAUNCH(zmi_bgzf_pack_kernel, dim3(n * split), dim3(PK_T), 0, stream, d_in, d_in_off, d_len, d_slots, slot_stride, d_olen, d_stored,
               d_crc, d_out, d_boff, out_cap, split, n * split);
    return 0;
}
extern "C" int zmi_launch_bgzf_close(uint8_t* d_out, uint64_t out_cap, const uint64_t* d_blocks_end, uint32_t eof, uint64_t* d_out_len,
                                     int32_t* d_status, hipStream_t stream) {
    ZMI_LAUNCH(zmi_bgzf_close_kernel, dim3(1), dim3(1), 0, stream, d_out, out_cap, d_blocks_end, eof, d_out_len, d_status);
    return 0;
}

// ---- ZIP archives (zmi_zip_directory_dev, zmi_zip_inflate_dev; the format rules: include/zmi355.h) ------------------
// A ZIP is a batch of raw-deflate (or stored) streams whose size table and CRC-32s stand in the central directory at the end of the
// file.  Three kernels read the directory -- locate (the end record, the ZIP64 record, the base), walk (the chain of directory entries:
// an entry's length stands inside it), parse (one thread per entry: the fixed fields, the ZIP64 extra, the local header) -- and two
// frame the batch decoder: prep (the tables of the selected slots) and verify (length, consumed input and CRC-32 against the table).
#define ZIP_T 256u
#define ZIP_TILE 16384u        // bytes of directory one window of the walk holds
#define ZIP_EOCD 22u
#define ZIP_TAIL 65557u        // 22 + the longest archive comment
#define ZIP_CEN 46u
#define ZIP_VERSION_ERROR (-6)
#define ZIP_E_ARG (-103)       // ZMI_E_ARG, in a slot's status word

static __device__ __forceinline__ uint32_t zip_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static __device__ __forceinline__ uint32_t zip_u32(const uint8_t* p) { return zip_u16(p) | (zip_u16(p + 2) << 16); }
static __device__ __forceinline__ uint64_t zip_u64(const uint8_t* p) { return (uint64_t)zip_u32(p) | ((uint64_t)zip_u32(p + 4) << 32); }

// w[0] the count the end structure names, w[1] != 0: that count is the 16-bit field (compared modulo 65536), w[2] / w[3] the first byte
// of the directory and the first byte behind it, as offsets in the input
#define ZIP_W_COUNT 0
#define ZIP_W_COUNT16 1
#define ZIP_W_DIR 2
#define ZIP_W_END 3

// One workgroup.  Every position p of the last <= 65557 bytes is tested for 50 4b 05 06 with the 16-byte lines of mm_line (a lane owns
// the 16 positions of its line and sees three bytes of the next one); a hit counts if its comment length ends the file exactly, the
// highest one wins (a maximum over 1 + p - lo, which fits 32 bits).  Thread 0 then parses the end record and, behind a locator, the
// ZIP64 record.
__global__ void __launch_bounds__(1024) zmi_zip_locate_kernel(const uint8_t* __restrict__ line0, uint32_t head, uint64_t n,
                                                               zmi_zip_info* __restrict__ info, uint64_t* __restrict__ w) {
    __shared__ uint32_t wbest[16];
    const uint32_t t = threadIdx.x;
    const uint8_t* in = line0 + head;
    const uint64_t lo = n > ZIP_TAIL ? n - ZIP_TAIL : 0ull;
    uint32_t best = 0;
    if (n >= ZIP_EOCD) {
        const uint64_t li0 = (lo + head) >> 4, li1 = (n - 1u + head) >> 4;
        for (uint64_t b = li0; b <= li1; b += 1024u) {   // (the same trip count in every lane: the lines talk through DPP)
            const uint64_t li = b + t;
            const zmi_b16 c = mm_line(line0, li, head, n);
            uint32_t fill = 0;
            if (zmi_lane() == 63u) fill = mm_line(line0, li + 1u, head, n).w[0];
            const uint32_t nx = zmi_lane_down1(c.w[0], fill);
#pragma unroll
            for (uint32_t i = 0; i < 16u; ++i) {
                const uint32_t l = c.w[i >> 2], h = (i >> 2) == 3u ? nx : c.w[(i >> 2) + 1u];
                const uint32_t v = (i & 3u) ? (l >> (8u * (i & 3u))) | (h << (32u - 8u * (i & 3u))) : l;
                if (v != 0x06054B50u) continue;
                const uint64_t q = li * 16u + i;             // (bytes in front of the input read as zero: q >= head here)
                const uint64_t p = q - head;
                if (p < lo || p + ZIP_EOCD > n) continue;
                if (p + ZIP_EOCD + zip_u16(in + p + 20u) == n) best = (uint32_t)(p - lo) + 1u;
            }
        }
    }
    best = zmi_wave_max(best);
    if (zmi_lane() == 0u) wbest[zmi_wave()] = best;
    __syncthreads();
    if (t != 0) return;
    for (uint32_t k = 1; k < 16u; ++k) best = wbest[k] > best ? wbest[k] : best;
    uint64_t cd_off = 0, cd_size = 0, base = 0, count = 0, count16 = 1, dir = 0, end = 0;
    int32_t st = 0, det = 0;
    if (best == 0u) { st = ZMI_DATA_ERROR; det = ZMI_ZA_NOEOCD; }
    else {
        const uint64_t p = lo + best - 1u;
        const uint8_t* e = in + p;
        uint32_t disks = zip_u16(e + 4) | zip_u16(e + 6);
        count = zip_u16(e + 10);
        cd_size = zip_u32(e + 12);
        cd_off = zip_u32(e + 16);
        end = p;
        if (p >= 20u && zip_u32(e - 20) == 0x07064B50u) {   // the locator: the 56-byte record stands in front of it
            if (p < 76u || zip_u32(e - 76) != 0x06064B50u || zip_u64(e - 72) != 44ull) { st = ZMI_DATA_ERROR; det = ZMI_ZA_ZIP64; }
            else {
                const uint8_t* r = e - 76;
                disks = zip_u32(r + 16) | zip_u32(r + 20) | zip_u32(e - 16) | (zip_u32(e - 4) > 1u ? 1u : 0u);
                if (zip_u16(e + 4) != 0xFFFFu) disks |= zip_u16(e + 4);
                if (zip_u16(e + 6) != 0xFFFFu) disks |= zip_u16(e + 6);
                count = zip_u64(r + 32);
                cd_size = zip_u64(r + 40);
                cd_off = zip_u64(r + 48);
                count16 = 0;
                end = p - 76u;
            }
        }
        if (st == 0 && disks != 0u) { st = ZIP_VERSION_ERROR; det = ZMI_ZA_MULTIDISK; }
        if (st == 0) {
            if (cd_size > end || cd_off > end - cd_size) { st = ZMI_DATA_ERROR; det = ZMI_ZA_BOUNDS; }
            else { base = end - cd_size - cd_off; dir = end - cd_size; }
        }
    }
    info->n_entries = 0;
    info->n_listed = 0;
    info->cd_off = cd_off;
    info->cd_size = cd_size;
    info->base = base;
    info->status = st;
    info->detail = det;
    w[ZIP_W_COUNT] = count;
    w[ZIP_W_COUNT16] = count16;
    w[ZIP_W_DIR] = dir;
    w[ZIP_W_END] = end;
}

// tile[mis + k] = in[p0 + k] for every k with mis + k < span, where span = min(want, mis + the bytes from p0 to `end`): aligned 16-byte
// loads from the line at or below in + p0, the first and last line byte-wise, so nothing outside [p0, end) is read.  Returns mis.
static __device__ __forceinline__ uint32_t zip_load_window(uint8_t* tile, const uint8_t* __restrict__ in, uint64_t p0, uint64_t end, uint32_t want,
                                                           uint32_t t, uint32_t* span_out) {
    const uint32_t mis = (uint32_t)((uintptr_t)(in + p0) & 15u);
    const uint8_t* line0 = in + p0 - mis;
    const uint64_t left = end - p0 + mis;
    const uint32_t span = left < want ? (uint32_t)left : want;
    for (uint32_t c = t * 16u; c < span; c += ZIP_T * 16u) {
        if (c + 16u <= span && (c >= 16u || mis == 0u)) {
            *(uint4*)(tile + c) = *(const uint4*)(line0 + c);
        } else {
            for (uint32_t j = 0; j < 16u; ++j)
                if (c + j >= mis && c + j < span) tile[c + j] = line0[c + j];
        }
    }
    *span_out = span;
    return mis;
}

// One step of the chain at `pos`, whose 46 header bytes stand at tile[o ..): the entry's length, or 0 where the chain breaks (wrong
// signature, or the entry would end behind the directory)
static __device__ __forceinline__ uint64_t zip_chain_step(const uint8_t* tile, uint32_t o, uint64_t pos, uint64_t end) {
    const uint32_t sig = zmi_load32u(tile, o), ne = zmi_load32u(tile, o + 28u), cl = zmi_load32u(tile, o + 32u) & 0xFFFFu;
    const uint64_t len = (uint64_t)ZIP_CEN + (ne & 0xFFFFu) + (ne >> 16) + cl;
    return (sig != 0x02014B50u || len > end - pos) ? 0ull : len;
}

// The chain is serial -- an entry's length stands inside it -- and one lane following it through LDS takes about 0.2 us an entry (measured:
// 19.6 ms of a 100 000-entry archive).  So the directory is cut into segments of ZIP_TILE bytes and every segment is followed on its own,
// one workgroup each, from a GUESS of where the chain enters it: the first position in the segment that holds 50 4b 01 02 (the chain's
// first entry in a segment holds it, so the guess is wrong only when a name, extra or comment in front of it spells the signature).
// seg[4k ..] = the guess q, the position x the segment's chase stopped at (the first chain position at or behind the segment's end, or
// where the chain broke or ended), the entries n in between, and a word the walk fills in.  The walk kernel below then only stitches: where
// the chain enters segment k at q exactly it takes (x, n) for the whole segment; where it does not, it follows the chain itself.
// pass 1, behind the walk: the segments the walk took write their positions at the rank the walk gave them (seg[4k + 3]).
// A header that starts in a segment may end up to 45 bytes behind it: the window holds 48 bytes more.
#define ZIP_SEG_NONE 0xFFFFFFFFFFFFFFFFull
__global__ void __launch_bounds__(ZIP_T) zmi_zip_segment_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ w, uint64_t* __restrict__ seg, uint64_t* __restrict__ chain,
                                                               uint32_t cap, uint32_t pass) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[ZIP_TILE + 96];
    __shared__ uint32_t s_q;
    const uint32_t t = threadIdx.x;
    const uint64_t dir = w[ZIP_W_DIR], end = w[ZIP_W_END];
    const uint64_t lo = dir + (uint64_t)blockIdx.x * ZIP_TILE;
    if (lo >= end) return;       // (the whole workgroup; an end record that gave no directory left dir = end = 0.  info->status is
                                 // not asked: behind the walk it may say CHAIN or COUNT, and the entries in front stay listed)
    uint64_t* sg = seg + 4ull * blockIdx.x;
    if (pass == 1u && sg[3] == ZIP_SEG_NONE) return;
    const uint64_t hi = end - lo < ZIP_TILE ? end : lo + ZIP_TILE;
    if (t == 0) s_q = 0xFFFFFFFFu;
    uint32_t span;
    const uint32_t mis = zip_load_window(tile, in, lo, end, ZIP_TILE + 64u, t, &span);
    __syncthreads();
    if (pass == 0u) {
        for (uint32_t i = t; i < (uint32_t)(hi - lo); i += ZIP_T)
            if (end - (lo + i) >= ZIP_CEN && zmi_load32u(tile, mis + i) == 0x02014B50u) { atomicMin(&s_q, i); break; }
        __syncthreads();
    }
    if (t != 0) return;
    uint64_t pos = pass == 0u ? (s_q == 0xFFFFFFFFu ? ZIP_SEG_NONE : lo + s_q) : sg[0];
    uint64_t n = 0, at = pass == 1u ? sg[3] : 0ull;
    const uint64_t q = pos;
    if (pos != ZIP_SEG_NONE) {
        while (pos < hi && end - pos >= ZIP_CEN) {
            const uint64_t len = zip_chain_step(tile, (uint32_t)(pos - lo) + mis, pos, end);
            if (len == 0ull) break;
            if (pass == 1u && at + n < cap) chain[at + n] = pos;
            ++n;
            pos += len;
        }
    }
    if (pass == 0u) { sg[0] = q; sg[1] = pos; sg[2] = n; sg[3] = ZIP_SEG_NONE; }
}

// One workgroup stitches.  Thread 0 keeps the chain's position: where it stands on a segment's guess it takes the segment whole and
// notes the rank of the segment's first entry; elsewhere the workgroup loads a window of ZIP_TILE bytes that starts at the 16-byte line
// of THAT position (aligned 16-byte loads, the first and last line byte-wise) and thread 0 follows the chain through it -- signature,
// the three lengths, 46 + name + extra + comment -- writing every entry's position, until the next header does not lie whole inside
// the window.  A window starts at the chain's position wherever it is: a header never straddles a window it is read from, and the
// tiles an entry of up to 46 + 3 x 65535 bytes spans are never loaded.
__global__ void __launch_bounds__(ZIP_T) zmi_zip_walk_kernel(const uint8_t* __restrict__ in, zmi_zip_info* info, const uint64_t* __restrict__ w,
                                                            uint64_t* __restrict__ seg, uint64_t nseg_max, uint64_t* __restrict__ chain, uint32_t cap) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[ZIP_TILE + 16];
    __shared__ uint64_t s_pos;
    __shared__ uint32_t s_state;   // 0 the chain goes on, 1 it ended on the directory's end, 2 it broke, 3 there is no directory
    const uint32_t t = threadIdx.x;
    const uint64_t dir = w[ZIP_W_DIR], end = w[ZIP_W_END];
    if (t == 0) { s_pos = dir; s_state = info->status != 0 ? 3u : 0u; }
    __syncthreads();
    if (s_state == 3u) return;   // (the whole workgroup: the end record gave no directory)
    uint64_t count = 0;
    for (;;) {
        if (t == 0) {
            uint64_t pos = s_pos;
            while (pos < end) {                              // whole segments, where the chain enters them at their guess
                const uint64_t k = (pos - dir) / ZIP_TILE;
                if (k >= nseg_max || seg[4u * k] != pos || seg[4u * k + 1u] == pos) break;
                seg[4u * k + 3u] = count;
                count += seg[4u * k + 2u];
                pos = seg[4u * k + 1u];
            }
            s_pos = pos;
            s_state = pos == end ? 1u : (end - pos < ZIP_CEN ? 2u : 0u);
        }
        __syncthreads();
        if (s_state != 0u) break;
        const uint64_t p0 = s_pos;
        uint32_t span;
        const uint32_t mis = zip_load_window(tile, in, p0, end, ZIP_TILE, t, &span);
        __syncthreads();
        if (t == 0) {
            uint64_t pos = p0;
            uint32_t state = 0;
            const uint64_t bound = dir + ((p0 - dir) / ZIP_TILE + 1u) * ZIP_TILE;   // the next segment may have guessed right again
            for (;;) {
                if (pos == end) { state = 1u; break; }
                if (end - pos < ZIP_CEN) { state = 2u; break; }
                if (pos >= bound) break;
                const uint64_t o64 = pos - p0 + mis;
                if (o64 + ZIP_CEN > span) break;             // the header is not whole in this window: the next one starts at it
                const uint64_t len = zip_chain_step(tile, (uint32_t)o64, pos, end);
                if (len == 0ull) { state = 2u; break; }
                if (count < cap) chain[count] = pos;
                ++count;
                pos += len;
            }
            s_pos = pos;
            s_state = state;
        }
        __syncthreads();
        if (s_state != 0u) break;
    }
    if (t != 0) return;
    info->n_entries = count;
    info->n_listed = count < cap ? count : cap;
    if (s_state == 2u) { info->status = ZMI_DATA_ERROR; info->detail = (int32_t)(ZMI_ZA_CHAIN | ((uint32_t)count << 8)); return; }
    const uint64_t want = w[ZIP_W_COUNT];
    if (w[ZIP_W_COUNT16] ? (count & 0xFFFFull) != want : count != want) { info->status = ZMI_DATA_ERROR; info->detail = ZMI_ZA_COUNT; }
}

// One thread per listed entry: the fixed fields of the directory entry, the values of its ZIP64 extra, its local header.
__global__ void __launch_bounds__(256) zmi_zip_parse_kernel(const uint8_t* __restrict__ in, zmi_zip_info* info, const uint64_t* __restrict__ w,
                                                            const uint64_t* __restrict__ chain, zmi_zip_entry* __restrict__ ent, uint32_t cap) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cap || (uint64_t)i >= info->n_listed) return;
    const uint64_t dir = w[ZIP_W_DIR], base = info->base, at = chain[i];
    const uint8_t* h = in + at;
    const uint32_t flags = zip_u16(h + 8), method = zip_u16(h + 10), nl = zip_u16(h + 28), el = zip_u16(h + 30);
    uint64_t csize = zip_u32(h + 20), usize = zip_u32(h + 24), lho = zip_u32(h + 42);
    int32_t st = 0;
    if (zip_u16(h + 34) != 0u && atomicCAS(&info->status, 0, ZIP_VERSION_ERROR) == 0) info->detail = ZMI_ZA_MULTIDISK;
    if (csize == 0xFFFFFFFFull || usize == 0xFFFFFFFFull || lho == 0xFFFFFFFFull) {
        // the ZIP64 extra: 8-byte values for exactly those of usize, csize, offset (in that order) whose field is all ones
        const uint8_t* x = h + ZIP_CEN + nl;
        st = ZMI_ZE_EXTRA;
        for (uint32_t a = 0; a + 4u <= el;) {
            const uint32_t id = zip_u16(x + a), sz = zip_u16(x + a + 2u);
            if (a + 4u + sz > el) break;
            if (id == 1u) {
                const uint32_t need = 8u * ((usize == 0xFFFFFFFFull) + (csize == 0xFFFFFFFFull) + (lho == 0xFFFFFFFFull));
                if (sz >= need) {
                    const uint8_t* q = x + a + 4u;
                    if (usize == 0xFFFFFFFFull) { usize = zip_u64(q); q += 8; }
                    if (csize == 0xFFFFFFFFull) { csize = zip_u64(q); q += 8; }
                    if (lho == 0xFFFFFFFFull) lho = zip_u64(q);
                    st = 0;
                }
                break;
            }
            a += 4u + sz;
        }
    }
    const bool big = st == 0 && (csize > 0xFFFFFFFFull || usize > 0xFFFFFFFFull);
    uint64_t data_off = 0;
    bool local_ok = false;
    if (st == 0 && lho <= dir - base && base + lho + 30u <= dir) {
        const uint8_t* l = in + base + lho;
        if (zip_u32(l) == 0x04034B50u && zip_u16(l + 8) == method) {
            data_off = base + lho + 30u + zip_u16(l + 26) + zip_u16(l + 28);   // the LOCAL name and extra lengths
            local_ok = data_off <= dir && csize <= dir - data_off;
        }
    }
    if (st == 0) {
        if (big) st = ZMI_ZE_BIG;
        else if (!local_ok) st = ZMI_ZE_LOCAL;
        else if (flags & 0x41u) st = ZMI_ZE_CRYPT;
        else if (method != 0u && method != 8u) st = ZMI_ZE_METHOD;
        else if (method == 0u && csize != usize) st = ZMI_ZE_STORED;
    }
    zmi_zip_entry e;
    e.data_off = data_off;
    e.name_off = at + ZIP_CEN;
    e.csize = csize > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)csize;
    e.usize = usize > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)usize;
    e.crc32 = zip_u32(h + 16);
    e.dos_time = (zip_u16(h + 14) << 16) | zip_u16(h + 12);
    e.ext_attr = zip_u32(h + 38);
    e.method = (uint16_t)method;
    e.flags = (uint16_t)flags;
    e.name_len = (uint16_t)nl;
    e.reserved = 0;
    e.status = st;
    ent[i] = e;
}

// What slot j reads: 0 a deflated entry, 1 a stored one, 2 an entry the directory flagged, 3 nothing the table allows (an index that
// is not in it, or data that leaves the input: the table was not made from this buffer)
static __device__ __forceinline__ uint32_t zip_slot_kind(const zmi_zip_entry* __restrict__ ent, uint32_t n_entries, const uint32_t* __restrict__ sel,
                                                         uint32_t j, uint64_t in_len, zmi_zip_entry* e) {
    const uint32_t k = sel ? sel[j] : j;
    if (k >= n_entries) return 3u;
    *e = ent[k];
    if (e->status != 0) return 2u;
    if (e->data_off > in_len || e->csize > in_len - e->data_off) return 3u;
    if (e->method == 8u) return 0u;
    return e->method == 0u && e->csize == e->usize ? 1u : 3u;
}

// the tables of the selection: what the plan, the batch decoder (deflated slots; the others hand it no input) and the range copy
// (stored slots) take
__global__ void __launch_bounds__(256) zmi_zip_prep_kernel(const zmi_zip_entry* __restrict__ ent, uint32_t n_entries, const uint32_t* __restrict__ sel,
                                                           uint32_t n_sel, uint64_t in_len, uint64_t* __restrict__ in_off,
                                                           uint32_t* __restrict__ in_n, uint32_t* __restrict__ size, uint32_t* __restrict__ slen) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    zmi_zip_entry e;
    const uint32_t kind = zip_slot_kind(ent, n_entries, sel, j, in_len, &e);
    in_off[j] = kind <= 1u ? e.data_off : 0ull;
    in_n[j] = kind == 0u ? e.csize : 0u;
    size[j] = kind <= 1u ? e.usize : 0u;
    slen[j] = kind == 1u ? e.usize : 0u;
}

// One thread per slot, behind the decode, the stored copies and the CRC-32 of every region (cap[j] bytes: the planned size where the
// region fits out_cap, else 0): the slot's final words.  Every status but 0 reports length 0.
__global__ void __launch_bounds__(256) zmi_zip_verify_kernel(const zmi_zip_entry* __restrict__ ent, uint32_t n_entries, const uint32_t* __restrict__ sel,
                                                             uint32_t n_sel, uint64_t in_len, const uint64_t* __restrict__ out_off, uint64_t out_cap,
                                                             const uint32_t* __restrict__ used, const uint32_t* __restrict__ crc,
                                                             uint32_t* __restrict__ out_len, int32_t* __restrict__ status, int32_t* __restrict__ detail) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    zmi_zip_entry e;
    const uint32_t kind = zip_slot_kind(ent, n_entries, sel, j, in_len, &e);
    int32_t st = 0, det = 0;
    if (kind == 3u) st = ZIP_E_ARG;
    else if (kind == 2u) { st = ZIP_VERSION_ERROR; det = e.status; }
    else if (out_off[j] + (uint64_t)e.usize > out_cap) { st = ZMI_BUF_ERROR; det = ZMI_ZE_OUT; }
    else {
        if (kind == 0u) {
            const int32_t ds = status[j];
            if (ds == ZMI_OK) { if (out_len[j] != e.usize || used[j] != e.csize) { st = ZMI_DATA_ERROR; det = ZMI_ZE_LENGTH; } }
            else if (ds == ZMI_BUF_ERROR) { st = ZMI_DATA_ERROR; det = ZMI_ZE_LENGTH; }   // the stream wants more input than csize, or more room than usize
            else if (ds == ZMI_DATA_ERROR) { st = ZMI_DATA_ERROR; det = ZMI_ZE_DATA; }
            else st = ds;
        }
        if (st == 0 && crc[j] != e.crc32) { st = ZMI_DATA_ERROR; det = ZMI_ZE_CHECK; }
    }
    status[j] = st;
    detail[j] = det;
    out_len[j] = st == 0 ? e.usize : 0u;
}

extern "C" uint32_t zmi_zip_walk_tile(void) { return ZIP_TILE; }
// segments a directory inside in_len bytes can have (its size is a device word: the launch covers the bound, the others return)
extern "C" uint64_t zmi_zip_segments(uint64_t in_len) { return in_len / ZIP_TILE + 1u; }
// d_w: four words, d_chain: u64[cap], d_seg: four words per segment of zmi_zip_segments(in_len).  stages 1: locate, 2: and the chain
// (segments, walk, segments' positions), 3: and the parse (the probe's split of the directory time)
extern "C" int zmi_launch_zip_directory(const uint8_t* d_in, uint64_t in_len, zmi_zip_entry* d_entries, uint32_t cap, zmi_zip_info* d_info,
                                        uint64_t* d_w, uint64_t* d_chain, uint64_t* d_seg, uint32_t stages, hipStream_t stream) {
    const uint32_t head = (uint32_t)((uintptr_t)d_in & 15u);
    ZMI_LAUNCH(zmi_zip_locate_kernel, dim3(1), dim3(1024), 0, stream, d_in - head, head, in_len, d_info, d_w);
    if (stages < 2u) return 0;
    const uint64_t nseg = zmi_zip_segments(in_len);
    const uint32_t grid = nseg > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)nseg;
    ZMI_LAUNCH(zmi_zip_segment_kernel, dim3(grid), dim3(ZIP_T), 0, stream, d_in, (const uint64_t*)d_w, d_seg, d_chain, cap, 0u);
    ZMI_LAUNCH(zmi_zip_walk_kernel, dim3(1), dim3(ZIP_T), 0, stream, d_in, d_info, (const uint64_t*)d_w, d_seg, (uint64_t)grid, d_chain, cap);
    if (cap == 0u) return 0;
    ZMI_LAUNCH(zmi_zip_segment_kernel, dim3(grid), dim3(ZIP_T), 0, stream, d_in, (const uint64_t*)d_w, d_seg, d_chain, cap, 1u);
    if (stages < 3u) return 0;
    ZMI_LAUNCH(zmi_zip_parse_kernel, dim3((cap + 255u) / 256u), dim3(256), 0, stream, d_in, d_info, (const uint64_t*)d_w, (const uint64_t*)d_chain,
               d_entries, cap);
    return 0;
}
extern "C" int zmi_launch_zip_prep(const zmi_zip_entry* d_entries, uint32_t n_entries, const uint32_t* d_sel, uint32_t n_sel, uint64_t in_len,
                                   uint64_t* d_in_off, uint32_t* d_in_n, uint32_t* d_size, uint32_t* d_slen, hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_zip_prep_kernel, dim3((n_sel + 255u) / 256u), dim3(256), 0, stream, d_entries, n_entries, d_sel, n_sel, in_len, d_in_off, d_in_n,
               d_size, d_slen);
    return 0;
}
extern "C" int zmi_launch_zip_verify(const zmi_zip_entry* d_entries, uint32_t n_entries, const uint32_t* d_sel, uint32_t n_sel, uint64_t in_len,
                                     const uint64_t* d_out_off, uint64_t out_cap, const uint32_t* d_used, const uint32_t* d_crc,
                                     uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_zip_verify_kernel, dim3((n_sel + 255u) / 256u), dim3(256), 0, stream, d_entries, n_entries, d_sel, n_sel, in_len, d_out_off,
               out_cap, d_used, d_crc, d_out_len, d_status, d_detail);
    return 0;
}

// ---- writing ZIP archives (zmi_zip_write_dev; every byte of the format: include/zmi355.h) ----------------------------
// An entry is cut into pieces of piece_bytes, the pieces of all entries form ONE table the independent-piece encoder works through in
// launch groups (a piece that is its entry's last ends a stream: the bitmap of chain mode 2, encode.hip); a piece's place in the
// archive is its compressed size, plus the hole of 30 + name bytes in front of an entry's first piece.  layout / pieces make the table,
// sizes / pack place and copy one group behind the device word the group before ended at, headers fills the holes and writes the
// directory once every offset is known, close writes the end structure.
#define ZW_E_ARG (-103)        // ZMI_E_ARG, in the call's status word
#define ZW_VOID 0xFFFFFFFFu    // head[] of a piece behind the true piece count
#define ZW_G 16u               // threads that share an entry in the headers kernel
#define ZW_LOC 30u

// per entry: the checked length (above ZMI_ZIP_ENTRY_MAX: empty, ZMI_E_ARG), the checked name length (cut at 65 535, ZMI_E_ARG) and
// the piece count max(1, ceil(len / piece_bytes)).  *sum (zeroed by the caller) receives the sum of the checked lengths, one atomic per
// wave, for the in_bytes check of the pieces kernel.
__global__ void __launch_bounds__(256) zmi_zip_layout_kernel(const uint32_t* __restrict__ in_len, const uint64_t* __restrict__ name_off, uint32_t n,
                                                             uint32_t piece_bytes, uint32_t* __restrict__ elen, uint32_t* __restrict__ nlen,
                                                             uint32_t* __restrict__ npc, unsigned long long* sum, int32_t* status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t l = 0u;                                     // (no early return: the wave's lanes meet in the shuffles below)
    if (i < n) {
        l = in_len[i];
        uint64_t nl = name_off[i + 1u] - name_off[i];
        if (l > ZMI_ZIP_ENTRY_MAX) { l = 0u; atomicCAS(status, 0, ZW_E_ARG); }
        if (nl > 65535ull) { nl = 65535ull; atomicCAS(status, 0, ZW_E_ARG); }
        elen[i] = l;
        nlen[i] = (uint32_t)nl;
        npc[i] = l ? (uint32_t)(((uint64_t)l + piece_bytes - 1u) / piece_bytes) : 1u;
    }
    unsigned long long w = l;
    for (uint32_t d = 1u; d < 64u; d <<= 1) w += __shfl_xor(w, (int)d);
    if ((threadIdx.x & 63u) == 0u && w) atomicAdd(sum, w);
}

// per piece of the table's `cap` places: first[] (the scan of the piece counts, n + 1 entries) names its entry, by bisection; piece k of
// an entry is [k * piece_bytes, + min(piece_bytes, len - k * piece_bytes)) of it.  head[i] = 30 + name bytes where it is its entry's
// first, 0 elsewhere, ZW_VOID behind the true count first[n].  The bit of an entry's last piece is set in `ends` (zeroed by the caller),
// which holds `wpg` words for every launch group of `group` pieces, so that every group's bits start at a word.  *sum > in_bytes -- the
// caller's bound on the lengths does not hold, the table may not have room for the pieces -- makes every piece void and the archive
// an empty one: *n_eff = 0, else n.
__global__ void __launch_bounds__(256) zmi_zip_pieces_kernel(const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ elen,
                                                             const uint32_t* __restrict__ nlen, const uint64_t* __restrict__ first,
                                                             const unsigned long long* __restrict__ sum, uint32_t n, uint64_t in_bytes,
                                                             uint32_t piece_bytes, uint32_t cap, uint32_t group, uint32_t wpg,
                                                             uint64_t* __restrict__ p_off, uint32_t* __restrict__ p_len,
                                                             uint32_t* __restrict__ head, uint32_t* ends, uint32_t* __restrict__ n_eff,
                                                             int32_t* status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool bad = *sum > in_bytes;
    if (i == 0u) {
        *n_eff = bad ? 0u : n;
        if (bad) atomicCAS(status, 0, ZW_E_ARG);
    }
    if (i >= cap) return;
    if (bad || (uint64_t)i >= first[n]) { p_off[i] = 0ull; p_len[i] = 0u; head[i] = ZW_VOID; return; }
    uint32_t lo = 0u, hi = n;                   // first[lo] <= i < first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= (uint64_t)i) lo = mid; else hi = mid;
    }
    const uint32_t k = i - (uint32_t)first[lo], l = elen[lo];
    const uint64_t o = (uint64_t)k * piece_bytes;
    p_off[i] = in_off[lo] + o;
    p_len[i] = l - o < piece_bytes ? (uint32_t)(l - o) : piece_bytes;
    head[i] = k == 0u ? ZW_LOC + nlen[lo] : 0u;
    if ((uint64_t)i + 1u == first[lo + 1u]) {
        const uint32_t j = i % group;
        atomicOr(&ends[(uint64_t)(i / group) * wpg + (j >> 5)], 1u << (j & 31u));
    }
}

// size[i] = the piece's place in the archive: its payload (the encoder's olen; at level 0 the caller passes the raw lengths and no
// statuses) plus the hole in front of an entry's first piece; 0 for a void piece.  The first encoder status lands in *status.
__global__ void __launch_bounds__(256) zmi_zip_sizes_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ olen,
                                                            const int32_t* __restrict__ st, uint32_t n, uint32_t* __restrict__ size, int32_t* status) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = head[i];
    if (h == ZW_VOID) { size[i] = 0u; return; }
    size[i] = h + olen[i];
    if (st && st[i] != 0) atomicCAS(status, 0, st[i]);
}

// n * split jobs as in zmi_copy_ranges_kernel: the payload of piece b / split goes behind its hole, from its slot or (slots NULL:
// level 0) from the raw input.  The holes are left alone; a payload that crosses out_cap is not written at all.
__global__ void __launch_bounds__(PK_T) zmi_zip_pack_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ p_off,
                                                            const uint32_t* __restrict__ head, const uint8_t* __restrict__ slots,
                                                            uint64_t slot_stride, const uint32_t* __restrict__ olen, uint8_t* __restrict__ out,
                                                            const uint64_t* __restrict__ pos, uint64_t out_cap, uint32_t split, uint32_t jobs) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[PK_TILE + 32];
    const uint32_t t = threadIdx.x;
  for (uint32_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const uint32_t r = job / split, part = job % split;
    const uint32_t h = head[r];
    if (h == ZW_VOID) continue;
    const uint32_t l = olen[r];
    const uint64_t d0 = pos[r] + h;
    if (d0 + l > out_cap) continue;   // does not fit: the call's status says so
    pk_copy_tiles(stage, slots ? slots + (uint64_t)r * slot_stride : in + p_off[r], l, out, d0, part, split, t);
  }
}

// what the local header and the central record of entry e say
struct zw_entry {
    uint64_t lho, data_off, abs_off;   // the local header and the first payload byte in d_out; base + lho
    uint32_t nl, csize, usize, crc, dos, ext;
    bool sat;                          // abs_off does not fit the 32-bit field: the ZIP64 extra carries it
    bool big;                          // the compressed size does not fit its 32-bit field (csize is then all ones): ZMI_E_ARG
};
static __device__ __forceinline__ zw_entry zw_entry_of(uint32_t e, const uint32_t* __restrict__ elen, const uint32_t* __restrict__ nlen,
                                                       const uint64_t* __restrict__ first, const uint64_t* __restrict__ pos,
                                                       const uint32_t* __restrict__ crc, const uint32_t* __restrict__ dos_time,
                                                       const uint32_t* __restrict__ ext_attr, uint64_t base) {
    zw_entry z;
    z.nl = nlen[e];
    z.lho = pos[first[e]];
    z.data_off = z.lho + ZW_LOC + z.nl;
    const uint64_t cs = pos[first[e + 1u]] - z.data_off;
    z.big = cs >= 0xFFFFFFFFull;       // (only pieces of a few bytes get there: every piece adds its flush marker and block header)
    z.csize = z.big ? 0xFFFFFFFFu : (uint32_t)cs;
    z.usize = elen[e];
    z.crc = crc[e];
    z.dos = dos_time ? dos_time[e] : 0x00210000u;
    z.ext = ext_attr ? ext_attr[e] : 0x81A40000u;
    z.abs_off = base + z.lho;
    z.sat = z.abs_off >= 0xFFFFFFFFull;
    return z;
}
// byte k of a record given as little-endian 64-bit words
static __device__ __forceinline__ uint8_t zw_byte(const uint64_t* w, uint32_t k) { return (uint8_t)(w[k >> 3] >> (8u * (k & 7u))); }

// ZW_G threads per entry, behind the last group.  pass 0: the local header and the name into the entry's hole, and the size of its
// central record (46 + name + the 12 bytes of the ZIP64 extra where base + offset needs them; 0 for the entries of a call whose
// in_bytes check failed) for the scan that places the directory.  pass 1: the central record at cen_off[e] and the row of d_entries.
// An entry whose compressed size does not fit 32 bits puts ZMI_E_ARG into *status (pass 0), its size fields are all ones.
// Either copies the name from the caller's blob -- the threads of the entry take its bytes in turn and learn on the way whether one
// is >= 0x80 (general-purpose bit 11) -- and writes the fixed bytes one per thread and round.  A record that crosses out_cap is not
// written.
__global__ void __launch_bounds__(256) zmi_zip_headers_kernel(const uint32_t* __restrict__ elen, const uint32_t* __restrict__ nlen,
                                                              const uint64_t* __restrict__ first, const uint64_t* __restrict__ pos,
                                                              const uint32_t* __restrict__ crc, const uint8_t* __restrict__ names,
                                                              const uint64_t* __restrict__ name_off, const uint32_t* __restrict__ dos_time,
                                                              const uint32_t* __restrict__ ext_attr, uint32_t n, const uint32_t* __restrict__ n_eff,
                                                              uint32_t method, uint64_t base, uint8_t* __restrict__ out, uint64_t out_cap,
                                                              uint32_t* __restrict__ cen_size, const uint64_t* __restrict__ cen_off,
                                                              zmi_zip_entry* __restrict__ ent, uint32_t pass, int32_t* status) {
    const uint64_t gi = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = (uint32_t)(gi % ZW_G);
    const bool live = gi / ZW_G < (uint64_t)n;           // (no early return: the group's threads meet in the shuffles below)
    const uint32_t e = live ? (uint32_t)(gi / ZW_G) : 0u;
    const bool listed = live && e < *n_eff;
    if (live && !listed && pass == 0u && g == 0u) cen_size[e] = 0u;
    zw_entry z = {};
    if (listed) z = zw_entry_of(e, elen, nlen, first, pos, crc, dos_time, ext_attr, base);
    const uint32_t cen = ZIP_CEN + z.nl + (z.sat ? 12u : 0u);
    const uint64_t at = pass == 0u ? z.lho : (listed ? cen_off[e] : 0ull);
    const bool fits = listed && at + (pass == 0u ? ZW_LOC + z.nl : cen) <= out_cap;
    const uint8_t* nm = names + (listed ? name_off[e] : 0ull);
    uint8_t* nd = out + at + (pass == 0u ? ZW_LOC : ZIP_CEN);
    uint32_t hi = 0u;
    if (listed)
        for (uint32_t k = g; k < z.nl; k += ZW_G) {
            const uint8_t b = nm[k];
            hi |= b;
            if (fits) nd[k] = b;
        }
    for (uint32_t d = 1u; d < ZW_G; d <<= 1) hi |= __shfl_xor(hi, (int)d);
    if (!listed) return;
    const uint64_t flags = hi & 0x80u ? 0x0800u : 0u;
    const uint64_t need = z.sat && pass == 1u ? 45u : (method ? 20u : 10u);
    const uint64_t time = z.dos & 0xFFFFu, date = z.dos >> 16;
    if (pass == 0u) {
        if (g == 0u) cen_size[e] = cen;
        if (g == 0u && z.big) atomicCAS(status, 0, ZW_E_ARG);
        if (!fits) return;
        const uint64_t w[4] = {0x04034B50ull | need << 32 | flags << 48,
                               (uint64_t)method | time << 16 | date << 32 | (uint64_t)(z.crc & 0xFFFFu) << 48,
                               (uint64_t)(z.crc >> 16) | (uint64_t)z.csize << 16 | (uint64_t)(z.usize & 0xFFFFu) << 48,
                               (uint64_t)(z.usize >> 16) | (uint64_t)z.nl << 16};
        for (uint32_t k = g; k < ZW_LOC; k += ZW_G) out[at + k] = zw_byte(w, k);
        return;
    }
    if (g == 0u && ent) {
        zmi_zip_entry r;
        r.data_off = z.data_off;
        r.name_off = at + ZIP_CEN;
        r.csize = z.csize;
        r.usize = z.usize;
        r.crc32 = z.crc;
        r.dos_time = z.dos;
        r.ext_attr = z.ext;
        r.method = (uint16_t)method;
        r.flags = (uint16_t)flags;
        r.name_len = (uint16_t)z.nl;
        r.reserved = 0;
        r.status = 0;
        ent[e] = r;
    }
    if (!fits) return;
    const uint64_t off32 = z.sat ? 0xFFFFFFFFull : z.abs_off;
    const uint64_t w[6] = {0x02014B50ull | (0x0300ull | need) << 32 | need << 48,
                           flags | (uint64_t)method << 16 | time << 32 | date << 48,
                           (uint64_t)z.crc | (uint64_t)z.csize << 32,
                           (uint64_t)z.usize | (uint64_t)z.nl << 32 | (z.sat ? 12ull : 0ull) << 48,
                           (uint64_t)(z.ext & 0xFFFFu) << 48,
                           (uint64_t)(z.ext >> 16) | off32 << 16};
    for (uint32_t k = g; k < ZIP_CEN; k += ZW_G) out[at + k] = zw_byte(w, k);
    if (z.sat && g < 12u) {
        const uint64_t x[2] = {0x00080001ull | z.abs_off << 32, z.abs_off >> 32};
        out[at + ZIP_CEN + z.nl + g] = zw_byte(x, g);
    }
}

// One thread: the end structure behind the directory [*pay_end, *cd_end) -- the ZIP64 record and its locator where the count, the
// directory's size or its absolute offset saturates a field, then the end record, each written where it ends at or before out_cap --,
// *out_len, d_info, and Z_BUF_ERROR for an archive that does not fit.
__global__ void zmi_zip_close_kernel(uint8_t* __restrict__ out, uint64_t out_cap, const uint64_t* __restrict__ pay_end,
                                     const uint64_t* __restrict__ cd_end, const uint32_t* __restrict__ n_eff, uint64_t base,
                                     uint64_t* __restrict__ out_len, zmi_zip_info* __restrict__ info, int32_t* status) {
    const uint64_t dir = *pay_end, end = *cd_end, n = *n_eff;
    const uint64_t cd_size = end - dir, cd_off = base + dir;
    const bool z64 = n >= 0xFFFFull || cd_size >= 0xFFFFFFFFull || cd_off >= 0xFFFFFFFFull;
    uint64_t at = end;
    if (z64) {
        const uint64_t r[7] = {0x06064B50ull | 44ull << 32, 0x032Dull << 32 | 45ull << 48, 0ull, n, n, cd_size, cd_off};
        if (at + 56u <= out_cap) for (uint32_t k = 0; k < 56u; ++k) out[at + k] = zw_byte(r, k);
        const uint64_t rec = base + at;
        at += 56u;
        const uint64_t l[3] = {0x07064B50ull, rec, 1ull};
        if (at + 20u <= out_cap) for (uint32_t k = 0; k < 20u; ++k) out[at + k] = zw_byte(l, k);
        at += 20u;
    }
    const uint64_t n16 = n < 0xFFFFull ? n : 0xFFFFull;
    const uint64_t s32 = cd_size < 0xFFFFFFFFull ? cd_size : 0xFFFFFFFFull, o32 = cd_off < 0xFFFFFFFFull ? cd_off : 0xFFFFFFFFull;
    const uint64_t w[3] = {0x06054B50ull, n16 | n16 << 16 | s32 << 32, o32};
    if (at + ZIP_EOCD <= out_cap) for (uint32_t k = 0; k < ZIP_EOCD; ++k) out[at + k] = zw_byte(w, k);
    at += ZIP_EOCD;
    *out_len = at;
    if (at > out_cap) atomicCAS(status, 0, ZMI_BUF_ERROR);
    if (info) {
        info->n_entries = n;
        info->n_listed = n;
        info->cd_off = dir;
        info->cd_size = cd_size;
        info->base = 0;
        info->status = 0;
        info->detail = 0;
    }
}

extern "C" int zmi_launch_zip_layout(const uint32_t* d_in_len, const uint64_t* d_name_off, uint32_t n, uint32_t piece_bytes, uint32_t* d_elen,
                                     uint32_t* d_nlen, uint32_t* d_npc, uint64_t* d_sum, int32_t* d_status, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_zip_layout_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_in_len, d_name_off, n, piece_bytes, d_elen, d_nlen, d_npc,
               (unsigned long long*)d_sum, d_status);
    return 0;
}
extern "C" int zmi_launch_zip_pieces(const uint64_t* d_in_off, const uint32_t* d_elen, const uint32_t* d_nlen, const uint64_t* d_first,
                                     const uint64_t* d_sum, uint32_t n, uint64_t in_bytes, uint32_t piece_bytes, uint32_t cap, uint32_t group,
                                     uint32_t wpg, uint64_t* d_p_off, uint32_t* d_p_len, uint32_t* d_head, uint32_t* d_ends, uint32_t* d_n_eff,
                                     int32_t* d_status, hipStream_t stream) {
    if (n == 0 || cap == 0) return 0;
    ZMI_LAUNCH(zmi_zip_pieces_kernel, dim3((cap + 255u) / 256u), dim3(256), 0, stream, d_in_off, d_elen, d_nlen, d_first,
               (const unsigned long long*)d_sum, n, in_bytes,
               piece_bytes, cap, group, wpg, d_p_off, d_p_len, d_head, d_ends, d_n_eff, d_status);
    return 0;
}
extern "C" int zmi_launch_zip_sizes(const uint32_t* d_head, const uint32_t* d_olen, const int32_t* d_st, uint32_t n, uint32_t* d_size,
                                    int32_t* d_status, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_zip_sizes_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_head, d_olen, d_st, n, d_size, d_status);
    return 0;
}
extern "C" int zmi_launch_zip_pack(const uint8_t* d_in, const uint64_t* d_p_off, const uint32_t* d_head, const uint8_t* d_slots,
                                   uint64_t slot_stride, const uint32_t* d_olen, uint32_t n, uint32_t max_len, uint8_t* d_out,
                                   const uint64_t* d_pos, uint64_t out_cap, hipStream_t stream) {
    if (n == 0) return 0;
    uint32_t split = 1;
    const uint32_t tiles = (max_len + PK_TILE - 1u) / PK_TILE;
    while ((uint64_t)n * split < 4096u && split < tiles) split <<= 1;
    ZMI_LAUNCH(zmi_zip_pack_kernel, dim3(n * split), dim3(PK_T), 0, stream, d_in, d_p_off, d_head, d_slots, slot_stride, d_olen, d_out, d_pos,
               out_cap, split, n * split);
    return 0;
}
extern "C" int zmi_launch_zip_headers(const uint32_t* d_elen, const uint32_t* d_nlen, const uint64_t* d_first, const uint64_t* d_pos,
                                      const uint32_t* d_crc, const uint8_t* d_names, const uint64_t* d_name_off, const uint32_t* d_dos_time,
                                      const uint32_t* d_ext_attr, uint32_t n, const uint32_t* d_n_eff, uint32_t method, uint64_t base,
                                      uint8_t* d_out, uint64_t out_cap, uint32_t* d_cen_size, const uint64_t* d_cen_off, zmi_zip_entry* d_entries,
                                      uint32_t pass, int32_t* d_status, hipStream_t stream) {
    if (n == 0) return 0;
    const uint32_t per = 256u / ZW_G;
    ZMI_LAUNCH(zmi_zip_headers_kernel, dim3((n + per - 1u) / per), dim3(256), 0, stream, d_elen, d_nlen, d_first, d_pos, d_crc, d_names, d_name_off,
               d_dos_time, d_ext_attr, n, d_n_eff, method, base, d_out, out_cap, d_cen_size, d_cen_off, d_entries, pass, d_status);
    return 0;
}
extern "C" int zmi_launch_zip_close(uint8_t* d_out, uint64_t out_cap, const uint64_t* d_pay_end, const uint64_t* d_cd_end, const uint32_t* d_n_eff,
                                    uint64_t base, uint64_t* d_out_len, zmi_zip_info* d_info, int32_t* d_status, hipStream_t stream) {
    ZMI_LAUNCH(zmi_zip_close_kernel, dim3(1), dim3(1), 0, stream, d_out, out_cap, d_pay_end, d_cd_end, d_n_eff, base, d_out_len, d_info, d_status);
    return 0;
}

// ---- reading PNG images (zmi_png_headers_dev / zmi_png_decode_dev) ------------------------------------------------------------------------
#include "png_kernels.h"

// ---- reading TIFF files (zmi_tiff_directory_dev / zmi_tiff_read_dev) ---------------------------------------------------------------------
#include "tiff_kernels.h"

// ---- writing TIFF files (zmi_tiff_write_dev) ------------------------------------------------------------------------------------------------
#include "tiff_write_kernels.h"

// ---- reading OpenEXR images (zmi_exr_headers_dev / zmi_exr_read_dev) ----------------------------------------------------------------------
#include "exr_kernels.h"

// ---- writing OpenEXR images (zmi_exr_bound / zmi_exr_write_dev) ---------------------------------------------------------------------------
#include "exr_write_kernels.h"
