// exr_kernels.h -- reading OpenEXR images with ZIP / ZIPS / PXR24 compression (zmi_exr_headers_dev / zmi_exr_read_dev, include/zmi355.h, which
// states the format); included by pack.hip.
//
// A file is a list of attributes, a table of chunk positions and the chunks: 16 scanlines (ZIP), one (ZIPS, NONE) or one tile each, every
// compressed chunk one zlib stream of its own -- the input shape of the batch decoder.  The kernels:
//   zmi_exr_headers_kernel   one lane per file walks the attribute list (it is serial: an attribute ends where its size says) and writes
//                            the zmi_exr_image record and the file's first chan_cap zmi_exr_channel records
//   zmi_exr_slots_kernel     pass 0: what every slot reads -- region size, chunk count, raw bytes -- for the plan and the two scans;
//                            pass 1, behind them: which slots fit the host's two bounds and out_cap
//   zmi_exr_chunks_kernel    one thread per chunk of the selection: table entry, chunk header, the decoder's tables, the raw copies'
//                            lengths, the work items of the unzip
//   zmi_exr_blocksum_kernel  one byte sum per EXR_BLOCK bytes of every inflated chunk, and zmi_exr_blockscan_kernel, their scan per chunk:
//                            the carries of the unzip
//   zmi_exr_unzip_kernel     the hot path, below
//   zmi_exr_pxr24_undo_kernel   the same for the streams of PXR24 files, which inflate to byte planes of differences: further below
//   zmi_exr_finish_kernel    one wave per slot: the slot's final words
#pragma once

static_assert(sizeof(zmi_exr_image) == 88u && sizeof(zmi_exr_channel) == 24u, "the records of include/zmi355.h: 88 and 24 bytes");
#define EXR_E_ARG (-103)
#define EXR_VERSION_ERROR (-6)
#define EXR_MEM_ERROR (-4)
#define EXR_TRIP 2048u               // output bytes of one trip of a wave: 64 lanes x 16 bytes of each of the two streams
#define EXR_PIECE (4u * EXR_TRIP)    // the longest piece of a run one work item writes
#define EXR_BLOCK 1024u              // bytes of an inflated chunk per byte sum
#define EXR_FL_CHUNK 1u
#define EXR_FL_MISSING 2u

static __device__ __forceinline__ uint32_t xr_u32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static __device__ __forceinline__ uint64_t xr_u64(const uint8_t* p) { return (uint64_t)xr_u32(p) | (uint64_t)xr_u32(p + 4) << 32; }
// a name at f[pos ..): *len = its bytes in front of the 0; false where it leaves [0, end) or is longer than max_name
static __device__ __forceinline__ bool xr_name(const uint8_t* f, uint64_t end, uint64_t pos, uint32_t max_name, uint32_t* len) {
    for (uint32_t k = 0u; k <= max_name; ++k) {
        if (pos + k >= end) return false;
        if (f[pos + k] == 0u) { *len = k; return true; }
    }
    return false;
}
static __device__ __forceinline__ bool xr_is(const uint8_t* p, uint32_t len, const char* word) {
    uint32_t k = 0u;
    while (k < len && word[k] != 0 && p[k] == (uint8_t)word[k]) ++k;
    return k == len && word[k] == 0;
}
static __device__ __forceinline__ uint32_t xr_lines(uint32_t compression) {
    return compression < 3u ? 1u : (compression == 3u || compression == 5u ? 16u : (compression == 9u ? 256u : 32u));
}
static __device__ __forceinline__ uint32_t xr_type_bytes(int32_t pixel_type) { return pixel_type == 1 ? 2u : 4u; }
// the bytes of a sample inside a PXR24 stream: a FLOAT keeps 24 bits
static __device__ __forceinline__ uint32_t xr_p24_bytes(int32_t pixel_type) { return pixel_type == 1 ? 2u : (pixel_type == 2 ? 3u : 4u); }

// What follows from the windows, the compression, the tile description and the channel types alone: the sizes the record keeps.
struct xr_geo {
    uint64_t W, H, row_bytes, region, n_chunks, chunk_raw;
    bool big;
};
// ch_type(c) is read through `chans` (the table) -- n_ch entries are there
static __device__ __forceinline__ void xr_geometry(const int32_t* dw, uint32_t lines, bool tiled, uint32_t tw, uint32_t th, const zmi_exr_channel* chans,
                                                   uint32_t n_listed, uint64_t n_ch, xr_geo* g) {
    g->W = (uint64_t)((int64_t)dw[2] - (int64_t)dw[0] + 1);
    g->H = (uint64_t)((int64_t)dw[3] - (int64_t)dw[1] + 1);
    uint64_t per_px = 0ull;
    for (uint32_t c = 0u; c < n_listed; ++c) per_px += xr_type_bytes(chans[c].pixel_type);
    g->big = g->W > 0xFFFFFFFFull || g->H > 0xFFFFFFFFull || n_ch > (uint64_t)n_listed;
    const uint64_t px = g->big ? 0ull : g->W * g->H;
    if (px > 0xFFFFFFFFull) g->big = true;
    g->row_bytes = g->big ? 0ull : g->W * per_px;
    uint64_t off = 0ull;
    if (!g->big)
        for (uint32_t c = 0u; c < n_listed; ++c) off = ((off + 3ull) & ~3ull) + px * xr_type_bytes(chans[c].pixel_type);
    g->region = off;
    const uint64_t cw = tiled && (uint64_t)tw < g->W ? (uint64_t)tw : g->W;
    const uint64_t rows = tiled ? ((uint64_t)th < g->H ? (uint64_t)th : g->H) : ((uint64_t)lines < g->H ? (uint64_t)lines : g->H);
    g->chunk_raw = g->big ? 0ull : rows * cw * per_px;
    if (g->row_bytes > 0xFFFFFFFFull || g->region > 0xFFFFFFFFull || g->chunk_raw > 0xFFFFFFFFull) g->big = true;
    if (tiled) {
        const uint64_t tx = (g->W + tw - 1ull) / tw, ty = (g->H + th - 1ull) / th;      // (tw, th >= 1: the caller's check)
        g->n_chunks = tx > 0xFFFFFFFFull / ty ? ~0ull : tx * ty;
    } else {
        g->n_chunks = (g->H + lines - 1ull) / lines;
    }
}

__global__ void __launch_bounds__(64) zmi_exr_headers_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                             const uint32_t* __restrict__ in_len, uint32_t n, zmi_exr_image* __restrict__ images,
                                                             zmi_exr_channel* __restrict__ chans, uint32_t chan_cap) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint8_t* f = in + in_off[i];
    const uint64_t L = in_len[i];
    zmi_exr_channel* ch = chans + (uint64_t)i * chan_cap;
    zmi_exr_image r;
    r.version = 0u; r.compression = r.line_order = r.tile_mode = r.tiled = 0u;
    for (uint32_t k = 0u; k < 4u; ++k) r.data_window[k] = r.display_window[k] = 0;
    r.width = r.height = r.lines_per_chunk = r.tile_w = r.tile_h = r.n_channels = r.n_chunks = r.row_bytes = r.region_bytes = 0u;
    r.status = 0; r.table_pos = 0ull;
    for (uint32_t c = 0u; c < chan_cap; ++c) { ch[c].name_pos = ch[c].name_len = ch[c].plane_off = 0u; ch[c].pixel_type = ch[c].x_sampling = ch[c].y_sampling = 0; }
    if (L < 8ull || f[0] != 0x76u || f[1] != 0x2Fu || f[2] != 0x31u || f[3] != 0x01u) { r.status = ZMI_XE_MAGIC; images[i] = r; return; }
    const uint32_t version = xr_u32(f + 4);
    r.version = version;
    r.tiled = (version & 0x200u) ? 1u : 0u;
    const uint32_t max_name = (version & 0x400u) ? 255u : 31u;
    bool bad = (version & 0xFFu) != 2u;
    bool has_ch = false, has_comp = false, has_dw = false, has_disp = false, has_lo = false, has_tiles = false;
    uint64_t ch_pos = 0ull, ch_end = 0ull, pos = 8ull;
    uint32_t comp = 0u, lo = 0u, tw = 0u, th = 0u, mode = 0u;
    uint32_t n_attr = 0u;
    while (!bad) {
        uint32_t nlen = 0u, tlen = 0u;
        if (!xr_name(f, L, pos, max_name, &nlen)) { bad = true; break; }
        if (nlen == 0u) { pos += 1ull; break; }                       // the header's end byte
        if (++n_attr > ZMI_EXR_ATTRS_MAX) { bad = true; break; }
        const uint8_t* name = f + pos;
        pos += nlen + 1ull;
        if (!xr_name(f, L, pos, max_name, &tlen) || tlen == 0u) { bad = true; break; }
        pos += tlen + 1ull;
        if (L - pos < 4ull) { bad = true; break; }
        const int32_t size = (int32_t)xr_u32(f + pos);
        pos += 4ull;
        if (size < 0 || (uint64_t)size > L - pos) { bad = true; break; }
        const uint8_t* v = f + pos;
        // (an attribute that stands twice: the first counts)
        if (xr_is(name, nlen, "channels")) {
            if (!has_ch) { has_ch = true; ch_pos = pos; ch_end = pos + (uint64_t)size; }
        } else if (xr_is(name, nlen, "compression")) {
            if (size != 1) bad = true; else if (!has_comp) { has_comp = true; comp = v[0]; }
        } else if (xr_is(name, nlen, "dataWindow")) {
            if (size != 16) bad = true; else if (!has_dw) { has_dw = true; for (uint32_t k = 0u; k < 4u; ++k) r.data_window[k] = (int32_t)xr_u32(v + 4u * k); }
        } else if (xr_is(name, nlen, "displayWindow")) {
            if (size != 16) bad = true; else if (!has_disp) { has_disp = true; for (uint32_t k = 0u; k < 4u; ++k) r.display_window[k] = (int32_t)xr_u32(v + 4u * k); }
        } else if (xr_is(name, nlen, "lineOrder")) {
            if (size != 1) bad = true; else if (!has_lo) { has_lo = true; lo = v[0]; }
        } else if (xr_is(name, nlen, "tiles")) {
            if (size != 9) bad = true; else if (!has_tiles) { has_tiles = true; tw = xr_u32(v); th = xr_u32(v + 4); mode = v[8]; }
        }
        pos += (uint64_t)size;
    }
    if (!has_ch || !has_comp || !has_dw || !has_lo || (r.tiled && !has_tiles)) bad = true;
    if (!bad && (r.data_window[2] < r.data_window[0] || r.data_window[3] < r.data_window[1] || comp > 9u || lo > 2u)) bad = true;
    if (!bad && r.tiled && (tw == 0u || th == 0u || (mode & 15u) > 2u || (mode >> 4) > 1u)) bad = true;
    // the channel list: n_ch counts every entry, the first chan_cap are written
    uint64_t n_ch = 0ull;
    bool sampled = false;
    if (!bad) {
        uint64_t p = ch_pos;
        for (;;) {
            uint32_t nlen = 0u;
            if (!xr_name(f, ch_end, p, max_name, &nlen)) { bad = true; break; }
            if (nlen == 0u) { if (p + 1ull != ch_end) bad = true; break; }
            const uint64_t q = p + nlen + 1ull;
            if (ch_end - q < 16ull) { bad = true; break; }
            const int32_t pt = (int32_t)xr_u32(f + q), xs = (int32_t)xr_u32(f + q + 8), ys = (int32_t)xr_u32(f + q + 12);
            if (pt < 0 || pt > 2 || xs < 1 || ys < 1) { bad = true; break; }
            if (xs != 1 || ys != 1) sampled = true;
            if (n_ch < (uint64_t)chan_cap) {
                zmi_exr_channel e;
                e.name_pos = (uint32_t)p; e.name_len = nlen; e.pixel_type = pt; e.x_sampling = xs; e.y_sampling = ys; e.plane_off = 0u;
                ch[n_ch] = e;
            }
            ++n_ch;
            p = q + 16ull;
        }
        if (n_ch == 0ull) bad = true;
    }
    xr_geo g;
    g.W = g.H = g.row_bytes = g.region = g.n_chunks = g.chunk_raw = 0ull; g.big = false;
    const uint32_t lines = xr_lines(comp > 9u ? 0u : comp);
    if (!bad) {
        const uint32_t n_listed = n_ch < (uint64_t)chan_cap ? (uint32_t)n_ch : chan_cap;
        xr_geometry(r.data_window, lines, r.tiled != 0u, tw, th, ch, n_listed, n_ch, &g);
        // the offset table stands directly behind the header (mip / rip files: at least the chunks of level 0)
        if (g.n_chunks > (L - pos) / 8ull) bad = true;
    }
    if (bad) {
        for (uint32_t k = 0u; k < 4u; ++k) r.data_window[k] = r.display_window[k] = 0;
        for (uint32_t c = 0u; c < chan_cap; ++c) { ch[c].name_pos = ch[c].name_len = 0u; ch[c].pixel_type = ch[c].x_sampling = ch[c].y_sampling = 0; }
        r.status = ZMI_XE_HEADER; images[i] = r;
        return;
    }
    r.compression = (uint8_t)comp; r.line_order = (uint8_t)lo; r.tile_mode = (uint8_t)mode;
    r.width = g.W > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)g.W;
    r.height = g.H > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)g.H;
    r.lines_per_chunk = lines;
    r.tile_w = r.tiled ? tw : 0u; r.tile_h = r.tiled ? th : 0u;
    r.n_channels = n_ch > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n_ch;
    r.n_chunks = (uint32_t)g.n_chunks;                                   // (inside the file: below 2^32 / 8)
    r.table_pos = pos;
    const bool many = n_ch > (uint64_t)chan_cap;
    if (!g.big) {
        r.row_bytes = (uint32_t)g.row_bytes; r.region_bytes = (uint32_t)g.region;
        uint64_t off = 0ull;
        for (uint32_t c = 0u; c < (uint32_t)n_ch; ++c) {                 // (not big: every channel is listed)
            off = (off + 3ull) & ~3ull;
            ch[c].plane_off = (uint32_t)off;
            off += g.W * g.H * xr_type_bytes(ch[c].pixel_type);
        }
    }
    if (version & 0x1800u) r.status = ZMI_XE_KIND;
    else if (comp != 0u && comp != 2u && comp != 3u && comp != 5u) r.status = ZMI_XE_COMPRESSION;
    else if (sampled) r.status = ZMI_XE_SAMPLING;
    else if (r.tiled && (mode & 15u) != 0u) r.status = ZMI_XE_LEVELS;
    else if (many) r.status = ZMI_XE_CHANNELS;
    else if (g.big) r.status = ZMI_XE_BIG;
    images[i] = r;
}

// A record with status 0 that a headers call would write for a file of L bytes (everything the reader derives an address from is
// derived again and compared).
static __device__ __forceinline__ bool xr_rec_ok(const zmi_exr_image& r, const zmi_exr_channel* ch, uint32_t chan_cap, uint64_t L) {
    if ((r.version & 0xFFu) != 2u || (r.version & 0x1800u) != 0u || (r.tiled != 0u) != ((r.version & 0x200u) != 0u) || r.tiled > 1u) return false;
    if (r.compression != 0u && r.compression != 2u && r.compression != 3u && r.compression != 5u) return false;
    if (r.lines_per_chunk != xr_lines(r.compression) || r.line_order > 2u) return false;
    if (r.data_window[2] < r.data_window[0] || r.data_window[3] < r.data_window[1]) return false;
    if (r.n_channels == 0u || r.n_channels > chan_cap) return false;
    if (r.tiled ? (r.tile_w == 0u || r.tile_h == 0u || (r.tile_mode & 15u) != 0u || (r.tile_mode >> 4) > 1u) : (r.tile_w != 0u || r.tile_h != 0u)) return false;
    for (uint32_t c = 0u; c < r.n_channels; ++c)
        if (ch[c].pixel_type < 0 || ch[c].pixel_type > 2 || ch[c].x_sampling != 1 || ch[c].y_sampling != 1) return false;
    xr_geo g;
    xr_geometry(r.data_window, r.lines_per_chunk, r.tiled != 0u, r.tile_w, r.tile_h, ch, r.n_channels, r.n_channels, &g);
    if (g.big || g.W != (uint64_t)r.width || g.H != (uint64_t)r.height || g.row_bytes != (uint64_t)r.row_bytes || g.region != (uint64_t)r.region_bytes) return false;
    if (g.n_chunks != (uint64_t)r.n_chunks) return false;
    if (r.table_pos < 9ull || r.table_pos > L || (uint64_t)r.n_chunks > (L - r.table_pos) / 8ull) return false;
    uint64_t off = 0ull;
    for (uint32_t c = 0u; c < r.n_channels; ++c) {
        off = (off + 3ull) & ~3ull;
        if ((uint64_t)ch[c].plane_off != off) return false;
        off += g.W * g.H * xr_type_bytes(ch[c].pixel_type);
    }
    return true;
}

// the largest k <= n - 1 with off[k] <= x (off: n + 1 ascending words, x < off[n])
static __device__ __forceinline__ uint32_t xr_find(const uint64_t* __restrict__ off, uint32_t n, uint64_t x) {
    uint32_t lo = 0u, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// kind[j]: 0 a readable file, 2 a file the headers call flagged, 3 nothing this call may touch (an index outside the table, a record
// no headers call writes for the file).  pass 0: size[j] = the region, nch[j] = the chunks, rawb[j] = the raw bytes of a readable slot,
// else 0.  pass 1, behind the plan (pcap) and the scans of nch and rawb: live[j] = the slot is read.
__global__ void __launch_bounds__(256) zmi_exr_slots_kernel(const uint32_t* __restrict__ in_len, const zmi_exr_image* __restrict__ images,
                                                            const zmi_exr_channel* __restrict__ chans, uint32_t chan_cap, uint32_t n_files,
                                                            const uint32_t* __restrict__ sel, uint32_t n_sel, uint32_t pass, uint64_t chunk_cap,
                                                            uint64_t decoded_bytes, const uint32_t* __restrict__ pcap,
                                                            const uint64_t* __restrict__ ch_off, const uint64_t* __restrict__ raw_off,
                                                            uint32_t* __restrict__ size, uint32_t* __restrict__ nch, uint32_t* __restrict__ rawb,
                                                            uint32_t* __restrict__ kind, uint32_t* __restrict__ live) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    if (pass == 1u) {
        live[j] = kind[j] == 0u && pcap[j] != 0u && ch_off[j + 1u] <= chunk_cap && raw_off[j + 1u] <= decoded_bytes ? 1u : 0u;
        return;
    }
    const uint32_t f = sel ? sel[j] : j;
    uint32_t k = 3u, sz = 0u, nc = 0u, rb = 0u;
    if (f < n_files) {
        const zmi_exr_image r = images[f];
        if (r.status != 0) { if (r.status >= ZMI_XE_MAGIC && r.status <= ZMI_XE_BIG) k = 2u; }
        else if (xr_rec_ok(r, chans + (uint64_t)f * chan_cap, chan_cap, in_len[f])) {
            k = 0u; sz = r.region_bytes; nc = r.n_chunks; rb = r.height * r.row_bytes;     // (at most the region: 32 bits)
        }
    }
    kind[j] = k; size[j] = sz; nch[j] = nc; rawb[j] = rb;
}

// Chunk k of a readable file: where it stands in the image and what it holds.
struct xr_chunk {
    uint32_t x0, y0, cw, rows;   // the first pixel, the pixels of a row, the rows
    uint32_t tx, ty;             // tiles: the tile's coordinates
};
static __device__ __forceinline__ void xr_chunk_of(const zmi_exr_image& r, uint32_t k, xr_chunk* c) {
    if (r.tiled) {
        const uint32_t across = (uint32_t)(((uint64_t)r.width + r.tile_w - 1ull) / r.tile_w);
        c->tx = k % across; c->ty = k / across;
        c->x0 = c->tx * r.tile_w; c->y0 = c->ty * r.tile_h;
        c->cw = r.width - c->x0 < r.tile_w ? r.width - c->x0 : r.tile_w;
        c->rows = r.height - c->y0 < r.tile_h ? r.height - c->y0 : r.tile_h;
    } else {
        c->tx = c->ty = 0u; c->x0 = 0u; c->cw = r.width;
        c->y0 = k * r.lines_per_chunk;
        c->rows = r.height - c->y0 < r.lines_per_chunk ? r.height - c->y0 : r.lines_per_chunk;
    }
}

// One thread per chunk q of the table of chunk_cap entries; the chunks of slot j are ch_off[j] .. ch_off[j + 1).  For a chunk of a live
// slot whose table entry and header are right: csz[q] = its raw size n, zin_off[q] = where its data stands in d_in, and either zin_len[q]
// = dataSize (a zlib stream, nblk[q] blocks of byte sums) or rawlen[q] = n (stored raw); items[q] = the pieces of its runs; cm[q] = the
// bytes its stream must inflate to: n, but m for a PXR24 stream (compression 5), which has no blocks and no items of the unzip --
// pitems[q] = its runs, the items of zmi_exr_pxr24_undo_kernel.  Every other entry is all zeros but fl[q] (EXR_FL_*).
__global__ void __launch_bounds__(256) zmi_exr_chunks_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                             const uint32_t* __restrict__ in_len, const zmi_exr_image* __restrict__ images,
                                                             const zmi_exr_channel* __restrict__ chans, uint32_t chan_cap,
                                                             const uint32_t* __restrict__ sel, uint32_t n_sel, const uint64_t* __restrict__ ch_off,
                                                             const uint32_t* __restrict__ live, uint32_t chunk_cap, uint64_t* __restrict__ zin_off,
                                                             uint32_t* __restrict__ zin_len, uint32_t* __restrict__ csz, uint32_t* __restrict__ rawlen,
                                                             uint32_t* __restrict__ fl, uint32_t* __restrict__ items, uint32_t* __restrict__ nblk,
                                                             uint32_t* __restrict__ cslot, uint32_t* __restrict__ cm,
                                                             uint32_t* __restrict__ pitems) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= chunk_cap) return;
    uint64_t zo = 0ull;
    uint32_t zl = 0u, n_raw = 0u, rl = 0u, flag = 0u, it = 0u, nb = 0u, slot = 0u, want = 0u, pit = 0u;
    if ((uint64_t)q < ch_off[n_sel]) {
        const uint32_t j = xr_find(ch_off, n_sel, q);
        slot = j;
        if (live[j]) {
            const uint32_t f = sel ? sel[j] : j;
            const zmi_exr_image r = images[f];
            const zmi_exr_channel* ch = chans + (uint64_t)f * chan_cap;
            const uint8_t* file = in + in_off[f];
            const uint64_t L = in_len[f];
            const uint32_t k = q - (uint32_t)ch_off[j];
            xr_chunk c;
            xr_chunk_of(r, k, &c);
            uint32_t per_px = 0u, pieces = 0u, per_p = 0u;
            for (uint32_t x = 0u; x < r.n_channels; ++x) {
                const uint32_t s = xr_type_bytes(ch[x].pixel_type);
                per_px += s;
                per_p += xr_p24_bytes(ch[x].pixel_type);
                pieces += (c.cw * s + EXR_PIECE - 1u) / EXR_PIECE;          // (a chunk's raw size fits 32 bits, so does a run's)
            }
            const uint32_t n = c.rows * c.cw * per_px;
            const uint64_t e = xr_u64(file + r.table_pos + 8ull * k);
            const uint64_t hdr = r.tiled ? 20ull : 8ull;
            if (e == 0ull) flag = EXR_FL_MISSING;
            else if (e > L || L - e < hdr) flag = EXR_FL_CHUNK;
            else {
                const uint8_t* h = file + e;
                bool ok;
                if (r.tiled) ok = xr_u32(h) == c.tx && xr_u32(h + 4) == c.ty && xr_u32(h + 8) == 0u && xr_u32(h + 12) == 0u;
                else ok = (int32_t)xr_u32(h) == (int32_t)((int64_t)r.data_window[1] + (int64_t)c.y0);
                const int32_t ds = (int32_t)xr_u32(h + hdr - 4ull);
                if (!ok || ds < 0 || (uint32_t)ds > n || (uint64_t)ds > L - e - hdr || (r.compression == 0u && (uint32_t)ds != n)) flag = EXR_FL_CHUNK;
                else {
                    zo = in_off[f] + e + hdr;
                    n_raw = want = n;
                    it = c.rows * pieces;
                    if ((uint32_t)ds == n) rl = n;
                    else if (r.compression == 5u) { zl = (uint32_t)ds; want = c.rows * c.cw * per_p; it = 0u; pit = c.rows * r.n_channels; }
                    else { zl = (uint32_t)ds; nb = (n + EXR_BLOCK - 1u) / EXR_BLOCK; }
                }
            }
        }
    }
    zin_off[q] = zo; zin_len[q] = zl; csz[q] = n_raw; rawlen[q] = rl; fl[q] = flag; items[q] = it; nblk[q] = nb; cslot[q] = slot;
    cm[q] = want; pitems[q] = pit;
}

// ---- the unzip (the predictor and the interleave of a ZIP / ZIPS chunk) and the placement ----------------------------------------------------
// The inflated chunk is d[0 .. n); t[i] = (d[0] + .. + d[i] - 128 i) mod 256 and, with h = (n + 1) / 2, raw[2 i] = t[i], raw[2 i + 1] =
// t[h + i]; raw is the chunk's rows, every row the planar runs of its channels, and a run goes to its place in the channel's plane.  The
// scan spans the whole chunk -- up to a few MiB -- but its operator is addition mod 256, so the carry into any position is the byte sum of
// everything in front of it: zmi_exr_blocksum_kernel writes one sum per EXR_BLOCK bytes of d, their scan per chunk (one wave a chunk,
// zmi_exr_blockscan_kernel) gives every block its carry, and the work item of the main pass is a span of the OUTPUT: a (chunk, row,
// channel) run cut into pieces of EXR_PIECE bytes, the items numbered by a scan of the chunks' device counts.  Runs start at even raw offsets (every pixel size is even), so a span raw[a .. a + S) needs t[a / 2 ..) and t[h + a / 2 ..): two
// streams, each with a carry-in of its own = its block's carry + the bytes between the block's start and the stream's.
// A trip is EXR_TRIP output bytes: every lane takes 16 bytes of each stream -- aligned dwords joined by v_alignbyte, every address
// lane-dependent (a wave-uniform address may become a scalar load that drops the low bits) --, sums them with
// packed arithmetic on the even and the odd bytes apart (16-bit fields: no carry crosses into a neighbour byte), the lane totals go
// through the DPP wave scan, the lane rebuilds its prefix bytes, adds 128 at the odd positions of t (-128 = +128 mod 256) and merges
// the two streams' dwords with v_perm_b32 into the output's byte order: 32 bytes a lane.  The carry from trip to trip is wave-uniform.
// Stores are dwords where the destination is 4-aligned, halves where it is 2-aligned, bytes otherwise.  Raw-stored chunks, copied into
// the same scratch, take the same placement without the scan.
// Bounds: loads touch the dwords that hold a lane's own bytes only, so at most 3 bytes in front of and behind a chunk, and the 16-byte
// lines of the carry sums reach at most 15 bytes behind it -- inside the scratch, where every chunk starts at a multiple of 16 and 16
// bytes of margin stand at either end of it (between chunks the neighbour's bytes are what such a load sees; they are masked).
static __device__ __forceinline__ uint32_t xr_perm(uint32_t hi, uint32_t lo, uint32_t s) {
#ifdef ZMI_EMU
    const uint64_t both = (uint64_t)hi << 32 | lo;
    uint32_t r = 0u;
    for (uint32_t k = 0u; k < 4u; ++k) r |= (uint32_t)((both >> (8u * ((s >> (8u * k)) & 7u))) & 0xFFull) << (8u * k);
    return r;
#else
    return __builtin_amdgcn_perm(hi, lo, s);
#endif
}
// the sum of the four bytes of w, added to acc
static __device__ __forceinline__ uint32_t xr_sad(uint32_t w, uint32_t acc) {
#ifdef ZMI_EMU
    return acc + (w & 0xFFu) + ((w >> 8) & 0xFFu) + ((w >> 16) & 0xFFu) + (w >> 24);
#else
    return __builtin_amdgcn_sad_u8(w, 0u, acc);
#endif
}
// the low nb bytes of a dword, nb = 0 .. 4 (and above: all)
static __device__ __forceinline__ uint32_t xr_keep(uint32_t w, uint32_t nb) { return nb >= 4u ? w : (w & ((1u << (8u * nb)) - 1u)); }

// the sum of the first m >= 1 bytes of the 16-byte line at p (16-aligned; the whole line is loaded)
static __device__ __forceinline__ uint32_t xr_sum16(const uint8_t* p, uint32_t m) {
    const uint4 v = *(const uint4*)p;
    return xr_sad(xr_keep(v.x, m), xr_sad(xr_keep(v.y, m > 4u ? m - 4u : 0u),
           xr_sad(xr_keep(v.z, m > 8u ? m - 8u : 0u), xr_sad(xr_keep(v.w, m > 12u ? m - 12u : 0u), 0u))));
}

// w[0 .. 4) = the v <= 16 bytes at p (any alignment), zeros behind them
static __device__ __forceinline__ void xr_ld16(const uint8_t* p, uint32_t v, uint32_t* w) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = (const uint32_t*)(p - mis);
    const uint32_t ndw = (mis + v + 3u) >> 2;
    uint32_t d[5];
#pragma unroll
    for (uint32_t k = 0u; k < 5u; ++k) d[k] = k < ndw ? q[k] : 0u;
#pragma unroll
    for (uint32_t k = 0u; k < 4u; ++k) w[k] = xr_keep(__builtin_amdgcn_alignbyte(d[k + 1u], d[k], mis), v > 4u * k ? v - 4u * k : 0u);
}
// the first ov <= 32 bytes (even) of o[0 .. 8) to p, which is even
static __device__ __forceinline__ void xr_st32(uint8_t* p, const uint32_t* o, uint32_t ov) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    if (mis == 0u) {
        uint32_t* p4 = (uint32_t*)p;
        const uint32_t nd = ov >> 2;
#pragma unroll
        for (uint32_t k = 0u; k < 8u; ++k) {
            if (k < nd) p4[k] = o[k];
            else if (k == nd && (ov & 2u)) *(uint16_t*)(p + 4u * k) = (uint16_t)o[k];
        }
    } else if (mis == 2u) {
        uint16_t* p2 = (uint16_t*)p;
#pragma unroll
        for (uint32_t k = 0u; k < 16u; ++k)
            if (2u * k < ov) p2[k] = (uint16_t)(o[k >> 1] >> (16u * (k & 1u)));
    } else {
#pragma unroll
        for (uint32_t k = 0u; k < 32u; ++k)
            if (k < ov) p[k] = (uint8_t)(o[k >> 2] >> (8u * (k & 3u)));
    }
}

// block g of the call is block g - blk_off[q] of chunk q; a fixed grid takes the blocks in turn
__global__ void __launch_bounds__(64) zmi_exr_blocksum_kernel(const uint8_t* __restrict__ sbuf, const uint64_t* __restrict__ soff,
                                                              const uint32_t* __restrict__ csz, const uint32_t* __restrict__ scap,
                                                              const uint64_t* __restrict__ blk_off, uint32_t chunk_cap,
                                                              uint32_t* __restrict__ bsum) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = blk_off[chunk_cap];
    for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
        uint32_t sum = 0u;
        const uint32_t q = xr_find(blk_off, chunk_cap, g);
        const uint32_t n = csz[q];
        const uint32_t b0 = (uint32_t)(g - blk_off[q]) * EXR_BLOCK;
        if (scap[q] == n && b0 < n) {
            const uint32_t valid = n - b0 < EXR_BLOCK ? n - b0 : EXR_BLOCK;
            if (16u * lane < valid) sum = xr_sum16(sbuf + soff[q] + b0 + 16u * lane, valid - 16u * lane);
        }
        sum = zmi_wave_sum(sum);
        if (lane == 0u) bsum[g] = sum;
    }
}
// One wave per chunk: bpre[b] = the sum of the chunk's block sums in front of block b (mod 2^32: only the low byte is used).  A chunk
// has a few hundred blocks, the call may have a million: a scan per chunk, 64 blocks a step, instead of one scan over all of them.
__global__ void __launch_bounds__(64) zmi_exr_blockscan_kernel(const uint64_t* __restrict__ blk_off, uint32_t chunk_cap,
                                                               const uint32_t* __restrict__ bsum, uint32_t* __restrict__ bpre) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t q = blockIdx.x; q < chunk_cap; q += gridDim.x) {
        const uint64_t b0 = blk_off[q];
        const uint32_t nb = (uint32_t)(blk_off[q + 1u] - b0);
        uint32_t carry = 0u;
        for (uint32_t i = 0u; i < nb; i += 64u) {
            const uint32_t v = i + lane < nb ? bsum[b0 + i + lane] : 0u;
            const uint32_t incl = zmi_wave_incl_scan(v);
            if (i + lane < nb) bpre[b0 + i + lane] = carry + incl - v;
            carry += zmi_readlane(incl, 63u);
        }
    }
}

// the byte sum of d[0 .. i) of a chunk mod 256: the scan of the block sums, and the bytes of i's own block in front of i
static __device__ __forceinline__ uint32_t xr_carry(const uint8_t* d, uint32_t i, const uint32_t* __restrict__ bpre, uint64_t blk0, uint32_t lane) {
    const uint32_t blk = i / EXR_BLOCK, part = i % EXR_BLOCK;
    uint32_t sum = 0u;
    if (16u * lane < part) sum = xr_sum16(d + blk * EXR_BLOCK + 16u * lane, part - 16u * lane);
    return (zmi_wave_sum(sum) + bpre[blk0 + blk]) & 0xFFu;
}

// One stream's 16 bytes of a lane: on return t[0 .. 4) = the bytes of t at the lane's positions; carry (wave-uniform) = the byte sum in
// front of the trip, moved on by the trip's.  odd = the parity of the stream's first position.
static __device__ __forceinline__ void xr_scan16(const uint8_t* p, uint32_t v, uint32_t odd, uint32_t* carry, uint32_t* t) {
    uint32_t w[4], pe[4], po[4], base[4];
    if (v != 0u) xr_ld16(p, v, w);
    else w[0] = w[1] = w[2] = w[3] = 0u;
    uint32_t tot = 0u;
#pragma unroll
    for (uint32_t k = 0u; k < 4u; ++k) {
        const uint32_t e = w[k] & 0x00FF00FFu, o = (w[k] >> 8) & 0x00FF00FFu;
        const uint32_t pr = e + o;                      // (b0 + b1, b2 + b3)
        pe[k] = e + (pr << 16);                         // (b0, b0 + b1 + b2)
        po[k] = pr + (pr << 16);                        // (b0 + b1, b0 + b1 + b2 + b3)
        base[k] = tot;
        tot += (pr & 0xFFFFu) + (pr >> 16);
    }
    const uint32_t incl = zmi_wave_incl_scan(tot);
    const uint32_t excl = incl - tot + *carry;
    *carry = (*carry + zmi_readlane(incl, 63u)) & 0xFFu;
    const uint32_t fix_e = odd ? 0x00800080u : 0u, fix_o = odd ? 0u : 0x00800080u;
#pragma unroll
    for (uint32_t k = 0u; k < 4u; ++k) {
        const uint32_t c = ((excl + base[k]) & 0xFFu) * 0x00010001u;
        t[k] = ((pe[k] + c + fix_e) & 0x00FF00FFu) | (((po[k] + c + fix_o) & 0x00FF00FFu) << 8);
    }
}

__global__ void __launch_bounds__(64) zmi_exr_unzip_kernel(const zmi_exr_image* __restrict__ images, const zmi_exr_channel* __restrict__ chans,
                                                           uint32_t chan_cap, const uint32_t* __restrict__ sel, const uint64_t* __restrict__ ch_off,
                                                           const uint32_t* __restrict__ cslot, uint32_t chunk_cap,
                                                           const uint64_t* __restrict__ item_off, const uint8_t* __restrict__ sbuf,
                                                           const uint64_t* __restrict__ soff, const uint32_t* __restrict__ csz,
                                                           const uint32_t* __restrict__ scap, const uint32_t* __restrict__ slen,
                                                           const int32_t* __restrict__ sst, const uint32_t* __restrict__ rawlen,
                                                           const uint64_t* __restrict__ blk_off, const uint32_t* __restrict__ bpre, uint8_t* out,
                                                           const uint64_t* __restrict__ out_off) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = item_off[chunk_cap];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t q = xr_find(item_off, chunk_cap, it);
        const uint32_t idx = (uint32_t)(it - item_off[q]);
        const uint32_t n = csz[q];
        const bool stored = rawlen[q] != 0u;
        if (n == 0u || scap[q] != n || (!stored && (sst[q] != 0 || slen[q] != n))) continue;      // the slot reports why
        const uint32_t j = cslot[q];
        const uint32_t f = sel ? sel[j] : j;
        const zmi_exr_image r = images[f];
        const zmi_exr_channel* ch = chans + (uint64_t)f * chan_cap;
        xr_chunk c;
        xr_chunk_of(r, q - (uint32_t)ch_off[j], &c);
        uint32_t rb = 0u, per_row = 0u;
        for (uint32_t x = 0u; x < r.n_channels; ++x) {
            const uint32_t run = c.cw * xr_type_bytes(ch[x].pixel_type);
            rb += run;
            per_row += (run + EXR_PIECE - 1u) / EXR_PIECE;
        }
        const uint32_t row = idx / per_row;
        uint32_t rem = idx % per_row, x = 0u, choff = 0u;
        for (;; ++x) {
            const uint32_t run = c.cw * xr_type_bytes(ch[x].pixel_type);
            const uint32_t pieces = (run + EXR_PIECE - 1u) / EXR_PIECE;
            if (rem < pieces || x + 1u == r.n_channels) break;
            rem -= pieces; choff += run;
        }
        const uint32_t size = xr_type_bytes(ch[x].pixel_type);
        const uint32_t run = c.cw * size, p0 = rem * EXR_PIECE;
        const uint32_t len = run - p0 < EXR_PIECE ? run - p0 : EXR_PIECE;
        const uint32_t a = row * rb + choff + p0;                         // the piece is raw[a .. a + len), a and len even
        uint8_t* dst = out + out_off[j] + ch[x].plane_off + ((uint64_t)(c.y0 + row) * r.width + c.x0) * size + p0;
        const uint8_t* d = sbuf + soff[q];
        if (stored) {
            for (uint32_t t0 = 0u; t0 < len; t0 += EXR_TRIP) {
                const uint32_t m = len - t0 < EXR_TRIP ? len - t0 : EXR_TRIP;
                const uint32_t ov = 32u * lane < m ? (m - 32u * lane < 32u ? m - 32u * lane : 32u) : 0u;
                uint32_t o[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                if (ov != 0u) {
                    xr_ld16(d + a + t0 + 32u * lane, ov < 16u ? ov : 16u, o);
                    if (ov > 16u) xr_ld16(d + a + t0 + 32u * lane + 16u, ov - 16u, o + 4);
                    xr_st32(dst + t0 + 32u * lane, o, ov);
                }
            }
            continue;
        }
        const uint32_t h = (n + 1u) / 2u, ia = a / 2u, ib = h + a / 2u;
        const uint64_t blk0 = blk_off[q];
        uint32_t carry_a = xr_carry(d, ia, bpre, blk0, lane), carry_b = xr_carry(d, ib, bpre, blk0, lane);
        for (uint32_t t0 = 0u; t0 < len; t0 += EXR_TRIP) {
            const uint32_t m = (len - t0 < EXR_TRIP ? len - t0 : EXR_TRIP) / 2u;      // bytes of each stream in this trip
            const uint32_t v = 16u * lane < m ? (m - 16u * lane < 16u ? m - 16u * lane : 16u) : 0u;
            uint32_t ta[4], tb[4], o[8];
            xr_scan16(d + ia + t0 / 2u + 16u * lane, v, ia & 1u, &carry_a, ta);
            xr_scan16(d + ib + t0 / 2u + 16u * lane, v, ib & 1u, &carry_b, tb);
#pragma unroll
            for (uint32_t k = 0u; k < 4u; ++k) {
                o[2u * k] = xr_perm(tb[k], ta[k], 0x05010400u);
                o[2u * k + 1u] = xr_perm(tb[k], ta[k], 0x07030602u);
            }
            if (v != 0u) xr_st32(dst + t0 + 32u * lane, o, 2u * v);
        }
    }
}

// ---- the PXR24 undo (compression 5; include/zmi355.h states the layout) -----------------------------------------------------------------------
// The inflated chunk is d[0 .. m): for every row, for every channel, a run of p planes of w bytes, most significant first, that hold
// the differences of neighbouring samples as p-byte integers (p = 2 / 3 / 4 for HALF / FLOAT / UINT).  The scan is a prefix sum of
// 16-, 24- or 32-bit words and spans one run only, so there are no block sums: the work item is a whole (chunk, row, channel) run, one
// wave an item, the items numbered by a scan of their own (pitems of zmi_exr_chunks_kernel).  A trip is EXR_P24_TRIP pixels, four
// consecutive ones a lane: the lane's 4 bytes of every plane are two aligned dwords joined by v_alignbyte (a plane starts at any byte
// offset; every address depends on the lane; a dword is loaded only where it holds a byte of the lane's own), the
// planes are transposed into per-pixel words with v_perm_b32, the lane sums its four, the lane totals go through the DPP wave scan, the
// carry from trip to trip is wave-uniform; sums are taken in 32 bits and masked to 8 p bits (2^(8p) divides 2^32), FLOAT is shifted
// left by 8.  Stores: 16 bytes a lane for UINT and FLOAT where the destination stands at a multiple of 16, dwords otherwise (such a
// row is always 4-aligned); a HALF lane has 8 bytes: two dwords where 4-aligned, halves otherwise.
// Bounds: loads as for the unzip -- at most 3 bytes in front of and behind the chunk's m <= n bytes, inside the scratch's margins.
#define EXR_P24_TRIP 256u            // pixels of one trip of a wave: 64 lanes x 4
// the v <= 4 bytes at p (any alignment), zeros behind them
static __device__ __forceinline__ uint32_t xr_ld4(const uint8_t* p, uint32_t v) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = (const uint32_t*)(p - mis);
    const uint32_t lo = v != 0u ? q[0] : 0u;
    const uint32_t hi = mis + v > 4u ? q[1] : 0u;
    return xr_keep(__builtin_amdgcn_alignbyte(hi, lo, mis), v);
}

__global__ void __launch_bounds__(64) zmi_exr_pxr24_undo_kernel(const zmi_exr_image* __restrict__ images, const zmi_exr_channel* __restrict__ chans,
                                                                uint32_t chan_cap, const uint32_t* __restrict__ sel, const uint64_t* __restrict__ ch_off,
                                                                const uint32_t* __restrict__ cslot, uint32_t chunk_cap,
                                                                const uint64_t* __restrict__ pitem_off, const uint8_t* __restrict__ sbuf,
                                                                const uint64_t* __restrict__ soff, const uint32_t* __restrict__ csz,
                                                                const uint32_t* __restrict__ scap, const uint32_t* __restrict__ cm,
                                                                const uint32_t* __restrict__ slen, const int32_t* __restrict__ sst, uint8_t* out,
                                                                const uint64_t* __restrict__ out_off) {
    const uint32_t lane = threadIdx.x;
    const uint64_t total = pitem_off[chunk_cap];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t q = xr_find(pitem_off, chunk_cap, it);
        const uint32_t idx = (uint32_t)(it - pitem_off[q]);
        const uint32_t n = csz[q];
        if (n == 0u || scap[q] != n || sst[q] != 0 || slen[q] != cm[q]) continue;                   // the slot reports why
        const uint32_t j = cslot[q];
        const uint32_t f = sel ? sel[j] : j;
        const zmi_exr_image r = images[f];
        const zmi_exr_channel* ch = chans + (uint64_t)f * chan_cap;
        xr_chunk c;
        xr_chunk_of(r, q - (uint32_t)ch_off[j], &c);
        const uint32_t row = idx / r.n_channels, x = idx % r.n_channels;
        uint32_t per_row = 0u, choff = 0u;
        for (uint32_t y = 0u; y < r.n_channels; ++y) {
            const uint32_t run = c.cw * xr_p24_bytes(ch[y].pixel_type);
            if (y < x) choff += run;
            per_row += run;
        }
        const int32_t type = ch[x].pixel_type;
        const uint32_t p = xr_p24_bytes(type), size = xr_type_bytes(type), w = c.cw;
        const uint32_t mask = p == 4u ? 0xFFFFFFFFu : (1u << (8u * p)) - 1u, sh = type == 2 ? 8u : 0u;
        const uint8_t* src = sbuf + soff[q] + (uint64_t)row * per_row + choff;
        uint8_t* dst = out + out_off[j] + ch[x].plane_off + ((uint64_t)(c.y0 + row) * r.width + c.x0) * size;
        uint32_t carry = 0u;
        for (uint32_t t0 = 0u; t0 < w; t0 += EXR_P24_TRIP) {
            const uint32_t left = w - t0 < EXR_P24_TRIP ? w - t0 : EXR_P24_TRIP;
            const uint32_t v = 4u * lane < left ? (left - 4u * lane < 4u ? left - 4u * lane : 4u) : 0u;
            const uint32_t px = t0 + 4u * lane;
            uint32_t a[4];
#pragma unroll
            for (uint32_t k = 0u; k < 4u; ++k) a[k] = k < p ? xr_ld4(src + (uint64_t)k * w + px, v) : 0u;
            // b0 .. b3: the planes of bits 24 - 31 .. 0 - 7
            const uint32_t b3 = p == 4u ? a[3] : (p == 3u ? a[2] : a[1]), b2 = p == 4u ? a[2] : (p == 3u ? a[1] : a[0]);
            const uint32_t b1 = p == 4u ? a[1] : (p == 3u ? a[0] : 0u), b0 = p == 4u ? a[0] : 0u;
            const uint32_t lo01 = xr_perm(b2, b3, 0x05010400u), lo23 = xr_perm(b2, b3, 0x07030602u);
            const uint32_t hi01 = xr_perm(b0, b1, 0x05010400u), hi23 = xr_perm(b0, b1, 0x07030602u);
            uint32_t s[4];
            s[0] = xr_perm(hi01, lo01, 0x05040100u);
            s[1] = s[0] + xr_perm(hi01, lo01, 0x07060302u);
            s[2] = s[1] + xr_perm(hi23, lo23, 0x05040100u);
            s[3] = s[2] + xr_perm(hi23, lo23, 0x07060302u);
            const uint32_t incl = zmi_wave_incl_scan(s[3]);
            const uint32_t excl = incl - s[3] + carry;
            carry += zmi_readlane(incl, 63u);
            uint32_t o[4];
#pragma unroll
            for (uint32_t k = 0u; k < 4u; ++k) o[k] = ((excl + s[k]) & mask) << sh;
            if (v == 0u) {
            } else if (size == 4u) {
                uint32_t* p4 = (uint32_t*)(dst + 4ull * px);
                if (v == 4u && ((uintptr_t)p4 & 15u) == 0u) {
                    uint4 u;
                    u.x = o[0]; u.y = o[1]; u.z = o[2]; u.w = o[3];
                    *(uint4*)p4 = u;
                } else {
#pragma unroll
                    for (uint32_t k = 0u; k < 4u; ++k)
                        if (k < v) p4[k] = o[k];
                }
            } else {
                uint8_t* p2 = dst + 2ull * px;
                if (v == 4u && ((uintptr_t)p2 & 3u) == 0u) {
                    ((uint32_t*)p2)[0] = o[0] | o[1] << 16;
                    ((uint32_t*)p2)[1] = o[2] | o[3] << 16;
                } else {
#pragma unroll
                    for (uint32_t k = 0u; k < 4u; ++k)
                        if (k < v) ((uint16_t*)p2)[k] = (uint16_t)o[k];
                }
            }
        }
    }
}

// the decoder's capacity of chunk q: the bytes its stream must inflate to, where the plan gave the chunk its room in the scratch
__global__ void __launch_bounds__(256) zmi_exr_deccap_kernel(const uint32_t* __restrict__ csz, const uint32_t* __restrict__ scap,
                                                             const uint32_t* __restrict__ cm, uint32_t chunk_cap, uint32_t* __restrict__ dcap) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q < chunk_cap) dcap[q] = scap[q] == csz[q] ? cm[q] : 0u;
}

// One wave per slot, behind everything else: the slot's final words (include/zmi355.h states the order).
__global__ void __launch_bounds__(64) zmi_exr_finish_kernel(const zmi_exr_image* __restrict__ images, const uint32_t* __restrict__ sel, uint32_t n_sel,
                                                            const uint32_t* __restrict__ kind, const uint32_t* __restrict__ size,
                                                            const uint32_t* __restrict__ pcap,
                                                            const uint64_t* __restrict__ ch_off, const uint64_t* __restrict__ raw_off,
                                                            uint64_t chunk_cap, uint64_t decoded_bytes, const uint32_t* __restrict__ csz,
                                                            const uint32_t* __restrict__ scap, const uint32_t* __restrict__ rawlen,
                                                            const uint32_t* __restrict__ fl, const uint32_t* __restrict__ cm,
                                                            const uint32_t* __restrict__ slen,
                                                            const int32_t* __restrict__ sst, uint32_t* __restrict__ out_len,
                                                            int32_t* __restrict__ status, int32_t* __restrict__ detail) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    if (j >= n_sel) return;
    int32_t st = 0, det = 0;
    const uint32_t k = kind[j];
    if (k == 3u) st = EXR_E_ARG;
    else if (k == 2u) {
        const uint32_t f = sel ? sel[j] : j;
        det = images[f].status;
        st = (det == ZMI_XE_MAGIC || det == ZMI_XE_HEADER) ? ZMI_DATA_ERROR : (det == ZMI_XE_CHANNELS ? ZMI_BUF_ERROR : EXR_VERSION_ERROR);
    } else if (ch_off[j + 1u] > chunk_cap || raw_off[j + 1u] > decoded_bytes) st = EXR_E_ARG;
    else if (pcap[j] == 0u) { st = ZMI_BUF_ERROR; det = ZMI_XE_OUT; }
    else {
        // the first code in the order of the header that any chunk has, and the first chunk that has it
        const uint32_t q0 = (uint32_t)ch_off[j], q1 = (uint32_t)ch_off[j + 1u];
        uint32_t code = 0xFFu, at = 0xFFFFFFFFu;
        for (uint32_t q = q0 + lane; q < q1; q += 64u) {
            uint32_t cq = 0u;
            const uint32_t flag = fl[q];
            if (flag & EXR_FL_CHUNK) cq = ZMI_XE_CHUNK;
            else if (flag & EXR_FL_MISSING) cq = ZMI_XE_MISSING;
            else if (csz[q] == 0u || scap[q] != csz[q]) cq = ZMI_XE_SCRATCH;
            else if (rawlen[q] == 0u) {
                const int32_t ds = sst[q];
                if (ds == EXR_MEM_ERROR) cq = ZMI_XE_SCRATCH;
                else if (ds == ZMI_BUF_ERROR) cq = ZMI_XE_LENGTH;     // the stream wants more input, or more room than the chunk
                else if (ds != ZMI_OK) cq = ZMI_XE_DATA;
                else if (slen[q] != cm[q]) cq = ZMI_XE_LENGTH;
            }
            if (cq != 0u && cq < code) { code = cq; at = q - q0; }
        }
        uint32_t best = code;
        for (uint32_t s = 32u; s >= 1u; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)best, (int)s); best = o < best ? o : best; }
        uint32_t first = code == best ? at : 0xFFFFFFFFu;
        for (uint32_t s = 32u; s >= 1u; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)first, (int)s); first = o < first ? o : first; }
        if (best != 0xFFu) {
            st = best == ZMI_XE_SCRATCH ? EXR_MEM_ERROR : ZMI_DATA_ERROR;
            det = (int32_t)(best | (first & 0x7FFFFFu) << 8);
        }
    }
    if (lane == 0u) {
        status[j] = st;
        detail[j] = det;
        out_len[j] = st == 0 ? size[j] : 0u;
    }
}

extern "C" uint32_t zmi_exr_trip(void) { return EXR_TRIP; }
extern "C" uint32_t zmi_exr_piece(void) { return EXR_PIECE; }
extern "C" int zmi_launch_exr_headers(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, zmi_exr_image* d_images,
                                      zmi_exr_channel* d_chans, uint32_t chan_cap, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_exr_headers_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, d_in, d_in_off, d_in_len, n, d_images, d_chans, chan_cap);
    return 0;
}
extern "C" int zmi_launch_exr_slots(const uint32_t* d_in_len, const zmi_exr_image* d_images, const zmi_exr_channel* d_chans, uint32_t chan_cap,
                                    uint32_t n_files, const uint32_t* d_sel, uint32_t n_sel, uint32_t pass, uint64_t chunk_cap,
                                    uint64_t decoded_bytes, const uint32_t* d_pcap, const uint64_t* d_ch_off, const uint64_t* d_raw_off,
                                    uint32_t* d_size, uint32_t* d_nch, uint32_t* d_rawb, uint32_t* d_kind, uint32_t* d_live, hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_exr_slots_kernel, dim3((n_sel + 255u) / 256u), dim3(256), 0, stream, d_in_len, d_images, d_chans, chan_cap, n_files, d_sel, n_sel,
               pass, chunk_cap, decoded_bytes, d_pcap, d_ch_off, d_raw_off, d_size, d_nch, d_rawb, d_kind, d_live);
    return 0;
}
extern "C" int zmi_launch_exr_chunks(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_exr_image* d_images,
                                     const zmi_exr_channel* d_chans, uint32_t chan_cap, const uint32_t* d_sel, uint32_t n_sel,
                                     const uint64_t* d_ch_off, const uint32_t* d_live, uint32_t chunk_cap, uint64_t* d_zin_off, uint32_t* d_zin_len,
                                     uint32_t* d_csz, uint32_t* d_rawlen, uint32_t* d_fl, uint32_t* d_items, uint32_t* d_nblk, uint32_t* d_cslot,
                                     uint32_t* d_cm, uint32_t* d_pitems, hipStream_t stream) {
    if (chunk_cap == 0) return 0;
    ZMI_LAUNCH(zmi_exr_chunks_kernel, dim3((chunk_cap + 255u) / 256u), dim3(256), 0, stream, d_in, d_in_off, d_in_len, d_images, d_chans, chan_cap,
               d_sel, n_sel, d_ch_off, d_live, chunk_cap, d_zin_off, d_zin_len, d_csz, d_rawlen, d_fl, d_items, d_nblk, d_cslot, d_cm, d_pitems);
    return 0;
}
// bound: the most blocks the call can have (decoded_bytes / EXR_BLOCK and one a chunk); d_bsum and d_bpre hold as many words
extern "C" int zmi_launch_exr_blocksum(const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_csz, const uint32_t* d_scap,
                                       const uint64_t* d_blk_off, uint32_t chunk_cap, uint64_t bound, uint32_t* d_bsum, uint32_t* d_bpre,
                                       hipStream_t stream) {
    if (chunk_cap == 0 || bound == 0) return 0;
    const uint32_t grid = bound > 16384u ? 16384u : (uint32_t)bound;
    ZMI_LAUNCH(zmi_exr_blocksum_kernel, dim3(grid), dim3(64), 0, stream, d_sbuf, d_soff, d_csz, d_scap, d_blk_off, chunk_cap, d_bsum);
    ZMI_LAUNCH(zmi_exr_blockscan_kernel, dim3(chunk_cap > 16384u ? 16384u : chunk_cap), dim3(64), 0, stream, d_blk_off, chunk_cap,
               (const uint32_t*)d_bsum, d_bpre);
    return 0;
}
// bound: the most items the call can have (decoded_bytes / 2: a piece holds at least one pixel of 2 bytes); a fixed grid takes them in turn
extern "C" int zmi_launch_exr_unzip(const zmi_exr_image* d_images, const zmi_exr_channel* d_chans, uint32_t chan_cap, const uint32_t* d_sel,
                                    const uint64_t* d_ch_off, const uint32_t* d_cslot, uint32_t chunk_cap, const uint64_t* d_item_off, uint64_t bound,
                                    const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_csz, const uint32_t* d_scap,
                                    const uint32_t* d_slen, const int32_t* d_sst, const uint32_t* d_rawlen, const uint64_t* d_blk_off,
                                    const uint32_t* d_bpre, uint8_t* d_out, const uint64_t* d_out_off, hipStream_t stream) {
    if (chunk_cap == 0) return 0;
    const uint32_t grid = bound < 1u ? 1u : (bound > 16384u ? 16384u : (uint32_t)bound);
    ZMI_LAUNCH(zmi_exr_unzip_kernel, dim3(grid), dim3(64), 0, stream, d_images, d_chans, chan_cap, d_sel, d_ch_off, d_cslot, chunk_cap, d_item_off,
               d_sbuf, d_soff, d_csz, d_scap, d_slen, d_sst, d_rawlen, d_blk_off, d_bpre, d_out, d_out_off);
    return 0;
}
extern "C" uint32_t zmi_exr_pxr24_trip(void) { return EXR_P24_TRIP; }
extern "C" int zmi_launch_exr_deccap(const uint32_t* d_csz, const uint32_t* d_scap, const uint32_t* d_cm, uint32_t chunk_cap, uint32_t* d_dcap,
                                     hipStream_t stream) {
    if (chunk_cap == 0) return 0;
    ZMI_LAUNCH(zmi_exr_deccap_kernel, dim3((chunk_cap + 255u) / 256u), dim3(256), 0, stream, d_csz, d_scap, d_cm, chunk_cap, d_dcap);
    return 0;
}
// bound: the most items the call can have (decoded_bytes / 2: a run holds at least one pixel of 2 bytes); a fixed grid takes them in turn
extern "C" int zmi_launch_exr_pxr24_undo(const zmi_exr_image* d_images, const zmi_exr_channel* d_chans, uint32_t chan_cap, const uint32_t* d_sel,
                                         const uint64_t* d_ch_off, const uint32_t* d_cslot, uint32_t chunk_cap, const uint64_t* d_pitem_off,
                                         uint64_t bound, const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_csz,
                                         const uint32_t* d_scap, const uint32_t* d_cm, const uint32_t* d_slen, const int32_t* d_sst, uint8_t* d_out,
                                         const uint64_t* d_out_off, hipStream_t stream) {
    if (chunk_cap == 0) return 0;
    const uint32_t grid = bound < 1u ? 1u : (bound > 16384u ? 16384u : (uint32_t)bound);
    ZMI_LAUNCH(zmi_exr_pxr24_undo_kernel, dim3(grid), dim3(64), 0, stream, d_images, d_chans, chan_cap, d_sel, d_ch_off, d_cslot, chunk_cap,
               d_pitem_off, d_sbuf, d_soff, d_csz, d_scap, d_cm, d_slen, d_sst, d_out, d_out_off);
    return 0;
}
extern "C" int zmi_launch_exr_finish(const zmi_exr_image* d_images, const uint32_t* d_sel, uint32_t n_sel,
                                     const uint32_t* d_kind, const uint32_t* d_size, const uint32_t* d_pcap,
                                     const uint64_t* d_ch_off, const uint64_t* d_raw_off, uint64_t chunk_cap, uint64_t decoded_bytes,
                                     const uint32_t* d_csz, const uint32_t* d_scap, const uint32_t* d_rawlen, const uint32_t* d_fl,
                                     const uint32_t* d_cm, const uint32_t* d_slen, const int32_t* d_sst, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail,
                                     hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_exr_finish_kernel, dim3(n_sel), dim3(64), 0, stream, d_images, d_sel, n_sel, d_kind, d_size, d_pcap,
               d_ch_off, d_raw_off, chunk_cap, decoded_bytes, d_csz, d_scap, d_rawlen, d_fl, d_cm, d_slen, d_sst, d_out_len, d_status, d_detail);
    return 0;
}
