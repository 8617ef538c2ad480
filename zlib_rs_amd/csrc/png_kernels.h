// png_kernels.h -- reading PNG images (zmi_png_headers_dev / zmi_png_decode_dev, include/zmi355.h); included by pack.hip.
//
// The format is the W3C PNG specification, third edition (RFC 2083): a chain of chunks -- length u32 big-endian | type | data | CRC-32
// of type + data (section 5.3) -- behind an eight-byte signature (5.2); the image is ONE zlib stream cut into consecutive IDAT chunks
// (10.1) that inflates to `height` scanlines of a filter byte and row_bytes bytes (7.2, 9.2).  The kernels:
//   zmi_png_headers_kernel    one thread per file follows the chain (it is serial: a chunk's length stands in its first four bytes;
//                             the batch is the parallelism) and writes the zmi_png_image record
//   zmi_png_prep_kernel       the slots' region sizes for the plan; then, behind the plan, the scanline sizes, the gather sizes and the
//                             number of 64-row bands of every slot that fits
//   zmi_png_walk_kernel       PNG_WALK_K workgroups per slot follow the chain again; chunk number i is taken by workgroup i mod K, which
//                             stages it through LDS in 4 KiB tiles, folds the CRC-32 of the tile (slice-by-4 per thread, the threads'
//                             values joined by the crc32_combine algebra) and, for an image of several IDAT chunks, stores the payload
//                             into the slot's gathered stream.  The tables a chunk-by-chunk CRC launch and range copy would need have a
//                             length only the device knows, and the entry point is given no size of the input to bound them by: the walk
//                             does both where it stands, one read of the file
//   zmi_png_unfilter_kernel   the hot path, below
//   zmi_png_finish_kernel     the slots' final words
#pragma once
#include <type_traits>

#define PNG_E_ARG (-103)
#define PNG_VERSION_ERROR (-6)
#define PNG_MEM_ERROR (-4)
#define PNG_T 256u
#define PNG_TILE 4096u
#define PNG_WALK_K 8u
#define PNG_STRIP 512u           // bytes of a scanline one LDS strip holds
#define PNG_PITCH 520u           // LDS bytes per row of the strip: lane k reads at k * 520 + (misalignment 0 .. 3) + (t - k) * bpp -- about 129
                                 // dwords from lane to lane for bpp <= 4, so the skewed byte reads of a step spread over the banks
#define PNG_ROWS 64u
#define PNG_UNFILTER_LDS (PNG_ROWS * PNG_PITCH + 16u + PNG_STRIP + 16u)
#define PNG_FL_CRC 1u
#define PNG_FL_SCRATCH 2u
#define PNG_FL_FILTER 4u

static __device__ __forceinline__ uint32_t png_be32(const uint8_t* p) {
    return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}
#define PNG_IHDR 0x49484452u
#define PNG_PLTE 0x504C5445u
#define PNG_IDAT 0x49444154u
#define PNG_IEND 0x49454E44u
#define PNG_TRNS 0x74524E53u

__global__ void __launch_bounds__(256) zmi_png_headers_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                              const uint32_t* __restrict__ in_len, uint32_t n, zmi_png_image* __restrict__ img) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint8_t* f = in + in_off[i];
    const uint32_t L = in_len[i];
    zmi_png_image r;
    r.width = r.height = 0u; r.depth = r.colour = r.channels = r.bpp = 0; r.row_bytes = 0u; r.idat_pos = r.n_idat = r.idat_bytes = 0u;
    r.plte_pos = r.plte_len = r.trns_pos = r.trns_len = 0u; r.status = 0;
    bool sig = L >= 8u;
    if (sig) {
        const uint32_t s0 = png_be32(f), s1 = png_be32(f + 4);
        sig = s0 == 0x89504E47u && s1 == 0x0D0A1A0Au;
    }
    if (!sig) { r.status = ZMI_PE_SIGNATURE; img[i] = r; return; }
    if (L < 16u) { r.status = ZMI_PE_TRUNC; img[i] = r; return; }
    if (png_be32(f + 8) != 13u || png_be32(f + 12) != PNG_IHDR) { r.status = ZMI_PE_IHDR; img[i] = r; return; }
    if (L < 33u) { r.status = ZMI_PE_TRUNC; img[i] = r; return; }
    const uint32_t w = png_be32(f + 16), h = png_be32(f + 20);
    const uint32_t depth = f[24], colour = f[25], comp = f[26], filt = f[27], lace = f[28];
    uint32_t ch = 0u;
    if (colour == 0u) ch = (depth == 1u || depth == 2u || depth == 4u || depth == 8u || depth == 16u) ? 1u : 0u;
    else if (colour == 3u) ch = (depth == 1u || depth == 2u || depth == 4u || depth == 8u) ? 1u : 0u;
    else if (colour == 2u || colour == 4u || colour == 6u) ch = (depth == 8u || depth == 16u) ? (colour == 2u ? 3u : (colour == 4u ? 2u : 4u)) : 0u;
    if (w == 0u || h == 0u || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || ch == 0u || comp != 0u || filt != 0u || lace > 1u) {
        r.status = ZMI_PE_IHDR; img[i] = r; return;
    }
    const uint64_t rb = ((uint64_t)w * ch * depth + 7ull) >> 3;
    const bool big = rb > 0xFFFFFFFFull || (1ull + rb) * h > 0xFFFFFFFFull;
    r.width = w; r.height = h; r.depth = (uint8_t)depth; r.colour = (uint8_t)colour; r.channels = (uint8_t)ch;
    r.bpp = (uint8_t)(ch * depth >= 8u ? ch * depth / 8u : 1u);
    r.row_bytes = rb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)rb;
    if (lace == 1u) { r.status = ZMI_PE_INTERLACE; img[i] = r; return; }
    bool trunc = false, critical = false, order = false, seen = false, ended = false;
    uint32_t pos = 33u;
    for (;;) {
        if (L - pos < 12u) { trunc = true; break; }                    // (pos <= L always: a chunk that leaves the file ends the walk)
        const uint32_t len = png_be32(f + pos), type = png_be32(f + pos + 4);
        if (len > 0x7FFFFFFFu || len > L - pos - 12u) { trunc = true; break; }
        if (type == PNG_IDAT) {
            if (!seen) { seen = true; r.idat_pos = pos; }
            if (ended) order = true;
            else { r.n_idat++; r.idat_bytes += len; }
        } else {
            if (seen) ended = true;
            if (type == PNG_IEND) break;
            if (type == PNG_PLTE) {
                if (seen || len % 3u != 0u || len > 768u || r.plte_pos != 0u) order = true;
                if (r.plte_pos == 0u) { r.plte_pos = pos + 8u; r.plte_len = len; }
            } else if (type == PNG_TRNS) {
                if (r.trns_pos == 0u) { r.trns_pos = pos + 8u; r.trns_len = len; }
            } else if (type == PNG_IHDR) order = true;
            else if (((type >> 24) & 0x20u) == 0u) critical = true;
        }
        pos += 12u + len;
    }
    if (trunc) r.status = ZMI_PE_TRUNC;
    else if (critical) r.status = ZMI_PE_CRITICAL;
    else if (order || !seen || (colour == 3u && r.plte_pos == 0u)) r.status = ZMI_PE_ORDER;
    else if (big) r.status = ZMI_PE_BIG;
    img[i] = r;
}

// what slot j reads: 0 a readable image (*e its record, *L its file's length), 2 one the headers call flagged, 3 nothing this call may
// touch (an index outside the table, a record that cannot stand for this file)
static __device__ __forceinline__ uint32_t png_slot_kind(const zmi_png_image* __restrict__ img, uint32_t n_images, const uint32_t* __restrict__ sel,
                                                         uint32_t j, const uint32_t* __restrict__ in_len, zmi_png_image* e, uint32_t* k_out, uint32_t* L) {
    const uint32_t k = sel ? sel[j] : j;
    if (k >= n_images) return 3u;
    *k_out = k;
    *e = img[k];
    *L = in_len[k];
    if (e->status != 0) return (e->status >= ZMI_PE_SIGNATURE && e->status <= ZMI_PE_BIG) ? 2u : 3u;
    if (e->height == 0u || e->row_bytes == 0u || e->bpp == 0u || e->bpp > 8u || e->bpp == 5u || e->bpp == 7u || e->row_bytes % e->bpp != 0u || e->n_idat == 0u) return 3u;
    if ((1ull + e->row_bytes) * e->height > 0xFFFFFFFFull) return 3u;
    // the IDAT run -- n_idat chunks of 12 bytes and idat_bytes of payload from idat_pos -- and the IEND behind it lie inside the file
    if (e->idat_pos < 33u || (uint64_t)e->idat_pos + 12ull * e->n_idat + e->idat_bytes + 12ull > (uint64_t)*L) return 3u;
    return 0u;
}

// pass 0: pix[j] = the region's size (0 for a slot that reads nothing).  pass 1, behind the plan of the regions (pcap[j] = pix[j] where
// the region fits out_cap, else 0): ssz[j] = the scanlines' size, gsz[j] = the bytes to gather (an image of several IDAT chunks),
// items[j] = its bands of 64 rows, all 0 for a slot that is not decoded; fl[j] = 0
__global__ void __launch_bounds__(256) zmi_png_prep_kernel(const zmi_png_image* __restrict__ img, uint32_t n_images, const uint32_t* __restrict__ sel,
                                                           uint32_t n_sel, const uint32_t* __restrict__ in_len, uint32_t pass, uint32_t* __restrict__ pix,
                                                           const uint32_t* __restrict__ pcap, uint32_t* __restrict__ ssz, uint32_t* __restrict__ gsz,
                                                           uint32_t* __restrict__ items, uint32_t* __restrict__ fl) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    zmi_png_image e;
    uint32_t k, L;
    const uint32_t kind = png_slot_kind(img, n_images, sel, j, in_len, &e, &k, &L);
    if (pass == 0u) { pix[j] = kind == 0u ? e.height * e.row_bytes : 0u; return; }
    const bool live = kind == 0u && pcap[j] != 0u;
    ssz[j] = live ? (1u + e.row_bytes) * e.height : 0u;
    gsz[j] = live && e.n_idat > 1u ? e.idat_bytes : 0u;
    items[j] = live ? (e.height + PNG_ROWS - 1u) / PNG_ROWS : 0u;
    fl[j] = 0u;
}

// ---- the walk: chunk CRC-32 and the gather ------------------------------------------------------------------------------------------------
#define PNG_CRC_POLY 0xEDB88320u
// a(x) * b(x) mod P and x^(8 * nbytes) mod P, reflected bit order (the crc32_combine algebra, as in checksum.hip)
static __device__ __forceinline__ uint32_t png_gf2_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? PNG_CRC_POLY : 0u);
    }
    return p;
}
static __device__ __forceinline__ uint32_t png_gf2_xpow8(uint64_t nbytes) {
    uint32_t r = 0x80000000u, pw = 0x00800000u;
    while (nbytes) {
        if (nbytes & 1u) r = png_gf2_mulmod(r, pw);
        pw = png_gf2_mulmod(pw, pw);
        nbytes >>= 1;
    }
    return r;
}

// zin_off / zin_len: where the batch decoder reads slot j's zlib stream, as an offset from `in` -- into the file for a single IDAT, into
// the gather buffer `gbuf` (the difference of the two device addresses, modulo 2^64) for several
__global__ void __launch_bounds__(PNG_T) zmi_png_walk_kernel(const uint8_t* __restrict__ in, const uint64_t* __restrict__ in_off,
                                                             const uint32_t* __restrict__ in_len, const zmi_png_image* __restrict__ img,
                                                             const uint32_t* __restrict__ sel, const uint32_t* __restrict__ ssz,
                                                             const uint32_t* __restrict__ gsz, const uint64_t* __restrict__ goff,
                                                             const uint32_t* __restrict__ gcap, uint8_t* __restrict__ gbuf, uint32_t check_crc, uint32_t K,
                                                             uint64_t* __restrict__ zin_off, uint32_t* __restrict__ zin_len, uint32_t* __restrict__ fl) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[PNG_TILE + 32];
    __shared__ uint32_t tab[4][256];
    __shared__ uint32_t red[4];
    const uint32_t j = blockIdx.x / K, part = blockIdx.x % K, t = threadIdx.x;   // (one grid dimension: the emulator has no more)
    const bool live = ssz[j] != 0u;
    const uint32_t k = live ? (sel ? sel[j] : j) : 0u;
    zmi_png_image e = {};
    if (live) e = img[k];
    const bool multi = live && gsz[j] != 0u;
    const bool gok = !multi || gcap[j] != 0u;
    if (part == 0u && t == 0u) {
        uint64_t zo = 0ull;
        uint32_t zl = 0u;
        if (live && gok) {
            zl = e.idat_bytes;
            zo = multi ? (uint64_t)((uintptr_t)gbuf - (uintptr_t)in) + goff[j] : in_off[k] + e.idat_pos + 8u;
        }
        zin_off[j] = zo;
        zin_len[j] = zl;
        if (live && !gok) atomicOr(&fl[j], PNG_FL_SCRATCH);
    }
    if (!live || !gok || (!check_crc && !multi)) return;
    // slice-by-4 tables: tab[k][b] = the CRC of byte b followed by k zero bytes
    {
        uint32_t c = t;
        for (int q = 0; q < 8; ++q) c = (c >> 1) ^ ((c & 1u) ? PNG_CRC_POLY : 0u);
        tab[0][t] = c;
        __syncthreads();
        for (uint32_t q = 1; q < 4u; ++q) {
            c = (c >> 8) ^ tab[0][c & 0xFFu];
            tab[q][t] = c;
        }
        __syncthreads();
    }
    const uint32_t kfull = check_crc ? png_gf2_xpow8(16u * (255u - t)) : 0u;   // a full tile: the bytes behind this thread's sixteen
    const uint32_t ktile = check_crc ? png_gf2_xpow8(PNG_TILE) : 0u;
    const uint8_t* f = in + in_off[k];
    const uint32_t L = in_len[k];
    uint8_t* gdst = gbuf + (multi ? goff[j] : 0ull);
    const uint32_t glim = multi ? gsz[j] : 0u;
    uint32_t pos = 8u, idx = 0u, run = 0u, gpos = 0u;
    while (pos <= L && L - pos >= 12u) {
        const uint32_t len = png_be32(f + pos), type = png_be32(f + pos + 4);
        if (len > 0x7FFFFFFFu || len > L - pos - 12u) break;
        const bool idat = type == PNG_IDAT;
        const bool crit = idat || type == PNG_IHDR || type == PNG_PLTE || type == PNG_IEND;
        bool copy = false;
        if (idat && multi && pos >= e.idat_pos && run < e.n_idat) { copy = gpos <= glim && len <= glim - gpos; ++run; }
        if ((crit && check_crc) || copy) {
            if (idx % K == part) {
                const uint8_t* s = f + pos + 4u;            // type + data
                const uint32_t l = len + 4u;
                const uint32_t mis = (uint32_t)((uintptr_t)s & 15u);
                uint32_t crc = 0u;                         // the zero-init raw CRC of the tiles so far
                for (uint32_t base = 0u; base < l; base += PNG_TILE) {
                    const uint32_t nb = l - base < PNG_TILE ? l - base : PNG_TILE;
                    // stage[mis + i] = s[base + i]: 16-byte aligned loads, the first / last line of the chunk byte-wise
                    const uint8_t* line0 = s + base - mis;
                    const uint32_t span = mis + nb;
                    for (uint32_t c = t * 16u; c < span; c += PNG_T * 16u) {
                        if (c >= mis && c + 16u <= span && (base != 0u || c >= 16u || mis == 0u)) {
                            *(uint4*)(stage + c) = *(const uint4*)(line0 + c);
                        } else {
                            for (uint32_t q = 0; q < 16u; ++q)
                                if (c + q >= mis && c + q < span) stage[c + q] = line0[c + q];
                        }
                    }
                    __syncthreads();
                    if (check_crc) {
                        const uint32_t b0 = t * 16u, b1 = b0 + 16u < nb ? b0 + 16u : nb;
                        uint32_t v = 0u;
                        if (b0 < nb) {
                            uint32_t i = b0;
                            for (; i + 4u <= b1; i += 4u) {
                                const uint32_t x = v ^ zmi_load32u(stage, mis + i);
                                v = tab[3][x & 0xFFu] ^ tab[2][(x >> 8) & 0xFFu] ^ tab[1][(x >> 16) & 0xFFu] ^ tab[0][x >> 24];
                            }
                            for (; i < b1; ++i) v = tab[0][(v ^ stage[mis + i]) & 0xFFu] ^ (v >> 8);
                            v = png_gf2_mulmod(v, nb == PNG_TILE ? kfull : png_gf2_xpow8(nb - b1));
                        }
#pragma unroll
                        for (int d = 32; d >= 1; d >>= 1) v ^= __shfl_xor(v, d);
                        if (zmi_lane() == 0) red[zmi_wave()] = v;
                        __syncthreads();
                        const uint32_t tile_crc = red[0] ^ red[1] ^ red[2] ^ red[3];
                        crc = png_gf2_mulmod(crc, nb == PNG_TILE ? ktile : png_gf2_xpow8(nb)) ^ tile_crc;
                    }
                    if (copy) {
                        const uint32_t skip = base == 0u ? 4u : 0u;   // the type's four bytes
                        if (nb > skip) {
                            const uint32_t m = nb - skip, so = mis + skip;
                            uint8_t* A = gdst + gpos + (base + skip - 4u);
                            uint32_t head = (4u - (uint32_t)((uintptr_t)A & 3u)) & 3u;
                            if (head > m) head = m;
                            const uint32_t ndw = (m - head) >> 2;
                            uint32_t* A4 = (uint32_t*)(A + head);
                            for (uint32_t q = t; q < ndw; q += PNG_T) A4[q] = zmi_load32u(stage, so + head + 4u * q);
                            if (t == 0) {
                                for (uint32_t q = 0; q < head; ++q) A[q] = stage[so + q];
                                for (uint32_t q = head + 4u * ndw; q < m; ++q) A[q] = stage[so + q];
                            }
                        }
                    }
                    __syncthreads();
                }
                if (check_crc && crit && t == 0u) {
                    const uint32_t got = crc ^ png_gf2_mulmod(0xFFFFFFFFu, png_gf2_xpow8(l)) ^ 0xFFFFFFFFu;
                    if (got != png_be32(f + pos + 8u + len)) atomicOr(&fl[j], PNG_FL_CRC);
                }
            }
            ++idx;
        }
        if (copy) gpos += len;
        if (type == PNG_IEND) break;
        pos += 12u + len;
    }
}

// ---- the unfilter (section 9.2) ---------------------------------------------------------------------------------------------------------
// x[r][i] = f[r][i] + pred_t(a, b, c) mod 256 with a = x[r][i - bpp], b = x[r - 1][i], c = x[r - 1][i - bpp], 0 outside the image, the
// filter type t per row.  Avg and Paeth are a serial chain along a row AND depend on the row above; the parallelism is
//   across images and across CHAINS of rows: a row of type None or Sub does not read the row above, so a chain may begin there.  The
//     work item is (slot, band b of 64 rows): it owns the chain that begins at the first such row inside its band (band 0: at row 0)
//     and runs it to the first such row of a later band -- so a chain is never shorter than what is left of its band, and an image
//     written with adaptive filters spreads over up to height / 64 waves.  An item whose band holds no such row has nothing to do.  No
//     table of chains is kept: every item reads the filter bytes of the bands it looks at (a strided byte per row, 64 rows per load);
//   inside a chain across 64 rows at a time by a skewed wavefront: lane k owns row r0 + k and runs k pixels behind lane k - 1.  Every
//     step a lane finishes one pixel of bpp bytes, kept packed in two registers: a is its own previous pixel, b the previous output of
//     the lane below -- moved up with zmi_lane_up1, one DPP move per register -- and c the b of the step before.  No lane waits on memory
//     for a neighbour.  Lane 0 reads b from the row above the band: the last row of the band before, re-read from the output.
// Memory: the skew makes direct global access uncoalesced (lane k reads at a stride of 1 + row_bytes), so the band goes through LDS in
// strips of PNG_STRIP bytes of the scanline: every row of the strip is loaded with aligned dwords side by side (its LDS place keeps
// the row's misalignment, so no byte is shuffled), unfiltered in place, and stored with aligned dwords where the output's alignment
// allows (zmi_load32u from LDS) and byte-wise at the edges.  A strip is drained before the next begins (the skew costs 63 steps per
// strip: a strip holds 512 / bpp pixels); a, b and c live on in the registers across strips.  One wave per workgroup, 34 KiB of LDS:
// four waves per CU by LDS.  NATIVE16 swaps the bytes of every sample where the pixel is written into LDS.
// Bounds: reads of the scanlines are whole dwords around [row, row + n): up to 3 bytes in front of and behind a row's strip, inside the
// scratch buffer the caller pads by 16 bytes on either side.  Stores write the region's own bytes only.
// One byte.  The filter type differs from lane to lane, so it arrives as masks made once per band -- sel = mA | mB << 8 | mP << 16 |
// shift << 24 with mA / mB = 0xFF where a / b enter the linear predictor (a + b) >> shift, mP = 0xFF for Paeth -- and nothing here
// branches (written as a chain of selects on the type, the compiler made five divergent branches per byte of it)
static __device__ __forceinline__ uint32_t png_filter_sel(uint32_t ft) {
    const uint32_t mA = (ft == 1u || ft == 3u) ? 0xFFu : 0u, mB = (ft == 2u || ft == 3u) ? 0xFFu : 0u;
    return mA | mB << 8 | (ft == 4u ? 0xFFu : 0u) << 16 | (ft == 3u ? 1u : 0u) << 24;
}
static __device__ __forceinline__ uint32_t png_unfilter_byte(uint32_t sel, uint32_t f, uint32_t a, uint32_t b, uint32_t c) {
    const int pa0 = (int)b - (int)c, pb0 = (int)a - (int)c;
    const uint32_t pa = (uint32_t)(pa0 < 0 ? -pa0 : pa0), pb = (uint32_t)(pb0 < 0 ? -pb0 : pb0);
    const int pc0 = pa0 + pb0;
    const uint32_t pc = (uint32_t)(pc0 < 0 ? -pc0 : pc0);
    const uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const uint32_t lin = ((a & sel) + (b & (sel >> 8))) >> (sel >> 24);
    const uint32_t mP = (sel >> 16) & 0xFFu;
    return (f + ((paeth & mP) | (lin & ~mP))) & 0xFFu;
}

// One strip of one band, bpp a compile-time constant (the byte loops unroll, every shift is a constant, a pixel of up to four bytes
// lives in one register): lane k runs k pixels behind lane k - 1; see the kernel below.  a, c and po live on across strips.
template <uint32_t BPP>
static __device__ __forceinline__ void png_strip_steps(uint8_t* tile, const uint8_t* prev, uint32_t mybase, uint32_t npx, uint32_t nrows,
                                                       uint32_t lane, bool valid, bool above, uint32_t sel, bool sw, uint64_t& a_io, uint64_t& c_io,
                                                       uint64_t& po_io) {
    typedef typename std::conditional<(BPP > 4u), uint64_t, uint32_t>::type px_t;
    px_t a = (px_t)a_io, c = (px_t)c_io, po = (px_t)po_io;
    const uint32_t steps = npx + nrows - 1u;
    // the filtered bytes of a step (and lane 0's row above) are read one step ahead: their LDS latency hides behind the arithmetic
    // of the step before
    px_t fnext = 0, pnext = 0;
    if (valid && lane == 0u) {
#pragma unroll
        for (uint32_t q = 0u; q < BPP; ++q) fnext |= (px_t)tile[mybase + q] << (8u * q);
        if (above) {
#pragma unroll
            for (uint32_t q = 0u; q < BPP; ++q) pnext |= (px_t)prev[q] << (8u * q);
        }
    }
    for (uint32_t t = 0u; t < steps; ++t) {
        px_t up = (px_t)zmi_lane_up1((uint32_t)po);
        if (BPP > 4u) up |= (px_t)((uint64_t)zmi_lane_up1((uint32_t)((uint64_t)po >> 32)) << 32);
        const uint32_t p = t - lane;
        const bool act = valid && t >= lane && p < npx;
        const px_t fv = fnext, pv = pnext;
        if (valid && t + 1u >= lane && p + 1u < npx) {
            const uint32_t at = mybase + (p + 1u) * BPP;
            px_t f2 = 0;
#pragma unroll
            for (uint32_t q = 0u; q < BPP; ++q) f2 |= (px_t)tile[at + q] << (8u * q);
            fnext = f2;
            if (lane == 0u && above) {
                px_t p2 = 0;
#pragma unroll
                for (uint32_t q = 0u; q < BPP; ++q) p2 |= (px_t)prev[(p + 1u) * BPP + q] << (8u * q);
                pnext = p2;
            }
        }
        if (act) {
            const uint32_t at = mybase + p * BPP;
            const px_t b = lane == 0u ? pv : up;
            px_t x = 0;
#pragma unroll
            for (uint32_t q = 0u; q < BPP; ++q) {
                const uint32_t sh = 8u * q;
                const uint32_t xb = png_unfilter_byte(sel, (uint32_t)(fv >> sh) & 0xFFu, (uint32_t)(a >> sh) & 0xFFu, (uint32_t)(b >> sh) & 0xFFu,
                                                      (uint32_t)(c >> sh) & 0xFFu);
                x |= (px_t)xb << sh;
                tile[at + (sw ? (q ^ 1u) : q)] = (uint8_t)xb;
            }
            c = b; a = x; po = x;
        }
    }
    a_io = a; c_io = c; po_io = po;
}

// The dword of a strip's row that lane `lane` stages in its k-th load: 0 .. 127 by the first two, 65 .. 128 by the third -- dword 128,
// which only a misaligned row of 512 bytes has, goes to lane 63 and the other lanes load a dword of theirs again.  (With lane + 128
// only lane 0 ever made the third load; the compiler then turned it into a scalar load from a base it had folded a byte offset into,
// and the scalar unit drops the base's low bits: the row's last dword came from 4 bytes in front.)
static __device__ __forceinline__ uint32_t png_stage_dw(uint32_t lane, uint32_t k) { return k < 2u ? lane + 64u * k : lane + 65u; }
#define PNG_STAGE_ROWS 16u       // rows whose loads are in flight together while a strip is staged (3 dwords a lane and row)
__global__ void __launch_bounds__(64) zmi_png_unfilter_kernel(const zmi_png_image* __restrict__ img, const uint32_t* __restrict__ sel, uint32_t n_sel,
                                                              const uint64_t* __restrict__ item_off, const uint8_t* __restrict__ sbuf,
                                                              const uint64_t* __restrict__ soff, const uint32_t* __restrict__ ssz,
                                                              const uint32_t* __restrict__ slen, const int32_t* __restrict__ sst,
                                                              uint8_t* __restrict__ out, const uint64_t* __restrict__ out_off, uint32_t native16,
                                                              uint32_t split, uint32_t* __restrict__ fl) {
    ZMI_DYN_SMEM(smem);          // PNG_UNFILTER_LDS bytes: the strip (16 bytes of slack for zmi_load32u), then the row above the band
    constexpr uint32_t pitch = PNG_PITCH, strip = PNG_STRIP;
    uint8_t* tile = smem;
    uint8_t* prev = smem + PNG_ROWS * PNG_PITCH + 16u;
    const uint32_t lane = threadIdx.x;
    const uint64_t total = item_off[n_sel];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        // the slot whose items hold `it`
        uint32_t lo = 0u, hi = n_sel;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (item_off[mid] <= it) lo = mid; else hi = mid;
        }
        const uint32_t j = lo;
        const uint32_t band = (uint32_t)(it - item_off[j]);
        if (ssz[j] == 0u || sst[j] != 0 || slen[j] != ssz[j]) continue;   // not decoded, or the stream failed: the slot reports that
        const zmi_png_image e = img[sel ? sel[j] : j];
        const uint32_t H = e.height, rb = e.row_bytes, bpp = e.bpp;
        const uint64_t stride = 1ull + rb;
        const uint8_t* scan = sbuf + soff[j];
        uint8_t* dst = out + out_off[j];
        const bool sw = native16 != 0u && e.depth == 16u;
        // this band's filter bytes: the check, and where its chain begins
        uint32_t start;
        {
            const uint32_t r = band * PNG_ROWS + lane;
            const uint32_t ft = r < H ? scan[(uint64_t)r * stride] : 0u;
            const uint64_t bad = __ballot(ft > 4u);
            if (bad != 0ull && lane == 0u) atomicOr(&fl[j], PNG_FL_FILTER);
            const uint64_t begins = __ballot(r < H && ft <= 1u);
            if (band == 0u) start = 0u;
            else if (!split || begins == 0ull) continue;
            else start = band * PNG_ROWS + (uint32_t)__ffsll((unsigned long long)begins) - 1u;
        }
        uint32_t end = H;
        for (uint32_t b2 = band + 1u; (uint64_t)b2 * PNG_ROWS < H; ++b2) {
            const uint32_t r = b2 * PNG_ROWS + lane;
            const uint32_t ft = r < H ? scan[(uint64_t)r * stride] : 255u;
            const uint64_t begins = __ballot(split && ft <= 1u);
            if (begins != 0ull) { end = b2 * PNG_ROWS + (uint32_t)__ffsll((unsigned long long)begins) - 1u; break; }
        }
        const uint32_t strip_b = (strip / bpp) * bpp;
        for (uint32_t r0 = start; r0 < end; r0 += PNG_ROWS) {
            const uint32_t nrows = end - r0 < PNG_ROWS ? end - r0 : PNG_ROWS;
            const bool valid = lane < nrows;
            const uint32_t myrow = r0 + (valid ? lane : 0u);
            const uint8_t* my = scan + (uint64_t)myrow * stride;
            uint32_t ft = valid ? my[0] : 0u;
            if (ft > 4u) ft = 0u;
            const uint32_t fsel = png_filter_sel(ft);
            const bool above = r0 > start;      // lane 0 has a row above it inside the chain
            uint64_t a = 0ull, c = 0ull, po = 0ull;
            for (uint32_t c0 = 0u; c0 < rb; c0 += strip_b) {
                const uint32_t nB = rb - c0 < strip_b ? rb - c0 : strip_b;
                const uint32_t npx = nB / bpp;
                // stage the strip: row q at tile + q * pitch, keeping its misalignment.  A row is at most (3 + 512 + 3) / 4 = 129 dwords,
                // three a lane; the loads of PNG_STAGE_ROWS rows are issued before the first is waited for (one row at a time, every row
                // cost a trip to memory: 0.8 ms of a 256 x 256 band's 1.4 ms)
                for (uint32_t q0 = 0u; q0 < nrows; q0 += PNG_STAGE_ROWS) {
                    uint32_t v[PNG_STAGE_ROWS][3];
#pragma unroll
                    for (uint32_t i = 0u; i < PNG_STAGE_ROWS; ++i) {
                        const uint8_t* g = scan + (uint64_t)(r0 + q0 + i) * stride + 1u + c0;
                        const uint32_t mis = (uint32_t)((uintptr_t)g & 3u);
                        const uint32_t* g4 = (const uint32_t*)(g - mis);
                        const uint32_t ndw = q0 + i < nrows ? (mis + nB + 3u) >> 2 : 0u;
#pragma unroll
                        for (uint32_t k = 0u; k < 3u; ++k) v[i][k] = png_stage_dw(lane, k) < ndw ? g4[png_stage_dw(lane, k)] : 0u;
                    }
#pragma unroll
                    for (uint32_t i = 0u; i < PNG_STAGE_ROWS; ++i) {
                        const uint8_t* g = scan + (uint64_t)(r0 + q0 + i) * stride + 1u + c0;
                        const uint32_t ndw = q0 + i < nrows ? ((uint32_t)((uintptr_t)g & 3u) + nB + 3u) >> 2 : 0u;
                        uint32_t* t4 = (uint32_t*)(tile + (q0 + i) * pitch);
#pragma unroll
                        for (uint32_t k = 0u; k < 3u; ++k)
                            if (png_stage_dw(lane, k) < ndw) t4[png_stage_dw(lane, k)] = v[i][k];
                    }
                }
                if (above) {
                    const uint8_t* pr = dst + (uint64_t)(r0 - 1u) * rb + c0;
                    for (uint32_t i = lane; i < nB; i += 64u) prev[sw ? (i ^ 1u) : i] = pr[i];
                }
                zmi_wave_sync();
                const uint32_t mybase = lane * pitch + (uint32_t)((uintptr_t)(my + 1u + c0) & 3u);
                switch (bpp) {      // (wave-uniform: bpp is the image's)
                case 1u: png_strip_steps<1u>(tile, prev, mybase, npx, nrows, lane, valid, above, fsel, sw, a, c, po); break;
                case 2u: png_strip_steps<2u>(tile, prev, mybase, npx, nrows, lane, valid, above, fsel, sw, a, c, po); break;
                case 3u: png_strip_steps<3u>(tile, prev, mybase, npx, nrows, lane, valid, above, fsel, sw, a, c, po); break;
                case 4u: png_strip_steps<4u>(tile, prev, mybase, npx, nrows, lane, valid, above, fsel, sw, a, c, po); break;
                case 6u: png_strip_steps<6u>(tile, prev, mybase, npx, nrows, lane, valid, above, fsel, sw, a, c, po); break;
                default: png_strip_steps<8u>(tile, prev, mybase, npx, nrows, lane, valid, above, fsel, sw, a, c, po); break;
                }
                zmi_wave_sync();
                // store the strip: row q's nB bytes to dst + (r0 + q) * rb + c0
#pragma unroll 4
                for (uint32_t q = 0u; q < nrows; ++q) {
                    const uint8_t* g = scan + (uint64_t)(r0 + q) * stride + 1u + c0;
                    const uint32_t so = q * pitch + (uint32_t)((uintptr_t)g & 3u);
                    uint8_t* A = dst + (uint64_t)(r0 + q) * rb + c0;
                    uint32_t head = (4u - (uint32_t)((uintptr_t)A & 3u)) & 3u;
                    if (head > nB) head = nB;
                    const uint32_t ndw = (nB - head) >> 2;
                    uint32_t* A4 = (uint32_t*)(A + head);
                    for (uint32_t d = lane; d < ndw; d += 64u) A4[d] = zmi_load32u(tile, so + head + 4u * d);
                    if (lane < head) A[lane] = tile[so + lane];
                    const uint32_t tail = head + 4u * ndw + lane;
                    if (lane < 3u && tail < nB) A[tail] = tile[so + tail];
                }
                zmi_wave_sync();
            }
        }
    }
}

// One thread per slot, behind everything else: the slot's final words (include/zmi355.h states the order).
__global__ void __launch_bounds__(256) zmi_png_finish_kernel(const zmi_png_image* __restrict__ img, uint32_t n_images, const uint32_t* __restrict__ sel,
                                                             uint32_t n_sel, const uint32_t* __restrict__ in_len, const uint64_t* __restrict__ out_off,
                                                             uint64_t out_cap, const uint32_t* __restrict__ ssz, const uint32_t* __restrict__ slen,
                                                             const int32_t* __restrict__ sst, const uint32_t* __restrict__ fl,
                                                             uint32_t* __restrict__ out_len, int32_t* __restrict__ status, int32_t* __restrict__ detail) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    zmi_png_image e;
    uint32_t k, L;
    const uint32_t kind = png_slot_kind(img, n_images, sel, j, in_len, &e, &k, &L);
    int32_t st = 0, det = 0;
    uint32_t n = 0u;
    if (kind == 3u) st = PNG_E_ARG;
    else if (kind == 2u) { det = e.status; st = (det == ZMI_PE_INTERLACE || det == ZMI_PE_BIG) ? PNG_VERSION_ERROR : ZMI_DATA_ERROR; }
    else {
        n = e.height * e.row_bytes;
        const uint32_t f = fl[j];
        const int32_t ds = sst[j];
        if (out_off[j] + (uint64_t)n > out_cap) { st = ZMI_BUF_ERROR; det = ZMI_PE_OUT; }
        else if (f & PNG_FL_SCRATCH) { st = PNG_MEM_ERROR; det = ZMI_PE_SCRATCH; }
        else if (f & PNG_FL_CRC) { st = ZMI_DATA_ERROR; det = ZMI_PE_CRC; }
        else if (ds == ZMI_BUF_ERROR) { st = ZMI_DATA_ERROR; det = ZMI_PE_LENGTH; }   // the stream wants more input, or more room than the scanlines
        else if (ds != ZMI_OK) { st = ds == PNG_MEM_ERROR ? PNG_MEM_ERROR : ZMI_DATA_ERROR; det = ds == PNG_MEM_ERROR ? ZMI_PE_SCRATCH : ZMI_PE_DATA; }
        else if (slen[j] != ssz[j]) { st = ZMI_DATA_ERROR; det = ZMI_PE_LENGTH; }
        else if (f & PNG_FL_FILTER) { st = ZMI_DATA_ERROR; det = ZMI_PE_FILTER; }
    }
    status[j] = st;
    detail[j] = det;
    out_len[j] = st == 0 ? n : 0u;
}

extern "C" uint32_t zmi_png_strip(void) { return PNG_STRIP; }
extern "C" int zmi_launch_png_headers(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n, zmi_png_image* d_images,
                                      hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_png_headers_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_in, d_in_off, d_in_len, n, d_images);
    return 0;
}
extern "C" int zmi_launch_png_prep(const zmi_png_image* d_images, uint32_t n_images, const uint32_t* d_sel, uint32_t n_sel, const uint32_t* d_in_len,
                                   uint32_t pass, uint32_t* d_pix, const uint32_t* d_pcap, uint32_t* d_ssz, uint32_t* d_gsz, uint32_t* d_items,
                                   uint32_t* d_fl, hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_png_prep_kernel, dim3((n_sel + 255u) / 256u), dim3(256), 0, stream, d_images, n_images, d_sel, n_sel, d_in_len, pass, d_pix, d_pcap,
               d_ssz, d_gsz, d_items, d_fl);
    return 0;
}
extern "C" int zmi_launch_png_walk(const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, const zmi_png_image* d_images,
                                   const uint32_t* d_sel, uint32_t n_sel, const uint32_t* d_ssz, const uint32_t* d_gsz, const uint64_t* d_goff,
                                   const uint32_t* d_gcap, uint8_t* d_gbuf, uint32_t check_crc, uint64_t* d_zin_off, uint32_t* d_zin_len,
                                   uint32_t* d_fl, hipStream_t stream) {
    if (n_sel == 0) return 0;
    // the chunks of a slot are dealt to K workgroups; a large batch fills the chip without that
    uint32_t K = 1u;
    while (K < PNG_WALK_K && (uint64_t)n_sel * K < 2048u) K <<= 1;
    ZMI_LAUNCH(zmi_png_walk_kernel, dim3(n_sel * K), dim3(PNG_T), 0, stream, d_in, d_in_off, d_in_len, d_images, d_sel, d_ssz, d_gsz, d_goff, d_gcap,
               d_gbuf, check_crc, K, d_zin_off, d_zin_len, d_fl);
    return 0;
}
// `bound`: what the items -- a device word -- can sum to (one per 64 rows of every region that fits out_cap); the grid is that, or a
// few waves per CU that take the items in turn
extern "C" int zmi_launch_png_unfilter(const zmi_png_image* d_images, const uint32_t* d_sel, uint32_t n_sel, const uint64_t* d_item_off,
                                       uint64_t bound, const uint8_t* d_sbuf, const uint64_t* d_soff, const uint32_t* d_ssz, const uint32_t* d_slen,
                                       const int32_t* d_sst, uint8_t* d_out, const uint64_t* d_out_off, uint32_t native16, uint32_t split,
                                       uint32_t* d_fl, hipStream_t stream) {
    if (n_sel == 0 || bound == 0) return 0;
    const uint32_t grid = bound < 16384ull ? (uint32_t)bound : 16384u;
    ZMI_LAUNCH(zmi_png_unfilter_kernel, dim3(grid), dim3(64), PNG_UNFILTER_LDS, stream, d_images, d_sel, n_sel, d_item_off, d_sbuf, d_soff, d_ssz, d_slen, d_sst,
               d_out, d_out_off, native16, split, d_fl);
    return 0;
}
extern "C" int zmi_launch_png_finish(const zmi_png_image* d_images, uint32_t n_images, const uint32_t* d_sel, uint32_t n_sel, const uint32_t* d_in_len,
                                     const uint64_t* d_out_off, uint64_t out_cap, const uint32_t* d_ssz, const uint32_t* d_slen, const int32_t* d_sst,
                                     const uint32_t* d_fl, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_png_finish_kernel, dim3((n_sel + 255u) / 256u), dim3(256), 0, stream, d_images, n_images, d_sel, n_sel, d_in_len, d_out_off, out_cap,
               d_ssz, d_slen, d_sst, d_fl, d_out_len, d_status, d_detail);
    return 0;
}
