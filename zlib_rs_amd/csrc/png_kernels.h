// png_kernels.h -- reading PNG images (zmi_png_headers_dev / zmi_png_decode_dev, include/zmi355.h) and, in the second half of the
// file, writing them (zmi_png_encode_dev); included by pack.hip.
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

// ---- writing PNG images (zmi_png_encode_dev; every byte of the file: include/zmi355.h) -------------------------------
// An image's filtered scanlines go into context scratch, are cut into pieces of piece_bytes and join ONE piece table that the
// independent-piece encoder works through in launch groups, exactly as the entries of zmi_zip_write_dev do -- the piece table, the bitmap
// of chain mode 2 and the payload copies ARE that call's kernels (zmi_zip_pieces_kernel with a "name" of 13 bytes: the hole of 43 bytes
// in front of an image's first piece; zmi_zip_pack_kernel).  What is new:
//   zmi_png_wlayout_kernel   one thread per image: the checks, the scanline size, the piece count, the bands of rows
//   zmi_png_filter_kernel    the hot path, below
//   zmi_png_place_kernel     one group's places: a piece takes its hole, its payload and, where it ends an image, the tail of 20 bytes;
//                            the place behind an image's last piece is rounded up to out_align -- a scan over (size, ends) pairs
//   zmi_png_wfinish_kernel   one wave per image: signature, IHDR, IDAT length and type, zlib header in the hole; Adler-32, the IDAT
//                            CRC-32 and IEND in the tail; the image's words and its zmi_png_image
#define PW_HEAD 43u              // 8 signature + 25 IHDR chunk + 8 IDAT length and type + 2 zlib header
#define PW_TAIL 20u              // 4 Adler-32 + 4 IDAT CRC-32 + 12 IEND chunk
#define PW_ROWS 8u               // most rows of a band, the filter kernel's work item
#define PW_TILE 256u             // bytes of a scanline one trip of a wave covers: an aligned dword of the output per lane
#define PW_ADAPTIVE 5u

// rows of a band: about 8 KiB of scanlines, one row at least, PW_ROWS at most (a single 8192 x 8192 image is 8192 items, not 1024;
// a full band is never less than 16 bytes of scanlines, which bounds the items by the caller's scan_bytes)
static __device__ __forceinline__ uint32_t pw_band_rows(uint32_t rb) {
    const uint32_t r = 8192u / (rb + 1u);
    return r < 1u ? 1u : (r > PW_ROWS ? PW_ROWS : r);
}
struct pw_geom { uint32_t w, h, depth, colour, ch, bpp, rb, scan; };
// the four fields of record i that are read, checked (include/zmi355.h lists the rules); false: the image is ZMI_E_ARG
static __device__ __forceinline__ bool pw_geom_of(const zmi_png_image* __restrict__ img, const uint32_t* __restrict__ in_len, uint32_t i, pw_geom* g) {
    const uint32_t w = img[i].width, h = img[i].height, depth = img[i].depth, colour = img[i].colour;
    uint32_t ch = 0u;
    if (colour == 0u) ch = (depth == 1u || depth == 2u || depth == 4u || depth == 8u || depth == 16u) ? 1u : 0u;
    else if (colour == 2u || colour == 4u || colour == 6u) ch = (depth == 8u || depth == 16u) ? (colour == 2u ? 3u : (colour == 4u ? 2u : 4u)) : 0u;
    if (w == 0u || h == 0u || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu || ch == 0u) return false;
    const uint64_t rb = ((uint64_t)w * ch * depth + 7ull) >> 3;
    if (rb >= ZMI_PNG_SCAN_MAX) return false;
    const uint64_t scan = (1ull + rb) * h;
    if (scan > ZMI_PNG_SCAN_MAX || (uint64_t)in_len[i] != rb * h) return false;
    g->w = w; g->h = h; g->depth = depth; g->colour = colour; g->ch = ch;
    g->bpp = ch * depth >= 8u ? ch * depth / 8u : 1u;
    g->rb = (uint32_t)rb; g->scan = (uint32_t)scan;
    return true;
}

// per image: ssz = (1 + row_bytes) * height, npc = its pieces, bands = its items of the filter kernel -- all 0 for an image that fails
// the checks --, nlen = 13 (what zmi_zip_pieces_kernel adds to 30 for the hole).  *sum (zeroed by the caller) receives the sum of ssz, one
// atomic per wave, for the scan_bytes check.
__global__ void __launch_bounds__(256) zmi_png_wlayout_kernel(const zmi_png_image* __restrict__ img, const uint32_t* __restrict__ in_len, uint32_t n,
                                                              uint32_t piece_bytes, uint32_t* __restrict__ ssz, uint32_t* __restrict__ nlen,
                                                              uint32_t* __restrict__ npc, uint32_t* __restrict__ bands, unsigned long long* sum) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t s = 0u;                                     // (no early return: the wave's lanes meet in the shuffles below)
    if (i < n) {
        pw_geom g;
        const bool ok = pw_geom_of(img, in_len, i, &g);
        s = ok ? g.scan : 0u;
        ssz[i] = s;
        nlen[i] = PW_HEAD - 30u;
        npc[i] = ok ? (uint32_t)(((uint64_t)s + piece_bytes - 1u) / piece_bytes) : 0u;
        bands[i] = ok ? (g.h + pw_band_rows(g.rb) - 1u) / pw_band_rows(g.rb) : 0u;
    }
    unsigned long long w = s;
    for (uint32_t d = 1u; d < 64u; d <<= 1) w += __shfl_xor(w, (int)d);
    if ((threadIdx.x & 63u) == 0u && w) atomicAdd(sum, w);
}

// ---- the forward filter (section 9.2, the choice of 12.7) -------------------------------------------------------------------------------
// f[r][i] = x[r][i] - pred_t(a, b, c) mod 256 with a = x[r][i - bpp], b = x[r - 1][i], c = x[r - 1][i - bpp], 0 outside the image: every
// neighbour is a RAW byte, so nothing here is serial and the work is one read of the pixels and one write of 1 + row_bytes per row.
// The work item is (image, band of pw_band_rows rows), one wave each; the wave walks a row in trips of PW_TILE bytes.  A lane owns the four
// row bytes that make up ONE ALIGNED DWORD OF THE OUTPUT (1 + row_bytes shifts every row by one more, so the row offset x of a lane's
// bytes is 4 * k - (the row's misalignment in the scratch)): the store is one dword per lane whatever the alignments are, and only the
// first and last dword of a row are written byte-wise.  The four operands -- the row and the row above at x and at x - bpp -- are each
// two aligned dword loads joined by v_alignbyte (pw_ld4: the input stands at any alignment); neighbouring lanes and the a / c loads hit
// the lines the x / b loads brought in, the row above comes from L2 (the same wave read it one row earlier, a band's first row from the
// band in front).  bpp is therefore only a distance between two loads, not a shift inside registers, and the kernel needs no variant
// per bpp.  Bytes outside [0, row_bytes) read as 0 by a mask, which also gives a and c of the first pixel and row 0's b and c.
// NATIVE16 swaps the two bytes of every sample as they are loaded (where x is odd the sample pairs lie across a lane's four bytes: the
// load then takes the eight bytes around them).
// Adaptive choice: pass 1 computes all five filtered dwords of a trip with packed byte arithmetic (Paeth byte by byte, branch-free) and
// adds sum(min(v, 256 - v)) -- v_sad_u8 of v ^ 0x80 against 0x80 -- into five 64-bit counters per lane; a wave reduction gives the exact
// costs, the smallest type of least cost wins, and pass 2 recomputes that type alone and stores it (the row comes from L1 / L2 again: a
// row of 24 KiB is what one wave just read).  A fixed type runs pass 2 only.
// Bounds: loads are aligned dwords that hold at least one byte of the row itself; stores write the row's own 1 + row_bytes bytes.
#ifdef ZMI_EMU
static inline uint32_t pw_sad4(uint32_t a, uint32_t b) {
    uint32_t s = 0u;
    for (int i = 0; i < 4; ++i) { const int d = (int)((a >> (8 * i)) & 0xFFu) - (int)((b >> (8 * i)) & 0xFFu); s += (uint32_t)(d < 0 ? -d : d); }
    return s;
}
#else
static __device__ __forceinline__ uint32_t pw_sad4(uint32_t a, uint32_t b) { return __builtin_amdgcn_sad_u8(a, b, 0u); }
#endif
// the bytes q of a dword at row offset y with 0 <= y + q < rb, as a mask
static __device__ __forceinline__ uint32_t pw_mask(int32_t y, int32_t rb) {
    const int32_t lo = y < 0 ? -y : 0;
    int32_t hi = rb - y;
    if (hi > 4) hi = 4;
    if (lo >= 4 || hi <= lo) return 0u;
    return (0xFFFFFFFFu << (8 * lo)) & (0xFFFFFFFFu >> (8 * (4 - hi)));
}
static __device__ __forceinline__ uint32_t pw_swap16(uint32_t v) { return ((v & 0x00FF00FFu) << 8) | ((v >> 8) & 0x00FF00FFu); }
// row[y .. y + 4) as a little-endian dword, bytes outside [0, rb) as 0
// (IN: the caller knows [y - 8, y + 12) to lie inside the row -- no test, no mask)
template <bool IN>
static __device__ __forceinline__ uint32_t pw_ld4_raw(const uint8_t* row, int32_t y, int32_t rb) {
    const uint8_t* p = row + y;
    const uint32_t m = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = (const uint32_t*)(p - m);
    if (IN) return __builtin_amdgcn_alignbyte(q[1], q[0], m);
    const int32_t q0 = y - (int32_t)m;                   // the row offset of q's first byte
    uint32_t w0 = 0u, w1 = 0u;
    if (q0 + 3 >= 0 && q0 < rb) w0 = q[0];
    if (m != 0u && q0 + 7 >= 0 && q0 + 4 < rb) w1 = q[1];
    return __builtin_amdgcn_alignbyte(w1, w0, m) & pw_mask(y, rb);
}
template <bool IN>
static __device__ __forceinline__ uint32_t pw_ld4(const uint8_t* row, int32_t y, int32_t rb, bool sw) {
    if (!sw) return pw_ld4_raw<IN>(row, y, rb);
    if ((y & 1) == 0) return pw_swap16(pw_ld4_raw<IN>(row, y, rb));
    const int32_t y0 = y - 1;                            // (rb is even: a sample is inside the row or outside it as a whole)
    return __builtin_amdgcn_alignbyte(pw_swap16(pw_ld4_raw<IN>(row, y0 + 4, rb)), pw_swap16(pw_ld4_raw<IN>(row, y0, rb)), 1u);
}
// packed bytes: x - p mod 256, and the Average predictor floor((a + b) / 2) on the 9-bit sum
static __device__ __forceinline__ uint32_t pw_sub4(uint32_t x, uint32_t p) {
    return ((x | 0x80808080u) - (p & 0x7F7F7F7Fu)) ^ ((x ^ ~p) & 0x80808080u);
}
static __device__ __forceinline__ uint32_t pw_avg4(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }
static __device__ __forceinline__ uint32_t pw_paeth4(uint32_t a4, uint32_t b4, uint32_t c4) {
    uint32_t r = 0u;
#pragma unroll
    for (uint32_t q = 0u; q < 4u; ++q) {
        const int a = (int)((a4 >> (8u * q)) & 0xFFu), b = (int)((b4 >> (8u * q)) & 0xFFu), c = (int)((c4 >> (8u * q)) & 0xFFu);
        const int pa0 = b - c, pb0 = a - c, pc0 = pa0 + pb0;
        const int pa = pa0 < 0 ? -pa0 : pa0, pb = pb0 < 0 ? -pb0 : pb0, pc = pc0 < 0 ? -pc0 : pc0;
        const int p = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        r |= (uint32_t)p << (8u * q);
    }
    return r;
}
// sum over the wave of a 64-bit value below 2^56, the same in every lane
static __device__ __forceinline__ uint64_t pw_wave_sum64(uint64_t v) {
    const uint64_t lo = zmi_wave_sum((uint32_t)(v & 0xFFFFFFull)), mid = zmi_wave_sum((uint32_t)((v >> 24) & 0xFFFFFFull));
    const uint64_t hi = zmi_wave_sum((uint32_t)(v >> 48));
    return lo + (mid << 24) + (hi << 48);
}

// one trip of pass 1: the five filtered dwords of this lane's bytes, their costs added to cost[]
template <bool IN>
static __device__ __forceinline__ void pw_trip_cost(const uint8_t* cur, const uint8_t* up, int32_t rb, int32_t bpp, int32_t x, bool sw, uint64_t* cost) {
    const uint32_t vm = IN ? 0xFFFFFFFFu : pw_mask(x, rb);
    const uint32_t x4 = pw_ld4<IN>(cur, x, rb, sw), a4 = pw_ld4<IN>(cur, x - bpp, rb, sw);
    const uint32_t b4 = up ? pw_ld4<IN>(up, x, rb, sw) : 0u, c4 = up ? pw_ld4<IN>(up, x - bpp, rb, sw) : 0u;
    const uint32_t f[5] = {x4, pw_sub4(x4, a4) & vm, pw_sub4(x4, b4) & vm, pw_sub4(x4, pw_avg4(a4, b4)) & vm, pw_sub4(x4, pw_paeth4(a4, b4, c4)) & vm};
#pragma unroll
    for (uint32_t k = 0u; k < 5u; ++k) cost[k] += pw_sad4(f[k] ^ 0x80808080u, 0x80808080u);
}
// one trip of pass 2: type t (the same in every lane) alone, stored
template <bool IN>
static __device__ __forceinline__ void pw_trip_store(const uint8_t* cur, const uint8_t* up, int32_t rb, int32_t bpp, int32_t x, bool sw, uint32_t t,
                                                     uint8_t* dst) {
    const uint32_t vm = IN ? 0xFFFFFFFFu : pw_mask(x, rb);
    if (vm == 0u) return;
    const uint32_t x4 = pw_ld4<IN>(cur, x, rb, sw);
    uint32_t p4 = 0u;
    if (t == 1u) p4 = pw_ld4<IN>(cur, x - bpp, rb, sw);
    else if (t == 2u) p4 = up ? pw_ld4<IN>(up, x, rb, sw) : 0u;
    else if (t >= 3u) {
        const uint32_t a4 = pw_ld4<IN>(cur, x - bpp, rb, sw);
        const uint32_t b4 = up ? pw_ld4<IN>(up, x, rb, sw) : 0u, c4 = up ? pw_ld4<IN>(up, x - bpp, rb, sw) : 0u;
        p4 = t == 3u ? pw_avg4(a4, b4) : pw_paeth4(a4, b4, c4);
    }
    const uint32_t f4 = pw_sub4(x4, p4);
    uint8_t* o = dst + 1 + x;
    if (vm == 0xFFFFFFFFu) *(uint32_t*)o = f4;
    else {
#pragma unroll
        for (uint32_t q = 0u; q < 4u; ++q)
            if ((vm >> (8u * q)) & 0xFFu) o[q] = (uint8_t)(f4 >> (8u * q));
    }
}

// one row: cur its rb bytes, up the row above (NULL: row 0), dst its 1 + rb bytes in the scratch.  A trip whose 256 bytes lie eight
// bytes and a pixel clear of both ends of the row (wave-uniform) needs no bounds test and no mask: all but the first and last of a row
static __device__ __forceinline__ void pw_filter_row(const uint8_t* cur, const uint8_t* up, int32_t rb, int32_t bpp, uint8_t* dst, uint32_t filter,
                                                     bool sw, uint32_t lane) {
    const int32_t md = (int32_t)((uintptr_t)(dst + 1) & 3u);
    uint32_t t = filter;
    if (filter == PW_ADAPTIVE) {
        uint64_t cost[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
        for (int32_t x0 = -md; x0 < rb; x0 += (int32_t)PW_TILE) {
            const int32_t x = x0 + 4 * (int32_t)lane;
            if (x0 - bpp >= 8 && x0 + (int32_t)PW_TILE + 8 <= rb) pw_trip_cost<true>(cur, up, rb, bpp, x, sw, cost);
            else pw_trip_cost<false>(cur, up, rb, bpp, x, sw, cost);
        }
        uint64_t best = 0ull;
        t = 0u;
#pragma unroll
        for (uint32_t k = 0u; k < 5u; ++k) {
            const uint64_t ck = pw_wave_sum64(cost[k]);
            if (k == 0u || ck < best) { best = ck; t = k; }
        }
    }
    for (int32_t x0 = -md; x0 < rb; x0 += (int32_t)PW_TILE) {
        const int32_t x = x0 + 4 * (int32_t)lane;
        if (x0 - bpp >= 8 && x0 + (int32_t)PW_TILE + 8 <= rb) pw_trip_store<true>(cur, up, rb, bpp, x, sw, t, dst);
        else pw_trip_store<false>(cur, up, rb, bpp, x, sw, t, dst);
    }
    if (lane == 0u) dst[0] = (uint8_t)t;
}

// *sum > scan_bytes: the scratch may not hold the scanlines, nothing is filtered (the pieces kernel voids the table for the same reason)
__global__ void __launch_bounds__(64) zmi_png_filter_kernel(const zmi_png_image* __restrict__ img, const uint8_t* __restrict__ in,
                                                            const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_len, uint32_t n,
                                                            const uint64_t* __restrict__ item_off, const unsigned long long* __restrict__ sum,
                                                            uint64_t scan_bytes, uint8_t* __restrict__ scan, const uint64_t* __restrict__ soff,
                                                            uint32_t filter, uint32_t native16) {
    if (*sum > scan_bytes) return;
    const uint32_t lane = threadIdx.x;
    const uint64_t total = item_off[n];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        uint32_t lo = 0u, hi = n;                       // the image whose items hold `it`
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (item_off[mid] <= it) lo = mid; else hi = mid;
        }
        pw_geom g;
        if (!pw_geom_of(img, in_len, lo, &g)) continue;  // (an image without items is never found: this cannot happen)
        const uint32_t band = (uint32_t)(it - item_off[lo]);
        const uint32_t rows = pw_band_rows(g.rb), r0 = band * rows, r1 = g.h - r0 < rows ? g.h : r0 + rows;
        const uint8_t* src = in + in_off[lo];
        uint8_t* dst = scan + soff[lo];
        const bool sw = native16 != 0u && g.depth == 16u;
        for (uint32_t r = r0; r < r1; ++r) {
            const uint8_t* cur = src + (uint64_t)r * g.rb;
            pw_filter_row(cur, r ? cur - g.rb : nullptr, (int32_t)g.rb, (int32_t)g.bpp, dst + (uint64_t)r * (1ull + g.rb), filter, sw, lane);
        }
    }
}

// One launch group's places, one workgroup.  Piece i of the group takes size_i = its hole + its payload (+ PW_TAIL where its bit in
// `ends` says that it ends an image), nothing for a void place; behind a piece that ends an image the running place is rounded up to
// align.  pos[0] holds where the group starts (the word the group before left, read before anything is written), pos[i] receives
// piece i's place and pos[n] where the group ends.  "p -> p + s, then round" composes: a run of pieces with at least one end is
// p -> roundup(p + a) + b, one without is p -> p + a, so the run of every thread is folded first and the 1024 folds are scanned.
struct pw_run { uint64_t a, b; uint32_t r; };
static __device__ __forceinline__ pw_run pw_then(pw_run f, pw_run g, uint64_t am) {   // f first, then g; am = align - 1
    pw_run o;
    if (!f.r) { o.a = f.a + g.a; o.r = g.r; o.b = g.r ? g.b : 0ull; return o; }
    o.a = f.a; o.r = 1u;
    o.b = g.r ? ((f.b + g.a + am) & ~am) + g.b : f.b + g.a;
    return o;
}
__global__ void __launch_bounds__(1024) zmi_png_place_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ olen,
                                                             const uint32_t* __restrict__ ends, uint32_t n, uint32_t align, uint64_t* pos) {
    __shared__ uint64_t sa[1024], sb[1024];
    __shared__ uint32_t sr[1024];
    const uint32_t t = threadIdx.x;
    const uint64_t am = (uint64_t)align - 1u;
    const uint64_t base = pos[0];
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    pw_run mine = {0ull, 0ull, 0u};
    for (uint32_t i = lo; i < hi; ++i) {
        const bool e = (ends[i >> 5] >> (i & 31u)) & 1u;
        const uint32_t h = head[i];
        const pw_run one = {h == 0xFFFFFFFFu ? 0ull : (uint64_t)h + olen[i] + (e ? PW_TAIL : 0u), 0ull, e ? 1u : 0u};
        mine = pw_then(mine, one, am);
    }
    sa[t] = mine.a; sb[t] = mine.b; sr[t] = mine.r;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
        pw_run f = {0ull, 0ull, 0u};
        if (t >= d) { f.a = sa[t - d]; f.b = sb[t - d]; f.r = sr[t - d]; }
        __syncthreads();
        if (t >= d) {
            pw_run g = {sa[t], sb[t], sr[t]};
            g = pw_then(f, g, am);
            sa[t] = g.a; sb[t] = g.b; sr[t] = g.r;
        }
        __syncthreads();
    }
    uint64_t p = base;
    if (t > 0u) p = sr[t - 1u] ? ((base + sa[t - 1u] + am) & ~am) + sb[t - 1u] : base + sa[t - 1u];
    for (uint32_t i = lo; i < hi; ++i) {
        const bool e = (ends[i >> 5] >> (i & 31u)) & 1u;
        const uint32_t h = head[i];
        pos[i] = p;
        p += h == 0xFFFFFFFFu ? 0ull : (uint64_t)h + olen[i] + (e ? PW_TAIL : 0u);
        if (e) p = (p + am) & ~am;
    }
    if (t == 1023u) pos[n] = p;
}

static __device__ __forceinline__ uint32_t pw_crc_byte(uint32_t c, uint32_t b) {
    c ^= b;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? PNG_CRC_POLY : 0u);
    return c;
}
// the CRC-32 of A | B from those of A and B (B of l2 bytes)
static __device__ __forceinline__ uint32_t pw_crc_join(uint32_t c1, uint32_t c2, uint64_t l2) { return png_gf2_mulmod(c1, png_gf2_xpow8(l2)) ^ c2; }
static __device__ __forceinline__ uint8_t pw_byte(const uint64_t* w, uint32_t k) { return (uint8_t)(w[k >> 3] >> (8u * (k & 7u))); }
static __device__ __forceinline__ void pw_put(uint64_t* w, uint32_t k, uint32_t b) { w[k >> 3] |= (uint64_t)(b & 0xFFu) << (8u * (k & 7u)); }
static __device__ __forceinline__ void pw_put_be32(uint64_t* w, uint32_t k, uint32_t v) {
    pw_put(w, k, v >> 24); pw_put(w, k + 1u, v >> 16); pw_put(w, k + 2u, v >> 8); pw_put(w, k + 3u, v);
}

// One wave per image, behind the last group.  *n_eff = 0: the scan_bytes check failed, every image is ZMI_E_ARG at offset 0.  Otherwise
// an image that failed the checks is ZMI_E_ARG where the images in front end; a good one sums its pieces' payloads (64 bits) and takes
// their first encoder status, and is written where it ends at or before out_cap: the lanes share the 43 + 20 bytes, every lane having
// computed the same words.  crc / adler: the folds per image of the pieces' CRC-32 (of the payload) and Adler-32 (of the scanlines).
__global__ void __launch_bounds__(256) zmi_png_wfinish_kernel(const zmi_png_image* __restrict__ img, const uint32_t* __restrict__ in_len, uint32_t n,
                                                              const uint32_t* __restrict__ n_eff, const uint64_t* __restrict__ first,
                                                              const uint64_t* __restrict__ pos, const uint32_t* __restrict__ olen,
                                                              const int32_t* __restrict__ st, const uint32_t* __restrict__ adler,
                                                              const uint32_t* __restrict__ crc, uint32_t level, uint32_t strategy,
                                                              uint8_t* __restrict__ out, uint64_t out_cap, uint64_t* __restrict__ out_off,
                                                              uint32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                              zmi_png_image* __restrict__ written) {
    const uint32_t lane = zmi_lane();
    const uint32_t i = blockIdx.x * 4u + zmi_wave();
    if (i >= n) return;                                  // (the whole wave)
    const bool bad = *n_eff == 0u;
    if (i == 0u && lane == 0u) out_off[n] = bad ? 0ull : pos[first[n]];
    pw_geom g = {};
    const bool ok = !bad && pw_geom_of(img, in_len, i, &g);
    zmi_png_image rec;
    rec.width = rec.height = 0u; rec.depth = rec.colour = rec.channels = rec.bpp = 0; rec.row_bytes = 0u; rec.idat_pos = rec.n_idat = rec.idat_bytes = 0u;
    rec.plte_pos = rec.plte_len = rec.trns_pos = rec.trns_len = 0u; rec.status = PNG_E_ARG;
    if (!ok) {
        if (lane == 0u) {
            out_off[i] = bad ? 0ull : pos[first[i]];
            out_len[i] = 0u;
            status[i] = PNG_E_ARG;
            if (written) written[i] = rec;
        }
        return;
    }
    const uint64_t p0 = first[i], p1 = first[i + 1u];
    uint64_t cl = 0ull;
    int32_t es = 0;
    for (uint64_t p = p0 + lane; p < p1; p += 64u) {
        cl += olen[p];
        if (es == 0) es = st[p];
    }
    const uint64_t clen = pw_wave_sum64(cl);
    const uint64_t failed = __ballot(es != 0);
    if (failed) es = __shfl(es, __ffsll((unsigned long long)failed) - 1);
    const uint64_t at = pos[p0], flen = PW_HEAD + clen + PW_TAIL;
    int32_t s = 0;
    if (es != 0) s = es;
    else if (clen + 6ull > 0x7FFFFFFFull) s = PNG_E_ARG;
    else if (at + flen > out_cap) s = ZMI_BUF_ERROR;
    if (lane == 0u) {
        out_off[i] = at;
        out_len[i] = s == 0 ? (uint32_t)flen : 0u;
        status[i] = s;
        if (written) {
            if (s == 0) {
                rec.width = g.w; rec.height = g.h; rec.depth = (uint8_t)g.depth; rec.colour = (uint8_t)g.colour; rec.channels = (uint8_t)g.ch;
                rec.bpp = (uint8_t)g.bpp; rec.row_bytes = g.rb; rec.idat_pos = 33u; rec.n_idat = 1u; rec.idat_bytes = (uint32_t)clen + 6u;
            }
            rec.status = s;
            written[i] = rec;
        }
    }
    if (s != 0) return;
    uint8_t zh[10];
    zmi_stream_header(1u, level, strategy, zh);
    uint64_t hw[6] = {0x0A1A0A0D474E5089ull, 0ull, 0ull, 0ull, 0ull, 0ull}, tw[3] = {0ull, 0ull, 0ull};
    pw_put_be32(hw, 8u, 13u);
    pw_put_be32(hw, 12u, PNG_IHDR);
    pw_put_be32(hw, 16u, g.w);
    pw_put_be32(hw, 20u, g.h);
    pw_put(hw, 24u, g.depth);
    pw_put(hw, 25u, g.colour);
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t k = 12u; k < 29u; ++k) c = pw_crc_byte(c, pw_byte(hw, k));
    pw_put_be32(hw, 29u, ~c);
    pw_put_be32(hw, 33u, (uint32_t)clen + 6u);
    pw_put_be32(hw, 37u, PNG_IDAT);
    pw_put(hw, 41u, zh[0]);
    pw_put(hw, 42u, zh[1]);
    const uint32_t ad = adler[i];
    pw_put_be32(tw, 0u, ad);
    c = 0xFFFFFFFFu;
    for (uint32_t k = 37u; k < 43u; ++k) c = pw_crc_byte(c, pw_byte(hw, k));
    uint32_t ic = pw_crc_join(~c, crc[i], clen);
    c = 0xFFFFFFFFu;
    for (uint32_t k = 0u; k < 4u; ++k) c = pw_crc_byte(c, pw_byte(tw, k));
    ic = pw_crc_join(ic, ~c, 4ull);
    pw_put_be32(tw, 4u, ic);
    pw_put_be32(tw, 12u, PNG_IEND);
    pw_put_be32(tw, 16u, 0xAE426082u);
    if (lane < PW_HEAD) out[at + lane] = pw_byte(hw, lane);
    if (lane < PW_TAIL) out[at + PW_HEAD + clen + lane] = pw_byte(tw, lane);
}

extern "C" uint32_t zmi_png_filter_tile(void) { return PW_TILE; }
extern "C" int zmi_launch_png_wlayout(const zmi_png_image* d_images, const uint32_t* d_in_len, uint32_t n, uint32_t piece_bytes, uint32_t* d_ssz,
                                      uint32_t* d_nlen, uint32_t* d_npc, uint32_t* d_bands, uint64_t* d_sum, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_png_wlayout_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, d_images, d_in_len, n, piece_bytes, d_ssz, d_nlen, d_npc, d_bands,
               (unsigned long long*)d_sum);
    return 0;
}
// The items are a device word; a full band is at least 2 * PW_ROWS bytes of scan_bytes, so they are at most n + scan_bytes / 16.  The grid
// is that, or a few waves per SIMD that take the items in turn
extern "C" int zmi_launch_png_filter(const zmi_png_image* d_images, const uint8_t* d_in, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                     const uint64_t* d_item_off, const uint64_t* d_sum, uint64_t scan_bytes, uint8_t* d_scan,
                                     const uint64_t* d_soff, uint32_t filter, uint32_t native16, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t bound = (uint64_t)n + scan_bytes / (2u * PW_ROWS);
    const uint32_t grid = bound < 32768ull ? (uint32_t)bound : 32768u;
    ZMI_LAUNCH(zmi_png_filter_kernel, dim3(grid), dim3(64), 0, stream, d_images, d_in, d_in_off, d_in_len, n, d_item_off, (const unsigned long long*)d_sum,
               scan_bytes, d_scan, d_soff, filter, native16);
    return 0;
}
extern "C" int zmi_launch_png_place(const uint32_t* d_head, const uint32_t* d_olen, const uint32_t* d_ends, uint32_t n, uint32_t align, uint64_t* d_pos,
                                    hipStream_t stream) {
    ZMI_LAUNCH(zmi_png_place_kernel, dim3(1), dim3(1024), 0, stream, d_head, d_olen, d_ends, n, align, d_pos);
    return 0;
}
extern "C" int zmi_launch_png_wfinish(const zmi_png_image* d_images, const uint32_t* d_in_len, uint32_t n, const uint32_t* d_n_eff, const uint64_t* d_first,
                                      const uint64_t* d_pos, const uint32_t* d_olen, const int32_t* d_st, const uint32_t* d_adler, const uint32_t* d_crc,
                                      uint32_t level, uint32_t strategy, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, uint32_t* d_out_len,
                                      int32_t* d_status, zmi_png_image* d_written, hipStream_t stream) {
    if (n == 0) return 0;
    ZMI_LAUNCH(zmi_png_wfinish_kernel, dim3((n + 3u) / 4u), dim3(256), 0, stream, d_images, d_in_len, n, d_n_eff, d_first, d_pos, d_olen, d_st, d_adler,
               d_crc, level, strategy, d_out, out_cap, d_out_off, d_out_len, d_status, d_written);
    return 0;
}
