// tiff_kernels.h -- reading TIFF files with Deflate compression (zmi_tiff_directory_dev / zmi_tiff_read_dev, include/zmi355.h);
// included by pack.hip.
//
// The format is TIFF 6.0 (section 2: the header and the image file directories, IFDs; section 3 and 15: strips and tiles; section 14:
// the horizontal-differencing predictor), the Adobe Photoshop TIFF Technical Notes (Deflate, compression 8; 32946 is the older code of
// the same), Adobe Technical Note 3 (the floating-point predictor) and BigTIFF as libtiff reads it (magic 43, 64-bit offsets, 20-byte
// entries).  A page is cut into segments -- strips or tiles --, every segment is one zlib stream of its own, and the file holds the
// table of their offsets and byte counts: the input shape of the batch decoder.  The kernels:
//   zmi_tiff_chain_kernel      one lane follows the IFD chain (it is serial: an IFD ends with the offset of the next) and writes
//                              zmi_tiff_info and the positions of the first `cap` IFDs
//   zmi_tiff_pages_kernel      one thread per listed IFD reads its tags, in whatever order they stand, into a zmi_tiff_page
//   zmi_tiff_slots_kernel      pass 0: what every slot reads -- offset and byte count of its segment from the file's two arrays, in the
//                              file's byte order and the array's value type --, the decoded sizes for the plan; pass 1, behind the plan:
//                              the decoder's tables, the raw copies' lengths, the row groups of the unpredict
//   zmi_tiff_unpredict_kernel  the hot path, below
//   zmi_tiff_finish_kernel     the slots' final words
#pragma once
#include <type_traits>

static_assert(sizeof(zmi_tiff_page) == 72u && sizeof(zmi_tiff_info) == 40u, "the records of include/zmi355.h: 72 and 40 bytes");
#define TIFF_E_ARG (-103)
#define TIFF_VERSION_ERROR (-6)
#define TIFF_MEM_ERROR (-4)
#define TIFF_ROWS 8u             // rows of a segment one work item of the unpredict covers
#define TIFF_ROW_TILE 1024u      // bytes of a row one trip covers per wave: 64 lanes x 16 bytes (see the kernel for pixels that do not divide 16)
#define TIFF_TRIP_MAX 4096u      // the longest trip: 64 lanes x one pixel of 8 samples x 8 bytes
#define TIFF_LDS (TIFF_TRIP_MAX + 32u)
#define TIFF_FL_BOUNDS 1u
#define TIFF_FL_SPARSE 2u
#define TIFF_FL_RAWLEN 4u

// an unsigned value of nb bytes (1, 2, 4, 8) at any alignment, in the file's byte order
static __device__ __forceinline__ uint64_t tf_rd(const uint8_t* p, uint32_t nb, bool be) {
    uint64_t v = 0ull;
    for (uint32_t i = 0u; i < nb; ++i) v |= (uint64_t)p[i] << (8u * (be ? nb - 1u - i : i));
    return v;
}
// bytes of a value of TIFF type `type`: BYTE 1, SHORT 3, LONG 4, LONG8 16; 0 for every type the reader does not take a number from
static __device__ __forceinline__ uint32_t tf_type_bytes(uint32_t type) {
    return type == 1u ? 1u : (type == 3u ? 2u : (type == 4u ? 4u : (type == 16u ? 8u : 0u)));
}

__global__ void __launch_bounds__(64) zmi_tiff_chain_kernel(const uint8_t* __restrict__ in, uint64_t L, uint32_t cap, zmi_tiff_info* __restrict__ info,
                                                            uint64_t* __restrict__ ifd_pos) {
    if (threadIdx.x != 0u || blockIdx.x != 0u) return;
    zmi_tiff_info r;
    r.n_pages = r.n_listed = r.first_ifd = 0ull; r.big_endian = r.bigtiff = 0u; r.status = 0; r.detail = 0;
    bool ok = L >= 8ull;
    bool be = false, big = false;
    uint64_t first = 0ull;
    if (ok) {
        be = in[0] == 0x4Du && in[1] == 0x4Du;
        ok = be || (in[0] == 0x49u && in[1] == 0x49u);
    }
    if (ok) {
        const uint32_t magic = (uint32_t)tf_rd(in + 2, 2u, be);
        if (magic == 42u) first = tf_rd(in + 4, 4u, be);
        else if (magic == 43u && L >= 16ull && tf_rd(in + 4, 2u, be) == 8ull && tf_rd(in + 6, 2u, be) == 0ull) { big = true; first = tf_rd(in + 8, 8u, be); }
        else ok = false;
    }
    if (!ok) { r.status = ZMI_DATA_ERROR; r.detail = ZMI_TA_HEADER; *info = r; return; }
    r.big_endian = be ? 1u : 0u; r.bigtiff = big ? 1u : 0u; r.first_ifd = first;
    const uint64_t cs = big ? 8ull : 2ull, es = big ? 20ull : 12ull, os = big ? 8ull : 4ull, hdr = big ? 16ull : 8ull;
    uint64_t pos = first, idx = 0ull;
    bool bad = first == 0ull;
    while (!bad && pos != 0ull) {
        if (idx >= (uint64_t)ZMI_TIFF_PAGES_MAX) { bad = true; break; }
        if (pos < hdr || pos > L || L - pos < cs) { bad = true; break; }
        const uint64_t n = tf_rd(in + pos, (uint32_t)cs, be);
        if (n == 0ull || n > (L - pos - cs) / es) { bad = true; break; }
        const uint64_t end = pos + cs + n * es;
        if (L - end < os) { bad = true; break; }
        if (idx < (uint64_t)cap) ifd_pos[idx] = pos;
        ++idx;
        pos = tf_rd(in + end, (uint32_t)os, be);
    }
    r.n_pages = idx;
    r.n_listed = idx < (uint64_t)cap ? idx : (uint64_t)cap;
    if (bad) { r.status = ZMI_DATA_ERROR; r.detail = (int32_t)(ZMI_TA_CHAIN | (uint32_t)idx << 8); }
    *info = r;
}

// one directory entry of interest: its value type, its count and the file position of its value bytes (inline or not: one path reads
// them); ok = a type numbers are read from, a count of at least 1, the bytes inside the file
struct tf_ent {
    uint32_t type, tsize;
    uint64_t count, pos;
    bool present, ok;
};
static __device__ __forceinline__ uint64_t tf_ent_value(const uint8_t* in, const tf_ent& e, uint64_t i, bool be) {
    return tf_rd(in + e.pos + i * e.tsize, e.tsize, be);
}

__global__ void __launch_bounds__(64) zmi_tiff_pages_kernel(const uint8_t* __restrict__ in, uint64_t L, const zmi_tiff_info* __restrict__ info,
                                                            const uint64_t* __restrict__ ifd_pos, uint32_t cap, zmi_tiff_page* __restrict__ pages) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= cap || (uint64_t)i >= info->n_listed) return;
    const bool be = info->big_endian != 0u, big = info->bigtiff != 0u;
    const uint32_t cs = big ? 8u : 2u, es = big ? 20u : 12u, os = big ? 8u : 4u;
    const uint64_t at = ifd_pos[i];
    const uint64_t n = tf_rd(in + at, cs, be);
    // the tags read, by their place in `ent`
    const uint32_t tags[17] = {256u, 257u, 258u, 259u, 262u, 273u, 277u, 278u, 279u, 284u, 317u, 322u, 323u, 324u, 325u, 338u, 339u};
    enum { T_W, T_H, T_BITS, T_COMP, T_PHOTO, T_SOFF, T_SPP, T_RPS, T_SCNT, T_PLANAR, T_PRED, T_TW, T_TL, T_TOFF, T_TCNT, T_EXTRA, T_SFMT, T_N };
    tf_ent ent[T_N];
    for (uint32_t k = 0u; k < (uint32_t)T_N; ++k) { ent[k].type = ent[k].tsize = 0u; ent[k].count = ent[k].pos = 0ull; ent[k].present = ent[k].ok = false; }
    for (uint64_t q = 0ull; q < n; ++q) {
        const uint64_t ea = at + cs + q * es;
        const uint32_t tag = (uint32_t)tf_rd(in + ea, 2u, be);
        uint32_t k = 0u;
        while (k < (uint32_t)T_N && tags[k] != tag) ++k;
        if (k == (uint32_t)T_N || ent[k].present) continue;     // (a tag that stands twice: the first counts)
        tf_ent e;
        e.present = true;
        e.type = (uint32_t)tf_rd(in + ea + 2u, 2u, be);
        e.tsize = tf_type_bytes(e.type);
        e.count = tf_rd(in + ea + 4u, os, be);
        e.pos = 0ull;
        e.ok = e.tsize != 0u && e.count != 0ull && e.count <= L;
        if (k == (uint32_t)T_EXTRA) e.ok = e.count <= L;          // (338: the count only)
        else if (e.ok) {
            const uint64_t bytes = e.count * e.tsize;
            e.pos = bytes <= (uint64_t)os ? ea + 4u + os : tf_rd(in + ea + 4u + os, os, be);
            e.ok = e.pos <= L && bytes <= L - e.pos;
        }
        ent[k] = e;
    }
    zmi_tiff_page r;
    r.offsets_pos = r.counts_pos = 0ull;
    r.width = r.height = r.seg_w = r.seg_h = r.segs_across = r.segs_down = r.n_segs = r.seg_bytes = 0u;
    r.bits = 1u; r.samples = 1u; r.sample_format = 1u; r.predictor = 1u; r.compression = 1u; r.photometric = 0u; r.extra_samples = 0u;
    r.sample_bytes = 0u; r.big_endian = be ? 1u : 0u; r.bigtiff = big ? 1u : 0u; r.tiled = 0u; r.offsets_type = r.counts_type = 0u;
    r.status = 0;
    bool tags_bad = false, format_bad = false;
    // scalars: the first value, clamped to the field that keeps it
#define TF_SCALAR(K, DEF, MAX) (ent[K].present ? (ent[K].ok ? (tf_ent_value(in, ent[K], 0ull, be) > (uint64_t)(MAX) ? (uint64_t)(MAX) : tf_ent_value(in, ent[K], 0ull, be)) \
                                                            : (tags_bad = true, (uint64_t)(DEF))) : (uint64_t)(DEF))
    const uint64_t w = TF_SCALAR(T_W, 0u, 0xFFFFFFFFu), h = TF_SCALAR(T_H, 0u, 0xFFFFFFFFu);
    const uint64_t spp = TF_SCALAR(T_SPP, 1u, 0xFFFFu);
    const uint64_t comp = TF_SCALAR(T_COMP, 1u, 0xFFFFu), photo = TF_SCALAR(T_PHOTO, 0u, 0xFFFFu), planar = TF_SCALAR(T_PLANAR, 1u, 0xFFFFu);
    const uint64_t pred = TF_SCALAR(T_PRED, 1u, 0xFFFFu), sfmt = TF_SCALAR(T_SFMT, 1u, 0xFFFFu);
    const uint64_t rps = TF_SCALAR(T_RPS, 0xFFFFFFFFu, 0xFFFFFFFFu);
    const uint64_t tw = TF_SCALAR(T_TW, 0u, 0xFFFFFFFFu), tl = TF_SCALAR(T_TL, 0u, 0xFFFFFFFFu);
    uint64_t bits = 1ull;
    if (ent[T_BITS].present) {
        if (!ent[T_BITS].ok) tags_bad = true;
        else {
            bits = tf_ent_value(in, ent[T_BITS], 0ull, be);
            const uint64_t nv = ent[T_BITS].count < spp ? ent[T_BITS].count : spp;
            for (uint64_t q = 1ull; q < nv && q < 8ull; ++q)
                if (tf_ent_value(in, ent[T_BITS], q, be) != bits) format_bad = true;
            if (bits > 0xFFFFull) bits = 0xFFFFull;
        }
    }
#undef TF_SCALAR
    if (ent[T_EXTRA].present) { if (ent[T_EXTRA].ok) r.extra_samples = (uint16_t)(ent[T_EXTRA].count > 0xFFFFull ? 0xFFFFull : ent[T_EXTRA].count); else tags_bad = true; }
    r.width = (uint32_t)w; r.height = (uint32_t)h;
    r.bits = (uint16_t)bits; r.samples = (uint16_t)spp; r.sample_format = (uint16_t)sfmt; r.predictor = (uint16_t)pred;
    r.compression = (uint16_t)comp; r.photometric = (uint16_t)photo;
    if (!ent[T_W].present || !ent[T_H].present || w == 0ull || h == 0ull) tags_bad = true;
    const bool tile_any = ent[T_TW].present || ent[T_TL].present || ent[T_TOFF].present || ent[T_TCNT].present;
    const bool strip_any = ent[T_SOFF].present || ent[T_SCNT].present;
    if (tile_any == strip_any) tags_bad = true;
    else if (tile_any && !(ent[T_TW].present && ent[T_TL].present && ent[T_TOFF].present && ent[T_TCNT].present)) tags_bad = true;
    else if (strip_any && !(ent[T_SOFF].present && ent[T_SCNT].present)) tags_bad = true;
    r.tiled = tile_any && !strip_any ? 1u : 0u;
    const tf_ent& eo = ent[r.tiled ? T_TOFF : T_SOFF];
    const tf_ent& ec = ent[r.tiled ? T_TCNT : T_SCNT];
    uint64_t sw = r.tiled ? tw : w, sh = r.tiled ? tl : (rps < h ? rps : h);
    if (sw == 0ull || sh == 0ull) tags_bad = true;
    if (!tags_bad) {
        const uint64_t across = (w + sw - 1ull) / sw, down = (h + sh - 1ull) / sh;
        const uint64_t ns = across * down;
        r.seg_w = (uint32_t)sw; r.seg_h = (uint32_t)sh; r.segs_across = (uint32_t)across; r.segs_down = (uint32_t)down;
        r.n_segs = ns > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)ns;
        // the arrays: SHORT, LONG or LONG8, n_segs values each, inside the file
        if (!eo.ok || !ec.ok || eo.type == 1u || ec.type == 1u || eo.count != ns || ec.count != ns) tags_bad = true;
        else { r.offsets_pos = eo.pos; r.counts_pos = ec.pos; r.offsets_type = (uint8_t)eo.type; r.counts_type = (uint8_t)ec.type; }
    }
    const bool depth_ok = bits == 8ull || bits == 16ull || bits == 32ull || bits == 64ull;
    if (depth_ok) r.sample_bytes = (uint8_t)(bits / 8ull);
    if (!depth_ok || spp == 0ull || spp > 8ull || pred == 0ull || pred > 3ull || (pred == 3ull && (sfmt != 3ull || bits < 16ull))) format_bad = true;
    bool too_big = false;
    if (!tags_bad && !format_bad) {
        const uint64_t px = sw * sh;                                   // (both below 2^32: no overflow)
        const uint64_t sb = px > 0xFFFFFFFFull ? ~0ull : px * spp * (bits / 8ull);
        too_big = sb > 0xFFFFFFFFull;
        r.seg_bytes = too_big ? 0xFFFFFFFFu : (uint32_t)sb;
    }
    if (tags_bad) r.status = ZMI_TP_TAGS;
    else if (format_bad) r.status = ZMI_TP_FORMAT;
    else if (comp != 1ull && comp != 8ull && comp != 32946ull) r.status = ZMI_TP_COMPRESSION;
    else if (planar == 2ull) r.status = ZMI_TP_PLANAR;
    else if (too_big) r.status = ZMI_TP_BIG;
    pages[i] = r;
}

// What slot j reads, and where its pixels go.  kind: 0 a segment of a readable page, 2 a page the directory flagged, 3 nothing this
// call may touch (an index outside the page or the table, a record no directory call writes for a file of L bytes)
struct tf_slot {
    zmi_tiff_page p;
    uint32_t kind, seg;
    uint32_t rows;       // decoded rows of the segment (the last strip: the rows left) and dsz = their bytes
    uint32_t dsz, pb;    // pb = bytes of a pixel
    uint32_t ow, oh;     // pixels of a row and rows that are written: the segment's own, or cropped at the image's edges (assemble)
    uint64_t opitch;     // bytes from row to row where they are written
    uint64_t ooff;       // assemble: the offset of the segment's first pixel in the image
    uint64_t image;      // bytes of the whole page as one image
};
static __device__ __forceinline__ bool tf_page_ok(const zmi_tiff_page& p, uint64_t L) {
    const uint32_t sb = p.sample_bytes;
    if (!(sb == 1u || sb == 2u || sb == 4u || sb == 8u) || p.bits != 8u * sb || p.samples == 0u || p.samples > 8u) return false;
    if (p.width == 0u || p.height == 0u || p.seg_w == 0u || p.seg_h == 0u || p.predictor == 0u || p.predictor > 3u) return false;
    if (p.predictor == 3u && (sb < 2u || p.sample_format != 3u)) return false;
    if (p.compression != 1u && p.compression != 8u && p.compression != 32946u) return false;
    if (!p.tiled && (p.seg_w != p.width || p.seg_h > p.height)) return false;
    const uint64_t across = ((uint64_t)p.width + p.seg_w - 1ull) / p.seg_w, down = ((uint64_t)p.height + p.seg_h - 1ull) / p.seg_h;
    if (across != p.segs_across || down != p.segs_down || across * down != (uint64_t)p.n_segs) return false;
    const uint64_t px = (uint64_t)p.seg_w * p.seg_h;
    if (px > 0xFFFFFFFFull || px * p.samples * sb != (uint64_t)p.seg_bytes) return false;
    const uint32_t to = tf_type_bytes(p.offsets_type), tc = tf_type_bytes(p.counts_type);
    if (to < 2u || tc < 2u) return false;
    if (p.offsets_pos > L || (uint64_t)p.n_segs * to > L - p.offsets_pos) return false;
    if (p.counts_pos > L || (uint64_t)p.n_segs * tc > L - p.counts_pos) return false;
    return true;
}
static __device__ __forceinline__ void tf_slot_of(const zmi_tiff_page* __restrict__ pages, uint32_t n_pages, uint32_t page, const uint32_t* __restrict__ sel,
                                                  uint32_t j, uint64_t L, uint32_t assemble, tf_slot* s) {
    s->kind = 3u; s->seg = 0u; s->rows = s->dsz = s->pb = s->ow = s->oh = 0u; s->opitch = s->ooff = s->image = 0ull;
    if (page >= n_pages) return;
    s->p = pages[page];
    const zmi_tiff_page& p = s->p;
    if (p.status != 0) { if (p.status >= ZMI_TP_TAGS && p.status <= ZMI_TP_BIG) s->kind = 2u; return; }
    if (!tf_page_ok(p, L)) return;
    s->pb = (uint32_t)p.samples * p.sample_bytes;
    s->image = (uint64_t)p.width * p.height * s->pb;
    const uint32_t k = sel ? sel[j] : j;
    if (k >= p.n_segs) return;
    s->kind = 0u; s->seg = k;
    const uint32_t tx = k % p.segs_across, ty = k / p.segs_across;
    const uint32_t left_h = p.height - ty * p.seg_h, left_w = p.width - tx * p.seg_w;      // (both at least 1)
    s->rows = p.tiled ? p.seg_h : (left_h < p.seg_h ? left_h : p.seg_h);
    s->dsz = (uint32_t)((uint64_t)s->rows * p.seg_w * s->pb);
    if (assemble) {
        s->ow = left_w < p.seg_w ? left_w : p.seg_w;
        s->oh = left_h < p.seg_h ? left_h : p.seg_h;
        s->opitch = (uint64_t)p.width * s->pb;
        s->ooff = ((uint64_t)ty * p.seg_h * p.width + (uint64_t)tx * p.seg_w) * s->pb;
    } else {
        s->ow = p.seg_w; s->oh = s->rows;
        s->opitch = (uint64_t)p.seg_w * s->pb;
    }
}

// pass 0: pix[j] = the decoded size of a slot that reads a segment (else 0), zin_off[j] / zin_len[j] = the segment's offset and byte
// count as the file's arrays give them, fl[j] = TIFF_FL_BOUNDS / TIFF_FL_SPARSE; assemble: out_off and pcap too (dense: the plan makes
// them).  pass 1, behind the plan and the sum pix_off[n_sel] of the decoded sizes: ssz[j] = the decoded size of a slot whose bytes are
// fetched, zin_len[j] = the byte count handed to the decoder (deflated) and rawlen[j] = the bytes to copy (compression 1, a byte count
// of exactly the decoded size), items[j] = the row groups the unpredict writes -- all 0 under a decoded_bytes that is too small
__global__ void __launch_bounds__(256) zmi_tiff_slots_kernel(const uint8_t* __restrict__ in, uint64_t L, const zmi_tiff_page* __restrict__ pages,
                                                             uint32_t n_pages, uint32_t page, const uint32_t* __restrict__ sel, uint32_t n_sel,
                                                             uint32_t assemble, uint32_t pass, uint64_t out_cap, uint64_t decoded_bytes,
                                                             const uint64_t* __restrict__ pix_off, uint32_t* __restrict__ pix, uint32_t* __restrict__ pcap,
                                                             uint64_t* __restrict__ zin_off, uint32_t* __restrict__ zin_len, uint32_t* __restrict__ ssz,
                                                             uint32_t* __restrict__ rawlen, uint32_t* __restrict__ items, uint32_t* __restrict__ fl,
                                                             uint64_t* __restrict__ out_off) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    tf_slot s;
    tf_slot_of(pages, n_pages, page, sel, j, L, assemble, &s);
    if (pass == 0u) {
        uint64_t off = 0ull, cnt = 0ull;
        uint32_t f = 0u;
        if (s.kind == 0u) {
            const bool be = s.p.big_endian != 0u;
            const uint32_t to = tf_type_bytes(s.p.offsets_type), tc = tf_type_bytes(s.p.counts_type);
            off = tf_rd(in + s.p.offsets_pos + (uint64_t)s.seg * to, to, be);
            cnt = tf_rd(in + s.p.counts_pos + (uint64_t)s.seg * tc, tc, be);
            if (cnt == 0ull) f = TIFF_FL_SPARSE;
            else if (cnt > 0xFFFFFFFFull || off > L || cnt > L - off) f = TIFF_FL_BOUNDS;
        }
        pix[j] = s.kind == 0u ? s.dsz : 0u;
        zin_off[j] = f == 0u ? off : 0ull;
        zin_len[j] = f == 0u ? (uint32_t)cnt : 0u;
        fl[j] = f;
        if (assemble) {
            out_off[j] = s.ooff;
            pcap[j] = s.kind == 0u && s.image <= out_cap ? s.dsz : 0u;
            if (j == 0u) out_off[n_sel] = s.image;
        }
        return;
    }
    const bool over = pix_off[n_sel] > decoded_bytes;
    const uint32_t f = fl[j];
    const bool placed = s.kind == 0u && pcap[j] != 0u && !(f & TIFF_FL_BOUNDS) && !over;
    const bool live = placed && !(f & TIFF_FL_SPARSE);
    const bool raw = s.kind == 0u && s.p.compression == 1u;
    const uint32_t cnt = zin_len[j];
    ssz[j] = live ? s.dsz : 0u;
    zin_len[j] = live && !raw ? cnt : 0u;
    rawlen[j] = live && raw && cnt == s.dsz ? s.dsz : 0u;
    if (live && raw && cnt != s.dsz) fl[j] = f | TIFF_FL_RAWLEN;
    items[j] = placed ? (s.oh + TIFF_ROWS - 1u) / TIFF_ROWS : 0u;
}

// ---- the unpredict (TIFF 6.0 section 14, Technical Note 3) and the placement ---------------------------------------------------------------
// A row of a segment is N = seg_w * samples samples of s bytes.  Predictor 1 copies (and swaps the bytes of every sample of an MM file);
// predictor 2 is x[i] = d[i] + x[i - samples] mod 2^(8 s) on the samples read in the file's byte order, an inclusive scan per channel;
// predictor 3 is the same scan over the row's N * s BYTES with a stride of `samples` bytes, after which byte b of sample k -- b = 0 the
// most significant, in II and MM files alike -- stands at p[b * N + k].  Every sample leaves little-endian.  Rows are independent and
// short (a 256-pixel RGB row is 768 bytes), so the parallelism is rows: the work item is (slot, group of TIFF_ROWS rows), one wave a
// workgroup, the items numbered by a scan of the slots' group counts and taken in turn by a fixed grid (both counts are device values).
// One row: trips of 64 runs.  A lane's run is the whole pixels that fit 16 bytes (one pixel where it is longer), so the channel phase
// is the same in every lane and a trip covers 64 x that: TIFF_ROW_TILE = 1024 bytes for the pixel sizes that divide 16, a little less
// for the others (960 for 3 bytes, 768 for 6), 64 pixels for pixels above 16 bytes.  The trip is staged through LDS with aligned dword
// loads at a place that keeps the row's misalignment (no byte is shuffled; every load address depends on the lane -- a wave-uniform
// address may become a scalar load, which drops the low bits of a misaligned base).  Every lane adds up its run
// per channel, the per-lane totals go through an exclusive wave scan per channel (DPP; 64-bit samples: six lane moves), a per-channel
// carry runs from trip to trip, and the lane's second walk over its run writes the sums in place, little-endian.  The row leaves LDS
// with aligned dwords where the destination allows (zmi_load32u) and byte-wise at its edges; in assemble mode the destination pitch is
// the image's row and the run is cropped.  Predictor 3 runs the byte scan in place in the scratch (the planes of one sample lie N bytes
// apart: the whole row would have to stand in LDS, and a strip may be of any width) and then gathers: for a fixed plane consecutive
// lanes read consecutive bytes, and the samples are stored whole.
// Bounds: the staged dwords reach up to 3 bytes in front of and behind a row, inside the scratch the caller pads by 16 bytes on either
// side; stores write the row's own bytes only.
template <uint32_t S> struct tf_acc { typedef uint32_t type; };
template <> struct tf_acc<8u> { typedef uint64_t type; };
static __device__ __forceinline__ uint32_t tf_wave_scan(uint32_t v) { return zmi_wave_incl_scan(v); }
static __device__ __forceinline__ uint64_t tf_wave_scan(uint64_t v) {
    const uint32_t lane = zmi_lane();
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, d);
        if (lane >= d) v += t;
    }
    return v;
}
static __device__ __forceinline__ uint32_t tf_wave_last(uint32_t v) { return zmi_readlane(v, 63u); }
static __device__ __forceinline__ uint64_t tf_wave_last(uint64_t v) {
    return (uint64_t)zmi_readlane((uint32_t)v, 63u) | (uint64_t)zmi_readlane((uint32_t)(v >> 32), 63u) << 32;
}
template <uint32_t S>
static __device__ __forceinline__ typename tf_acc<S>::type tf_lds_rd(const uint8_t* p, bool be) {
    typename tf_acc<S>::type v = 0;
#pragma unroll
    for (uint32_t i = 0u; i < S; ++i) v |= (typename tf_acc<S>::type)p[i] << (8u * (be ? S - 1u - i : i));
    return v;
}
template <uint32_t S>
static __device__ __forceinline__ void tf_lds_wr(uint8_t* p, typename tf_acc<S>::type v) {
#pragma unroll
    for (uint32_t i = 0u; i < S; ++i) p[i] = (uint8_t)(v >> (8u * i));
}

// One row: n_src bytes at src (elements of S bytes in the file's byte order), the first n_dst of them stored at dst little-endian.
// st = the scan's stride in elements (the samples of a pixel), 0 = no scan.
template <uint32_t S>
static __device__ __forceinline__ void tf_scan_row(uint8_t* lds, const uint8_t* src, uint8_t* dst, uint32_t n_src, uint32_t n_dst, uint32_t st, bool be,
                                                   uint32_t lane) {
    typedef typename tf_acc<S>::type acc_t;
    const uint32_t pb = (st ? st : 1u) * S;
    const uint32_t run = pb <= 16u ? (16u / pb) * pb : pb;
    const uint32_t trip = 64u * run;
    acc_t carry[8];
#pragma unroll
    for (uint32_t c = 0u; c < 8u; ++c) carry[c] = 0;
    uint32_t* lds4 = (uint32_t*)lds;
    for (uint32_t t0 = 0u; t0 < n_src; t0 += trip) {
        const uint32_t nb = n_src - t0 < trip ? n_src - t0 : trip;
        const uint8_t* g = src + t0;
        const uint32_t mis = (uint32_t)((uintptr_t)g & 3u);
        const uint32_t* g4 = (const uint32_t*)(g - mis);
        const uint32_t ndw = (mis + nb + 3u) >> 2;
        for (uint32_t d = lane; d < ndw; d += 64u) lds4[d] = g4[d];
        zmi_wave_sync();
        const uint32_t my0 = lane * run;
        const uint32_t myn = my0 < nb ? (nb - my0 < run ? nb - my0 : run) : 0u;
        uint8_t* mine = lds + mis + my0;
        if (st != 0u) {
            acc_t acc[8];
#pragma unroll
            for (uint32_t c = 0u; c < 8u; ++c) acc[c] = 0;
            for (uint32_t o = 0u; o < myn; o += pb) {
#pragma unroll
                for (uint32_t c = 0u; c < 8u; ++c)
                    if (c < st) acc[c] += tf_lds_rd<S>(mine + o + c * S, be);
            }
#pragma unroll
            for (uint32_t c = 0u; c < 8u; ++c) {
                if (c < st) {       // (wave-uniform: the page's samples)
                    const acc_t incl = tf_wave_scan(acc[c]);
                    acc[c] = incl - acc[c] + carry[c];
                    carry[c] += tf_wave_last(incl);
                }
            }
            for (uint32_t o = 0u; o < myn; o += pb) {
#pragma unroll
                for (uint32_t c = 0u; c < 8u; ++c) {
                    if (c < st) {
                        acc[c] += tf_lds_rd<S>(mine + o + c * S, be);
                        tf_lds_wr<S>(mine + o + c * S, acc[c]);
                    }
                }
            }
        } else if (be && S > 1u) {
            for (uint32_t o = 0u; o < myn; o += S) tf_lds_wr<S>(mine + o, tf_lds_rd<S>(mine + o, true));
        }
        zmi_wave_sync();
        if (t0 < n_dst) {
            const uint32_t m = n_dst - t0 < nb ? n_dst - t0 : nb;
            uint8_t* A = dst + t0;
            uint32_t head = (4u - (uint32_t)((uintptr_t)A & 3u)) & 3u;
            if (head > m) head = m;
            const uint32_t nd = (m - head) >> 2;
            uint32_t* A4 = (uint32_t*)(A + head);
            for (uint32_t d = lane; d < nd; d += 64u) A4[d] = zmi_load32u(lds, mis + head + 4u * d);
            if (lane < head) A[lane] = lds[mis + lane];
            const uint32_t tail = head + 4u * nd + lane;
            if (lane < 3u && tail < m) A[tail] = lds[mis + tail];
        }
        zmi_wave_sync();
    }
}

// Technical Note 3, behind the byte scan: sample k of the row = the bytes p[b * N + k], b = 0 the most significant
template <uint32_t S>
static __device__ __forceinline__ void tf_gather_row(const uint8_t* p, uint8_t* dst, uint32_t N, uint32_t n_out, uint32_t lane) {
    typedef typename tf_acc<S>::type acc_t;
    const bool whole = ((uintptr_t)dst & (uintptr_t)(S - 1u)) == 0u;
    for (uint32_t k = lane; k < n_out; k += 64u) {
        acc_t v = 0;
#pragma unroll
        for (uint32_t b = 0u; b < S; ++b) v = (acc_t)(v << 8) | (acc_t)p[(uint64_t)b * N + k];
        if (whole) {
            if (S == 2u) *(uint16_t*)(dst + (uint64_t)k * S) = (uint16_t)v;
            else if (S == 4u) *(uint32_t*)(dst + (uint64_t)k * S) = (uint32_t)v;
            else *(uint64_t*)(dst + (uint64_t)k * S) = (uint64_t)v;
        } else {
            tf_lds_wr<S>(dst + (uint64_t)k * S, v);
        }
    }
}

__global__ void __launch_bounds__(64) zmi_tiff_unpredict_kernel(const zmi_tiff_page* __restrict__ pages, uint32_t n_pages, uint32_t page,
                                                                const uint32_t* __restrict__ sel, uint32_t n_sel, uint64_t L, uint32_t assemble,
                                                                const uint64_t* __restrict__ item_off, uint8_t* sbuf, const uint64_t* __restrict__ soff,
                                                                const uint32_t* __restrict__ ssz, const uint32_t* __restrict__ slen,
                                                                const int32_t* __restrict__ sst, const uint32_t* __restrict__ rawlen,
                                                                const uint32_t* __restrict__ fl, uint8_t* out, const uint64_t* __restrict__ out_off) {
    ZMI_DYN_SMEM(smem);          // TIFF_LDS bytes: one trip and the slack of zmi_load32u
    const uint32_t lane = threadIdx.x;
    const uint64_t total = item_off[n_sel];
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        uint32_t lo = 0u, hi = n_sel;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (item_off[mid] <= it) lo = mid; else hi = mid;
        }
        const uint32_t j = lo;
        const uint32_t group = (uint32_t)(it - item_off[j]);
        tf_slot s;
        tf_slot_of(pages, n_pages, page, sel, j, L, assemble, &s);
        if (s.kind != 0u) continue;
        const bool sparse = (fl[j] & TIFF_FL_SPARSE) != 0u;
        const bool raw = s.p.compression == 1u;
        const bool good = sparse || (raw ? rawlen[j] != 0u : (ssz[j] != 0u && sst[j] == 0 && slen[j] == ssz[j]));
        if (!good) continue;        // the slot reports why
        const uint32_t S = s.p.sample_bytes, spp = s.p.samples, pred = s.p.predictor;
        const bool be = s.p.big_endian != 0u;
        const uint32_t rb = s.p.seg_w * s.pb, n_dst = s.ow * s.pb;
        const uint32_t N = s.p.seg_w * spp;
        uint8_t* seg = sbuf + soff[j];
        uint8_t* dst0 = out + out_off[j];
        const uint32_t r1 = (group + 1u) * TIFF_ROWS < s.oh ? (group + 1u) * TIFF_ROWS : s.oh;
        for (uint32_t r = group * TIFF_ROWS; r < r1; ++r) {
            uint8_t* src = seg + (uint64_t)r * rb;
            uint8_t* dst = dst0 + (uint64_t)r * s.opitch;
            if (sparse) {
                for (uint32_t i = lane; i < n_dst; i += 64u) dst[i] = 0u;
            } else if (pred == 3u) {
                tf_scan_row<1u>(smem, src, src, rb, rb, spp, false, lane);
                __threadfence_block();      // the scanned bytes, stored by other lanes of this wave, are read back below
                zmi_wave_sync();
                if (S == 2u) tf_gather_row<2u>(src, dst, N, s.ow * spp, lane);
                else if (S == 4u) tf_gather_row<4u>(src, dst, N, s.ow * spp, lane);
                else tf_gather_row<8u>(src, dst, N, s.ow * spp, lane);
            } else {
                const uint32_t st = pred == 2u ? spp : 0u;
                if (S == 1u) tf_scan_row<1u>(smem, src, dst, rb, n_dst, st, be, lane);
                else if (S == 2u) tf_scan_row<2u>(smem, src, dst, rb, n_dst, st, be, lane);
                else if (S == 4u) tf_scan_row<4u>(smem, src, dst, rb, n_dst, st, be, lane);
                else tf_scan_row<8u>(smem, src, dst, rb, n_dst, st, be, lane);
            }
        }
    }
}

// One thread per slot, behind everything else: the slot's final words (include/zmi355.h states the order).
__global__ void __launch_bounds__(256) zmi_tiff_finish_kernel(const zmi_tiff_page* __restrict__ pages, uint32_t n_pages, uint32_t page,
                                                              const uint32_t* __restrict__ sel, uint32_t n_sel, uint64_t L, uint32_t assemble,
                                                              uint64_t out_cap, uint64_t decoded_bytes, const uint64_t* __restrict__ pix_off,
                                                              const uint64_t* __restrict__ out_off, const uint32_t* __restrict__ ssz,
                                                              const uint32_t* __restrict__ slen, const int32_t* __restrict__ sst,
                                                              const uint32_t* __restrict__ fl, uint32_t* __restrict__ out_len,
                                                              int32_t* __restrict__ status, int32_t* __restrict__ detail) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n_sel) return;
    tf_slot s;
    tf_slot_of(pages, n_pages, page, sel, j, L, assemble, &s);
    int32_t st = 0, det = 0;
    uint32_t n = 0u;
    if (pix_off[n_sel] > decoded_bytes || s.kind == 3u) st = TIFF_E_ARG;
    else if (s.kind == 2u) { det = s.p.status; st = (det == ZMI_TP_TAGS || det == ZMI_TP_FORMAT) ? ZMI_DATA_ERROR : TIFF_VERSION_ERROR; }
    else {
        n = (uint32_t)((uint64_t)s.oh * s.ow * s.pb);
        const uint32_t f = fl[j];
        const int32_t ds = sst[j];
        const bool fits = assemble ? s.image <= out_cap : out_off[j] + (uint64_t)n <= out_cap;
        if (!fits) { st = ZMI_BUF_ERROR; det = ZMI_TE_OUT; }
        else if (f & TIFF_FL_BOUNDS) { st = ZMI_DATA_ERROR; det = ZMI_TE_BOUNDS; }
        else if (f & TIFF_FL_SPARSE) det = ZMI_TE_SPARSE;
        else if (s.p.compression == 1u) { if (f & TIFF_FL_RAWLEN) { st = ZMI_DATA_ERROR; det = ZMI_TE_LENGTH; } }
        else if (ds == ZMI_BUF_ERROR) { st = ZMI_DATA_ERROR; det = ZMI_TE_LENGTH; }     // the stream wants more input, or more room than the segment
        else if (ds != ZMI_OK) { st = ds == TIFF_MEM_ERROR ? TIFF_MEM_ERROR : ZMI_DATA_ERROR; det = ZMI_TE_DATA; }
        else if (slen[j] != ssz[j]) { st = ZMI_DATA_ERROR; det = ZMI_TE_LENGTH; }
    }
    status[j] = st;
    detail[j] = det;
    out_len[j] = st == 0 ? n : 0u;
}

extern "C" uint32_t zmi_tiff_row_tile(void) { return TIFF_ROW_TILE; }
extern "C" int zmi_launch_tiff_directory(const uint8_t* d_in, uint64_t in_len, zmi_tiff_page* d_pages, uint32_t cap, zmi_tiff_info* d_info,
                                         uint64_t* d_ifd_pos, hipStream_t stream) {
    ZMI_LAUNCH(zmi_tiff_chain_kernel, dim3(1), dim3(64), 0, stream, d_in, in_len, cap, d_info, d_ifd_pos);
    if (cap == 0u) return 0;
    ZMI_LAUNCH(zmi_tiff_pages_kernel, dim3((cap + 63u) / 64u), dim3(64), 0, stream, d_in, in_len, (const zmi_tiff_info*)d_info,
               (const uint64_t*)d_ifd_pos, cap, d_pages);
    return 0;
}
extern "C" int zmi_launch_tiff_slots(const uint8_t* d_in, uint64_t in_len, const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page,
                                     const uint32_t* d_sel, uint32_t n_sel, uint32_t assemble, uint32_t pass, uint64_t out_cap, uint64_t decoded_bytes,
                                     const uint64_t* d_pix_off, uint32_t* d_pix, uint32_t* d_pcap, uint64_t* d_zin_off, uint32_t* d_zin_len,
                                     uint32_t* d_ssz, uint32_t* d_rawlen, uint32_t* d_items, uint32_t* d_fl, uint64_t* d_out_off, hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_tiff_slots_kernel, dim3((n_sel + 255u) / 256u), dim3(256), 0, stream, d_in, in_len, d_pages, n_pages, page, d_sel, n_sel, assemble,
               pass, out_cap, decoded_bytes, d_pix_off, d_pix, d_pcap, d_zin_off, d_zin_len, d_ssz, d_rawlen, d_items, d_fl, d_out_off);
    return 0;
}
// bound: the most row groups the call can have (decoded_bytes / TIFF_ROWS and one a slot); a fixed grid takes them in turn
extern "C" int zmi_launch_tiff_unpredict(const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page, const uint32_t* d_sel, uint32_t n_sel,
                                         uint64_t in_len, uint32_t assemble, const uint64_t* d_item_off, uint64_t bound, uint8_t* d_sbuf,
                                         const uint64_t* d_soff, const uint32_t* d_ssz, const uint32_t* d_slen, const int32_t* d_sst,
                                         const uint32_t* d_rawlen, const uint32_t* d_fl, uint8_t* d_out, const uint64_t* d_out_off, hipStream_t stream) {
    if (n_sel == 0) return 0;
    const uint32_t grid = bound < 1u ? 1u : (bound > 8192u ? 8192u : (uint32_t)bound);
    ZMI_LAUNCH(zmi_tiff_unpredict_kernel, dim3(grid), dim3(64), TIFF_LDS, stream, d_pages, n_pages, page, d_sel, n_sel, in_len, assemble, d_item_off,
               d_sbuf, d_soff, d_ssz, d_slen, d_sst, d_rawlen, d_fl, d_out, d_out_off);
    return 0;
}
extern "C" int zmi_launch_tiff_finish(const zmi_tiff_page* d_pages, uint32_t n_pages, uint32_t page, const uint32_t* d_sel, uint32_t n_sel,
                                      uint64_t in_len, uint32_t assemble, uint64_t out_cap, uint64_t decoded_bytes, const uint64_t* d_pix_off,
                                      const uint64_t* d_out_off, const uint32_t* d_ssz, const uint32_t* d_slen, const int32_t* d_sst,
                                      const uint32_t* d_fl, uint32_t* d_out_len, int32_t* d_status, int32_t* d_detail, hipStream_t stream) {
    if (n_sel == 0) return 0;
    ZMI_LAUNCH(zmi_tiff_finish_kernel, dim3((n_sel + 255u) / 256u), dim3(256), 0, stream, d_pages, n_pages, page, d_sel, n_sel, in_len, assemble,
               out_cap, decoded_bytes, d_pix_off, d_out_off, d_ssz, d_slen, d_sst, d_fl, d_out_len, d_status, d_detail);
    return 0;
}
